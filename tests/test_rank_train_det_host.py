"""Host side of the ranker's deterministic LoRA step (no GPU): the flag, the bound symbol, the engine's method."""
import ctypes as C
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deterministic_flag_parses_for_the_ranker():
    from llamarec_amd import config

    base = ["--dataset_code", "synthetic", "--llm_retrieved_path", "x"]
    assert config.parse(base + ["--deterministic"], model_code="llm").deterministic is True
    assert config.parse(base, model_code="llm").deterministic is False
    help_text = " ".join(config.build_parser().format_help().split())       # the flag's help names both entry points
    assert re.search(r"--deterministic .*train_retriever\.py.*train_ranker\.py", help_text)


def test_symbol_is_declared_and_bound_with_the_right_types():
    from llamarec_amd import _lib

    res, args = _lib.PROTOTYPES["lr_llama_lora_set_deterministic"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32]
    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    assert re.search(r"int\s+lr_llama_lora_set_deterministic\(lr_llama_lora_t\*\s*h,\s*int32_t\s+enable\);", header)


def test_engine_method_and_entry_point_call_it():
    from llamarec_amd.rank_train import LoraTrainEngine

    src = inspect.getsource(LoraTrainEngine.set_deterministic)
    assert "lr_llama_lora_set_deterministic" in src and "self._ws = None" in src   # the next call re-queries the size
    assert LoraTrainEngine.deterministic is False
    ranker = open(os.path.join(REPO, "train_ranker.py")).read()
    assert re.search(r"if args\.deterministic:.*\n\s+engine\.set_deterministic\(True\)", ranker)
