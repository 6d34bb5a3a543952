"""CPU: --lora_target_modules on the host side. The float64 restatement of tests/lora_modules_ref.py against the goldens the
reference's own training forward produced, PEFT adapter files (what is accepted, what is refused by name), the flag, and
the adapter a training run writes read back by the loader."""
import json
import os

import numpy as np
import pytest
import torch

from tests import lora_modules_ref as R

CASES = [(n, t) for n in ("tiny_hd128", "tiny_gqa") for t in ("all7", "kod")]


def load_case(golden_dir, name, tag):
    from llamarec_amd.synth import synth_llama_state

    z = np.load(os.path.join(golden_dir, f"llama_lora_modules_{name}_{tag}.npz"))
    cfg = json.loads(str(z["config"]))
    mods = tuple(str(m) for m in z["modules"])
    return z, cfg, synth_llama_state(cfg, int(z["weight_seed"])), mods, R.lora_init(cfg, int(z["weight_seed"]), mods)


def unpack(z, step):
    lens = z[f"step{step}/lens"]
    cu = np.concatenate([[0], np.cumsum(lens)])
    ids, lab = z[f"step{step}/packed_ids"], z[f"step{step}/packed_labels"]
    return [ids[cu[i]:cu[i + 1]] for i in range(len(lens))], [lab[cu[i]:cu[i + 1]] for i in range(len(lens))]


@pytest.mark.parametrize("name,tag", CASES)
def test_float64_restatement_reproduces_the_reference(golden_dir, name, tag):
    """float64 here vs the reference's fp32 run. Measured on these four cases: loss within 2.5e-7, every gradient tensor
    within 1.4e-6 relative L2 (fp32 accumulation over at most 131 tokens); the bars are one order of magnitude above."""
    z, cfg, sd, mods, lora = load_case(golden_dir, name, tag)
    seqs, labels = unpack(z, 0)
    loss, grads, _ = R.loss_and_grads(sd, cfg, lora, seqs, labels, int(z["lora_r"]), float(z["lora_alpha"]))
    assert abs(loss - float(z["step0/loss"])) < 2.5e-6
    assert sorted(grads) == sorted(str(n) for n in z["param_names"])
    assert {k.split(".")[2] for k in grads} == set(mods)
    for n, g in grads.items():
        assert np.abs(g).max() > 0, n                       # B != 0: every A has a gradient
        assert R.rel(z["step0/grad/" + n], g) < 1.5e-5, (n, R.rel(z["step0/grad/" + n], g))


# ---- PEFT adapter files ------------------------------------------------------------------------------------------------
CFG = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
           num_key_value_heads=2, rms_norm_eps=1e-5)


def write_adapter(path, modules, r=4, alpha=8, config=None, extra=None, drop=()):
    from safetensors.torch import save_file

    from llamarec_amd.rank_train import adapter_config, lora_shapes, peft_key

    os.makedirs(path, exist_ok=True)
    ac = adapter_config(r, alpha, modules) if config is None else config
    json.dump(ac, open(os.path.join(path, "adapter_config.json"), "w"))
    g = torch.Generator().manual_seed(0)
    t = {}
    for (mod, ab), shape in lora_shapes(CFG, r, modules).items():
        for l in range(CFG["num_hidden_layers"]):
            t[peft_key(l, mod, ab)] = torch.randn(shape, generator=g)
    t.update(extra or {})
    for k in drop:
        del t[k]
    save_file(t, os.path.join(path, "adapter_model.safetensors"))
    return t


def test_save_adapter_files_round_trip_through_the_loader(tmp_path):
    """The config and the key / shape mapping LoraTrainEngine.save_adapter writes (adapter_config, peft_key, lora_shapes are
    the pure functions it calls) come back through load_peft_adapter as from_state_dict's `lora` argument."""
    from llamarec_amd.llm import LORA_MODULE_BLOCK, load_peft_adapter

    for modules in (("q_proj", "v_proj"), ["all-linear"], ("down_proj", "k_proj", "o_proj")):
        d = str(tmp_path / "-".join(modules))
        t = write_adapter(d, modules)
        ac = json.load(open(os.path.join(d, "adapter_config.json")))
        want = tuple(LORA_MODULE_BLOCK) if "all-linear" in modules else tuple(m for m in LORA_MODULE_BLOCK if m in modules)
        assert tuple(ac["target_modules"]) == want        # the real modules, no longer the literal q/v
        lora = load_peft_adapter(d)
        assert (lora["r"], lora["alpha"], lora["target_modules"]) == (4, 8, want)
        assert len(lora["weights"]) == len(t) == 2 * 2 * len(want)
        for mod in want:
            blk = LORA_MODULE_BLOCK[mod]
            for l in range(2):
                for ab in "AB":
                    k = f"model.layers.{l}.{blk}.{mod}.lora_{ab}.weight"
                    src = t[f"base_model.model.model.layers.{l}.{blk}.{mod}.lora_{ab}.weight"]
                    assert np.array_equal(lora["weights"][k], src.numpy()), k
        a, b = lora["weights"]["model.layers.1.self_attn.k_proj.lora_A.weight"] if "k_proj" in want else None, None
        if a is not None:
            assert a.shape == (4, 64)
            assert lora["weights"]["model.layers.1.self_attn.k_proj.lora_B.weight"].shape == (32, 4)


def test_loader_accepts_all_linear_string_sparse_config_and_default_adapter_name(tmp_path):
    from safetensors.torch import load_file, save_file

    from llamarec_amd.llm import LORA_MODULE_BLOCK, load_peft_adapter

    d = str(tmp_path / "a")
    t = write_adapter(d, ["all-linear"], config={"r": 4, "lora_alpha": 8, "target_modules": "all-linear"})
    assert len(t) == 28 and load_peft_adapter(d)["target_modules"] == tuple(LORA_MODULE_BLOCK)
    d2 = str(tmp_path / "b")
    write_adapter(d2, ("o_proj",), config={"r": 4, "lora_alpha": 8})          # no target_modules at all: the keys decide
    lora = load_peft_adapter(d2)
    assert lora["target_modules"] is None and len(lora["weights"]) == 4
    # keys that carry peft's adapter name (".lora_A.default.weight", as in a state_dict saved without peft's own renaming)
    f = os.path.join(d2, "adapter_model.safetensors")
    named = {k.replace(".lora_A.weight", ".lora_A.default.weight").replace(".lora_B.weight", ".lora_B.default.weight"): v
             for k, v in load_file(f).items()}
    assert all(".default." in k for k in named)
    save_file(named, f)
    again = load_peft_adapter(d2)
    assert sorted(again["weights"]) == sorted(lora["weights"])
    assert all(np.array_equal(again["weights"][k], lora["weights"][k]) for k in lora["weights"])


REFUSALS = [
    ({"peft_type": "IA3"}, "peft_type"),
    ({"peft_type": "ADALORA"}, "peft_type"),
    ({"use_dora": True}, "use_dora"),
    ({"use_rslora": True}, "use_rslora"),
    ({"rank_pattern": {"q_proj": 16}}, "rank_pattern"),
    ({"alpha_pattern": {"q_proj": 16}}, "alpha_pattern"),
    ({"bias": "all"}, "bias"),
    ({"bias": "lora_only"}, "bias"),
    ({"fan_in_fan_out": True}, "fan_in_fan_out"),
    ({"modules_to_save": ["lm_head"]}, "modules_to_save"),
    ({"target_modules": ["qkv_proj"]}, "qkv_proj"),
    ({"target_modules": ["q_proj", "lm_head"]}, "lm_head"),
]


@pytest.mark.parametrize("field,needle", REFUSALS, ids=[f"{list(f)[0]}={list(f.values())[0]}" for f, _ in REFUSALS])
def test_loader_refuses_what_it_cannot_merge_by_name(tmp_path, field, needle):
    from llamarec_amd.llm import load_peft_adapter
    from llamarec_amd.rank_train import adapter_config

    ok = adapter_config(4, 8, ("q_proj", "v_proj"))
    write_adapter(str(tmp_path), ("q_proj", "v_proj"), config=dict(ok, **field))
    with pytest.raises(NotImplementedError, match=needle):
        load_peft_adapter(str(tmp_path))
    # PEFT's defaults for the same fields are accepted
    write_adapter(str(tmp_path), ("q_proj", "v_proj"), config=dict(ok, use_dora=False, use_rslora=False, rank_pattern={},
                                                                    alpha_pattern={}, modules_to_save=None))
    assert load_peft_adapter(str(tmp_path))["r"] == 4


@pytest.mark.parametrize("key", ["base_model.model.lm_head.lora_A.weight",
                                 "base_model.model.model.embed_tokens.lora_embedding_A",
                                 "base_model.model.model.layers.0.self_attn.qkv_proj.lora_A.weight",
                                 "base_model.model.model.layers.0.mlp.q_proj.lora_A.weight"])
def test_loader_refuses_tensors_that_map_to_no_decoder_linear(tmp_path, key):
    from llamarec_amd.llm import load_peft_adapter

    write_adapter(str(tmp_path), ("q_proj",), config={"r": 4, "lora_alpha": 8}, extra={key: torch.zeros(4, 64)})
    with pytest.raises(NotImplementedError, match="maps to no Linear"):
        load_peft_adapter(str(tmp_path))


def test_loader_refuses_inconsistent_files(tmp_path):
    from llamarec_amd.llm import load_peft_adapter
    from llamarec_amd.rank_train import adapter_config, peft_key

    write_adapter(str(tmp_path / "a"), ("q_proj", "o_proj"), config=adapter_config(4, 8, ("q_proj",)))
    with pytest.raises(ValueError, match="target_modules"):      # a tensor of a module the config does not name
        load_peft_adapter(str(tmp_path / "a"))
    write_adapter(str(tmp_path / "b"), ("q_proj",), drop=[peft_key(1, "q_proj", "B")])
    with pytest.raises(ValueError, match="partner"):
        load_peft_adapter(str(tmp_path / "b"))
    write_adapter(str(tmp_path / "c"), ("q_proj",), config=adapter_config(8, 8, ("q_proj",)))
    with pytest.raises(ValueError, match="rank 8"):
        load_peft_adapter(str(tmp_path / "c"))


# ---- the flag ------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_all_linear_expands():
    from llamarec_amd import config as cfg
    from llamarec_amd._abi import LORA_MODULES
    from llamarec_amd.llm import expand_target_modules as normalize_target_modules

    base = ["--dataset_code", "ml-100k"]
    a = cfg.parse(base, model_code="llm")
    assert a.lora_target_modules == ["q_proj", "v_proj"] and isinstance(a.lora_target_modules, list)
    a = cfg.parse(base + ["--lora_target_modules", "k_proj", "down_proj"], model_code="llm")
    assert a.lora_target_modules == ["k_proj", "down_proj"]
    assert normalize_target_modules(a.lora_target_modules) == ("k_proj", "down_proj")
    a = cfg.parse(base + ["--lora_target_modules", "all-linear"], model_code="llm")
    assert tuple(a.lora_target_modules) == tuple(m for m in normalize_target_modules(["all-linear"]))
    assert set(a.lora_target_modules) == set(LORA_MODULES) and len(a.lora_target_modules) == 7
    assert normalize_target_modules(["up_proj", "q_proj"]) == ("q_proj", "up_proj")     # the kernels' order
    with pytest.raises(SystemExit):
        cfg.parse(base + ["--lora_target_modules", "qkv_proj"], model_code="llm")       # phi-3's fused projection
    with pytest.raises(NotImplementedError, match="qkv_proj"):
        normalize_target_modules(["qkv_proj"])
