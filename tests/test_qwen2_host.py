"""Host side of the Qwen2 ranker (--llm qwen2), no GPU: the committed goldens against the fp32 restatement, config dispatch and
its refusals, presets, the sliding-window rule, the q/k/v biases in wqkv's row order, synth_qwen2_state's names, train_ranker's
refusal to train a Qwen2 base, and the declarations of the new C calls."""
import json
import os
import re

import numpy as np
import pytest
import torch

from llamarec_amd.synth import synth_qwen2_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QWEN2_GOLDENS = ("hd64_ragged", "hd128_gqa", "hd16")


def load_qwen2_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"qwen2_tiny_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_qwen2_state(cfg, int(z["weight_seed"]), std=float(z["weight_std"]), bias_std=float(z["bias_std"]),
                           v_bias_std=float(z["v_bias_std"]))
    T = z["input_ids"].shape[1]
    seqs = [z["input_ids"][b, T - n:] for b, n in enumerate(z["lens"])]
    return z, cfg, sd, seqs


@pytest.mark.parametrize("name", QWEN2_GOLDENS)
def test_restatement_matches_the_reference_goldens(golden_dir, name):
    """tests/qwen2_ref.py in fp32 sits on the reference's fp32 logits (padded and unpadded), its bf16 run within the archive's
    tolerance, and each misreading of the biases is at least ten tolerances away."""
    from tests import qwen2_ref as QR
    from tests.gen_goldens_qwen2 import golden_tolerance

    z, cfg, sd, seqs = load_qwen2_golden(golden_dir, name)
    assert cfg["model_type"] == "qwen2" and "model.layers.0.self_attn.q_proj.bias" in sd
    assert ("lm_head.weight" in sd) == (not cfg["tie_word_embeddings"])
    assert list(z["lens"]) == [37, 5, 64, 1, 20, 130] and float(z["eval_loss"]) == -1.0 and sum(z["lens"]) == 257
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    got = QR.last_logits(sd, cfg, seqs)
    scale = max(1.0, float(np.abs(z["logits_fp32"]).max()))
    assert np.abs(got - z["logits_fp32"]).max() < 1e-4 * scale
    assert np.abs(got - z["logits_fp32_unpadded"]).max() < 1e-4 * scale
    assert np.abs(QR.last_logits(sd, cfg, seqs, torch.bfloat16) - z["logits_bf16"]).max() < tol
    for mutant in QR.QWEN2_MUTANTS:
        assert np.abs(QR.last_logits(sd, cfg, seqs, mutant=mutant) - z["logits_fp32"]).max() >= 10 * tol, mutant
    assert np.array_equal(z["scores_fp32"], z["logits_fp32"][:, z["label_ids"]])


def test_qwen2_model_type_dispatch_needs_a_complete_config():
    from llamarec_amd.llm import (LLAMA2_7B, LLAMA3_ROPE_SCALING, QWEN2_0_5B, QWEN2_1_5B, QWEN2_7B, QWEN2_FAMILY,
                                  QWEN2_REQUIRED_KEYS, SUPPORTED_MODEL_TYPES, LlamaRanker, model_family)

    assert QWEN2_FAMILY == ("qwen2",) and "qwen2" in SUPPORTED_MODEL_TYPES
    for preset in (QWEN2_0_5B, QWEN2_1_5B, QWEN2_7B):
        assert model_family(preset) == "qwen2"
    assert model_family(dict(QWEN2_0_5B, sliding_window=None)) == "qwen2"                  # null with use_sliding_window false
    assert model_family(dict(QWEN2_0_5B, head_dim=64)) == "qwen2"
    assert model_family(dict(QWEN2_0_5B, rope_scaling={"rope_type": "default"})) == "qwen2"
    assert QWEN2_REQUIRED_KEYS == ("hidden_act", "use_sliding_window", "sliding_window", "max_window_layers")
    for key in QWEN2_REQUIRED_KEYS:
        cfg = {k: v for k, v in QWEN2_0_5B.items() if k != key}
        with pytest.raises(NotImplementedError, match=rf"'qwen2'.*{key}.*supported families"):
            model_family(cfg)
        with pytest.raises(NotImplementedError, match=key):
            LlamaRanker(cfg, device="cpu")
    with pytest.raises(NotImplementedError, match=r"'qwen2'.*hidden_act, use_sliding_window, sliding_window, max_window_layers.*"
                                                  r"supported families"):
        model_family(dict(LLAMA2_7B, model_type="qwen2"))                                    # a Llama config relabelled
    for bad, pattern in [(dict(hidden_act="gelu"), "hidden_act='gelu'"),
                         (dict(hidden_act=None), "hidden_act"),
                         (dict(rope_scaling={"type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}), "yarn"),
                         (dict(rope_scaling={"rope_type": "dynamic", "factor": 2.0}), "dynamic"),
                         (dict(rope_scaling=dict(LLAMA3_ROPE_SCALING)), "llama3"),
                         (dict(head_dim=128), "head_dim=128"),
                         (dict(use_sliding_window=None), "use_sliding_window"),
                         (dict(use_sliding_window=True, sliding_window=0), "sliding_window=0"),
                         (dict(use_sliding_window=True, sliding_window=None), "sliding_window=None")]:
        with pytest.raises(NotImplementedError, match=pattern) as e:
            model_family(dict(QWEN2_0_5B, **bad))
        assert "qwen2" in str(e.value), bad


def test_qwen2_presets():
    from llamarec_amd.llm import QWEN2_0_5B, QWEN2_1_5B, QWEN2_7B, LlamaRanker

    want = {"0.5B": (QWEN2_0_5B, 896, 4864, 24, 14, 2, True, 151936, 64), "1.5B": (QWEN2_1_5B, 1536, 8960, 28, 12, 2, True, 151936, 128),
            "7B": (QWEN2_7B, 3584, 18944, 28, 28, 4, False, 152064, 128)}
    for name, (c, d, f, nl, nh, nkv, tied, vocab, hd) in want.items():
        assert (c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["num_attention_heads"],
                c["num_key_value_heads"], c["tie_word_embeddings"], c["vocab_size"]) == (d, f, nl, nh, nkv, tied, vocab), name
        assert c["rope_theta"] == 1e6 and c["rms_norm_eps"] == 1e-6 and c["hidden_act"] == "silu"
        r = LlamaRanker(c, device="cpu")
        assert r.family == "qwen2" and r.hd == hd and r.rope_scaling is None and r.rope_theta == 1e6 and r.max_prompt_len is None
        assert r.default_gemm_variant == 6
        a = r.arch()
        assert (a.norm_style, a.mlp_act, a.embed_scale) == (0, 0, 1.0)
    # Qwen2-0.5B: three of a layer's four products miss the 256-column tile but sit on 64 columns; 1.5B and 7B fit the tile
    shapes = lambda c, hd: ((c["num_attention_heads"] + 2 * c["num_key_value_heads"]) * hd, c["hidden_size"], 2 * c["intermediate_size"])  # noqa: E731
    assert [n % 256 for n in shapes(QWEN2_0_5B, 64)] == [128, 128, 0] and all(n % 64 == 0 for n in shapes(QWEN2_0_5B, 64))
    assert QWEN2_0_5B["hidden_size"] % 64 == 0 and QWEN2_0_5B["intermediate_size"] % 64 == 0
    for c in (QWEN2_1_5B, QWEN2_7B):
        assert all(n % 256 == 0 for n in shapes(c, 128))
    from llamarec_amd.llm import LLAMA2_7B, PHI3_MINI
    assert LlamaRanker(LLAMA2_7B, device="cpu").default_gemm_variant == 0 and LlamaRanker(PHI3_MINI, device="cpu").default_gemm_variant == 0


def test_qwen2_window_rule_follows_use_sliding_window():
    from llamarec_amd.llm import QWEN2_0_5B, LlamaRanker

    r = LlamaRanker(dict(QWEN2_0_5B, use_sliding_window=True, sliding_window=100), device="cpu")
    assert r.max_prompt_len == 100
    with pytest.raises(NotImplementedError, match="Qwen2's sliding window of 100"):
        r._check_lengths(np.array([0, 50, 151], np.int32))
    r._check_lengths(np.array([0, 100, 150], np.int32))
    off = LlamaRanker(dict(QWEN2_0_5B, use_sliding_window=False, sliding_window=100), device="cpu")
    assert off.max_prompt_len is None
    off._check_lengths(np.array([0, 5000], np.int32))                                        # the window is ignored


def _tensors_of(monkeypatch, sd, cfg, **kw):
    from llamarec_amd.llm import LlamaRanker

    monkeypatch.setattr(LlamaRanker, "_create", lambda self: None)
    return LlamaRanker.from_state_dict(sd, cfg, device="cpu", **kw)._tensors


def _tiny_cfg():
    from llamarec_amd.synth import QWEN2_TINY

    return dict(QWEN2_TINY, vocab_size=64, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=64)


def test_biases_are_stored_in_wqkv_row_order(monkeypatch):
    """q_proj.bias[i] = i at head_dim 64: the stored bias starts 0, 32, 1, 33 (the weight rows' pair interleave), every head
    alike, k's part the same, and v's part in HF's order. The weight rows and the bias move together."""
    cfg = _tiny_cfg()
    nh, nkv, hd, d = 4, 2, 64, 256
    sd = synth_qwen2_state(cfg, 3)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}.self_attn."
        sd[p + "q_proj.bias"] = np.arange(nh * hd, dtype=np.float32)
        sd[p + "k_proj.bias"] = 0.5 + np.arange(nkv * hd, dtype=np.float32)       # exact in bf16, like the rest
        sd[p + "v_proj.bias"] = -np.arange(nkv * hd, dtype=np.float32)
        sd[p + "q_proj.weight"] = sd[p + "q_proj.weight"].copy()
        sd[p + "q_proj.weight"][:, 0] = np.arange(nh * hd)
    T = _tensors_of(monkeypatch, sd, cfg)
    b = T["0.bqkv"]
    assert b.dtype == torch.bfloat16 and b.shape == ((nh + 2 * nkv) * hd,) and b.is_contiguous()
    b = b.float()
    assert b[:4].tolist() == [0.0, 32.0, 1.0, 33.0] and b[hd: hd + 4].tolist() == [64.0, 96.0, 65.0, 97.0]
    assert b[nh * hd: nh * hd + 4].tolist() == [0.5, 32.5, 1.5, 33.5]
    assert torch.equal(b[(nh + nkv) * hd:], -torch.arange(nkv * hd, dtype=torch.float32))
    assert torch.equal(T["0.wqkv"].float()[: nh * hd, 0], b[: nh * hd])                        # rows and bias: one permutation
    assert "lm_head.weight" not in sd and T["lm_head"] is T["embed"]                            # the tied head
    assert sorted(k for k in T if k.startswith("1.")) == sorted(f"1.{n}" for n in ("wqkv", "bqkv", "wo", "wgu", "wdown", "input_norm", "post_norm"))


def test_a_missing_bias_is_an_error_that_names_it(monkeypatch):
    cfg = _tiny_cfg()
    sd = synth_qwen2_state(cfg, 3)
    for n in "qkv":
        key = f"model.layers.1.self_attn.{n}_proj.bias"
        with pytest.raises(KeyError, match=re.escape(key)):
            _tensors_of(monkeypatch, {k: v for k, v in sd.items() if k != key}, cfg)
    # the same tensors relabelled llama load without their biases: only the family decides
    llama = _tensors_of(monkeypatch, dict(sd, **{"lm_head.weight": sd["model.embed_tokens.weight"]}),
                        {k: v for k, v in cfg.items() if k != "model_type"})
    assert "0.bqkv" not in llama


def test_an_adapter_changes_wqkv_and_leaves_the_bias_alone(monkeypatch):
    cfg = _tiny_cfg()
    d, nkv, hd = 256, 2, 64
    sd = synth_qwen2_state(cfg, 4)
    rng = np.random.default_rng(0)
    w = {}
    for i in range(cfg["num_hidden_layers"]):
        for m, rows in (("q_proj", d), ("v_proj", nkv * hd)):
            base = f"model.layers.{i}.self_attn.{m}"
            w[base + ".lora_A.weight"] = rng.standard_normal((8, d)).astype(np.float32) * 0.1
            w[base + ".lora_B.weight"] = rng.standard_normal((rows, 8)).astype(np.float32) * 0.1
    plain = _tensors_of(monkeypatch, sd, cfg)
    tuned = _tensors_of(monkeypatch, sd, cfg, lora=dict(r=8, alpha=32, weights=w))
    for i in range(cfg["num_hidden_layers"]):
        assert torch.equal(tuned[f"{i}.bqkv"], plain[f"{i}.bqkv"])
        dq = (tuned[f"{i}.wqkv"].float() - plain[f"{i}.wqkv"].float()).abs().amax(1)
        assert (dq[:d] > 0).all() and (dq[d: d + nkv * hd] == 0).all() and (dq[d + nkv * hd:] > 0).all()   # q and v rows, not k
        assert torch.equal(tuned[f"{i}.wo"], plain[f"{i}.wo"])


def test_synth_qwen2_state_has_the_bias_names_and_shapes():
    from llamarec_amd.synth import QWEN2_TINY, qwen2_param_shapes

    c = QWEN2_TINY
    assert (c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], c["intermediate_size"], c["num_hidden_layers"],
            c["tie_word_embeddings"]) == (896, 14, 2, 1280, 2, True)
    names = dict(qwen2_param_shapes(c))
    assert names["model.layers.1.self_attn.q_proj.weight"] == (896, 896) and names["model.layers.1.self_attn.q_proj.bias"] == (896,)
    assert names["model.layers.1.self_attn.k_proj.bias"] == (128,) and names["model.layers.1.self_attn.v_proj.bias"] == (128,)
    assert not any(n.endswith("bias") and ("o_proj" in n or "mlp" in n) for n in names) and "lm_head.weight" not in names
    assert "lm_head.weight" in dict(qwen2_param_shapes(dict(c, tie_word_embeddings=False)))
    sd = synth_qwen2_state(c, 7)
    assert sorted(sd) == sorted(names) and all(sd[n].shape == s for n, s in names.items())
    bias = sd["model.layers.0.self_attn.q_proj.bias"]
    assert 0.4 < bias.std() < 0.6 and abs(bias.mean()) < 0.1                                   # U(0.5), not 1 + jitter
    assert abs(sd["model.layers.0.input_layernorm.weight"].mean() - 1.0) < 0.05
    narrow = synth_qwen2_state(c, 7, v_bias_std=0.1)
    assert narrow["model.layers.0.self_attn.v_proj.bias"].std() < 0.12
    assert np.array_equal(narrow["model.layers.0.self_attn.k_proj.bias"], sd["model.layers.0.self_attn.k_proj.bias"])


def test_train_ranker_refuses_to_train_a_qwen2_base(tmp_path):
    import train_ranker

    assert "Qwen2" in train_ranker.TRAIN_LLAMA_ONLY and "Phi-3" in train_ranker.TRAIN_LLAMA_ONLY
    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "qwen2", "--llm_retrieved_path", str(tmp_path)])


def test_new_symbols_are_declared_and_prototyped():
    import ctypes as C

    from llamarec_amd import _lib

    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    for name in ("lr_llama_set_qkv_bias", "lr_gemm_bf16_nt_bias_epi"):
        assert name in _lib.PROTOTYPES and re.search(rf"\bint {name}\(", header), name
    assert _lib.PROTOTYPES["lr_llama_set_qkv_bias"] == (C.c_int, [C.c_void_p, C.c_void_p])
    epi, bias = _lib.PROTOTYPES["lr_gemm_bf16_nt_epi"][1], _lib.PROTOTYPES["lr_gemm_bf16_nt_bias_epi"][1]
    assert bias == epi[:-1] + [C.c_void_p, C.c_void_p]                                       # ..., bias, hip_stream
    assert "gemm 6" in header
    if os.path.exists(_lib.LIB_PATH):
        l = _lib.lib()
        assert hasattr(l, "lr_llama_set_qkv_bias") and hasattr(l, "lr_gemm_bf16_nt_bias_epi")
