"""CPU: the Gemma-2 ranker's host side -- model_type dispatch and its complete-config rule, the extension words, parameter
shapes against HF, the window refusal, the training refusal, the golden generator's archive format, and the torch
restatement (tests/gemma2_ref.py) against the reference's goldens."""
import json
import os

import numpy as np
import pytest
import torch

from llamarec_amd.synth import gemma2_param_shapes, synth_gemma2_state

GEMMA2_GOLDENS = ("tiny_hd256_gqa", "tiny_hd256_qpas", "tiny_hd16")


def load_gemma2_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"gemma2_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_gemma2_state(cfg, int(z["weight_seed"]), std=float(z["weight_std"]))
    T = z["input_ids"].shape[1]
    seqs = [z["input_ids"][b, T - n:] for b, n in enumerate(z["lens"])]
    return z, cfg, sd, seqs


def test_gemma2_model_type_dispatch_needs_a_complete_config():
    from llamarec_amd.llm import GEMMA2_2B, GEMMA2_9B, GEMMA2_REQUIRED_KEYS, LLAMA3_ROPE_SCALING, LlamaRanker, model_family

    assert model_family(GEMMA2_2B) == "gemma2" and model_family(GEMMA2_9B) == "gemma2"
    assert model_family(dict(GEMMA2_2B, attn_logit_softcapping=None, final_logit_softcapping=None)) == "gemma2"   # caps may be null
    assert (GEMMA2_2B["num_hidden_layers"], GEMMA2_2B["num_attention_heads"], GEMMA2_2B["num_key_value_heads"]) == (26, 8, 4)
    assert (GEMMA2_9B["num_hidden_layers"], GEMMA2_9B["num_attention_heads"], GEMMA2_9B["num_key_value_heads"]) == (42, 16, 8)
    for key in GEMMA2_REQUIRED_KEYS:
        cfg = {k: v for k, v in GEMMA2_2B.items() if k != key}
        with pytest.raises(NotImplementedError, match=rf"'gemma2'.*{key}.*supported families: .*gemma2$"):
            model_family(cfg)
        with pytest.raises(NotImplementedError, match=key):
            LlamaRanker(cfg, device="cpu")
    for key in ("query_pre_attn_scalar", "sliding_window", "head_dim"):    # null is "missing" for everything but the caps
        with pytest.raises(NotImplementedError, match=key):
            model_family(dict(GEMMA2_2B, **{key: None}))
    with pytest.raises(NotImplementedError, match="hidden_activation.*supported families"):
        model_family(dict(GEMMA2_2B, hidden_activation="gelu"))
    with pytest.raises(NotImplementedError, match="rope_scaling.*supported families"):
        model_family(dict(GEMMA2_2B, rope_scaling=dict(LLAMA3_ROPE_SCALING)))
    with pytest.raises(NotImplementedError, match="rope_scaling"):
        model_family(dict(GEMMA2_2B, rope_scaling={"rope_type": "linear", "factor": 2.0}))
    with pytest.raises(NotImplementedError, match="attn_logit_softcapping"):
        model_family(dict(GEMMA2_2B, attn_logit_softcapping=-1.0))
    with pytest.raises(NotImplementedError, match="query_pre_attn_scalar"):     # a foreign scale needs the capped kernels
        model_family(dict(GEMMA2_2B, attn_logit_softcapping=None, query_pre_attn_scalar=144))
    assert model_family(dict(GEMMA2_2B, query_pre_attn_scalar=144)) == "gemma2"


def test_gemma2_extension_words():
    from llamarec_amd import _abi as A
    from llamarec_amd.llm import GEMMA2_2B, GEMMA2_9B, LlamaRanker
    import ctypes

    for cfg, embed_scale in ((GEMMA2_2B, 48.0), (GEMMA2_9B, 59.75)):    # bf16(sqrt(2304)), bf16(sqrt(3584))
        r = LlamaRanker(dict(cfg), device="cpu")
        a = r.arch()
        assert r.family == "gemma2" and r.hd == 256
        assert (a.norm_style, a.mlp_act, a.embed_scale, list(a.reserved)) == (1, 1, embed_scale, [0] * 5)
        e, arrs = r.gemma2_ext()
        assert (e.attn_softcap, e.final_softcap, e.attn_scale, list(e.reserved)) == (50.0, 30.0, 0.0625, [0] * 5)
        assert arrs is None and not e.attn_out_norm and not e.mlp_out_norm    # no weights loaded: no out-norm arrays
    e, _ = LlamaRanker(dict(GEMMA2_2B, query_pre_attn_scalar=144), device="cpu").gemma2_ext()    # gemma-2-27b's scalar
    assert e.attn_scale == np.float32(1.0 / 12.0)
    e, _ = LlamaRanker(dict(GEMMA2_2B, final_logit_softcapping=None), device="cpu").gemma2_ext()
    assert e.final_softcap == 0.0 and e.attn_softcap == 50.0
    assert ctypes.sizeof(A.LrGemma2Ext) == 48    # 3 floats + 5 reserved words + 2 pointers


def test_gemma2_param_shapes_equal_hf():
    from transformers import Gemma2Config, Gemma2ForCausalLM

    from tests.gen_goldens_gemma2 import gemma2_cfg_dict

    cd = gemma2_cfg_dict("tiny_hd16")
    kw = {k: v for k, v in cd.items() if k not in ("model_type", "rope_theta")}
    model = Gemma2ForCausalLM(Gemma2Config(**kw, tie_word_embeddings=True))
    hf = [(n, tuple(p.shape)) for n, p in model.named_parameters() if n != "lm_head.weight"]
    assert hf == gemma2_param_shapes(cd)
    sd = synth_gemma2_state(cd, 1)
    assert list(sd) == [n for n, _ in hf] and all(sd[n].shape == s for n, s in hf)


def test_gemma2_check_lengths_refuses_above_the_window():
    from llamarec_amd.llm import GEMMA2_2B, LlamaRanker

    r = LlamaRanker(dict(GEMMA2_2B, sliding_window=100), device="cpu")
    with pytest.raises(NotImplementedError, match="sliding window of 100"):
        r._check_lengths(np.array([0, 50, 151], np.int32))
    r._check_lengths(np.array([0, 100, 150], np.int32))
    with pytest.raises(NotImplementedError, match="folded"):
        r.set_fold_norms(True)


def test_train_ranker_refuses_to_train_a_gemma2_base(tmp_path):
    import train_ranker

    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma2", "--llm_retrieved_path",
                           str(tmp_path)])


def test_gemma2_llm_flag_keeps_the_reference_batch_sizes():
    from llamarec_amd import config as cfg

    a = cfg.parse(["--dataset_code", "beauty", "--llm", "gemma2"], model_code="llm")
    b = cfg.parse(["--dataset_code", "beauty", "--llm", "llama2"], model_code="llm")
    assert a.llm_base_model == "google/gemma-2-9b"
    assert (a.lora_micro_batch_size, a.test_batch_size, a.train_batch_size) == \
        (b.lora_micro_batch_size, b.test_batch_size, b.train_batch_size)       # the reference does not scale gemma2's


def test_gemma2_golden_archive_is_byte_stable(golden_dir, tmp_path):
    """The generator's writer gives the same bytes for the same arrays, and the committed archives carry its keys."""
    from tests.gen_goldens_gemma2 import GEMMA2_CONFIGS, golden_tolerance, save_npz_fixed

    assert tuple(GEMMA2_CONFIGS) == GEMMA2_GOLDENS
    z = np.load(os.path.join(golden_dir, "gemma2_tiny_hd16.npz"))
    arrays = {k: z[k] for k in z.files}
    save_npz_fixed(tmp_path / "one.npz", **arrays)
    save_npz_fixed(tmp_path / "two.npz", **arrays)
    assert (tmp_path / "one.npz").read_bytes() == (tmp_path / "two.npz").read_bytes()
    assert (tmp_path / "one.npz").read_bytes() == open(os.path.join(golden_dir, "gemma2_tiny_hd16.npz"), "rb").read()
    gz = np.load(os.path.join(golden_dir, "gemma_tiny_hd16.npz"))
    assert set(gz.files) <= set(z.files)
    assert golden_tolerance(np.zeros(3), np.full(3, 0.01)) == 3e-2 and golden_tolerance(np.zeros(3), np.full(3, 0.05)) == \
        pytest.approx(0.15)


@pytest.mark.parametrize("name", GEMMA2_GOLDENS)
def test_gemma2_restatement_matches_reference_goldens(golden_dir, name):
    from tests import gemma2_ref as G

    z, cfg, sd, seqs = load_gemma2_golden(golden_dir, name)
    assert cfg["model_type"] == "gemma2" and cfg["head_dim"] in (16, 256) and max(z["lens"]) < cfg["sliding_window"]
    l32 = G.last_logits(sd, cfg, seqs)
    # fp32 against fp32 on the unpadded prompts: the same operations in the same order up to the BLAS blocking. Measured on
    # the CPU: 2.4e-6 / 2.1e-6 / 8.3e-7 for the three archives at logit scales 7.84 / 7.81 / 3.88, i.e. at most 5 ulps of
    # the largest logit; the bound is 16 of them.
    ulp = float(np.spacing(np.float32(np.abs(z["logits_fp32_unpadded"]).max())))
    assert np.abs(l32 - z["logits_fp32_unpadded"]).max() <= 16 * ulp
    assert np.abs(l32 - z["logits_fp32"]).max() <= 64 * ulp          # the padded batch masks instead of cutting
    lbf = G.last_logits(sd, cfg, seqs, torch.bfloat16)
    from tests.gen_goldens_gemma2 import golden_tolerance

    assert np.abs(lbf - z["logits_bf16"]).max() <= golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    assert np.array_equal(z["scores_bf16"], z["logits_bf16"][:, z["label_ids"]])
    # the goldens really are Gemma-2's arithmetic: without either cap, or with Gemma v1's layer (its reading of the same norm
    # names: no out-norms, post_attention_layernorm in front of the MLP), the same weights score far away
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    for k in ("attn_logit_softcapping", "final_logit_softcapping"):
        assert np.abs(G.last_logits(sd, dict(cfg, **{k: None}), seqs) - l32).max() >= 10 * tol, k
    from tests import gemma_ref as G1

    v1 = G1.last_logits(sd, cfg, seqs)
    assert np.abs(v1 - l32).max() >= 10 * tol
