"""Host side of the Phi-3 ranker (--llm phi3), no GPU: the committed goldens against the fp32 restatement, config dispatch and
its refusals, the split of the fused qkv_proj / gate_up_proj Linears, presets, the sliding window, and train_ranker's refusal
to train a Phi-3 base."""
import json
import os

import numpy as np
import pytest
import torch

from llamarec_amd.synth import synth_phi3_state

PHI3_GOLDENS = ("hd96_mha", "hd96_gqa", "hd16")


def load_phi3_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"phi3_tiny_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_phi3_state(cfg, int(z["weight_seed"]), std=float(z["weight_std"]))
    T = z["input_ids"].shape[1]
    seqs = [z["input_ids"][b, T - n:] for b, n in enumerate(z["lens"])]
    return z, cfg, sd, seqs


@pytest.mark.parametrize("name", PHI3_GOLDENS)
def test_restatement_matches_the_reference_goldens(golden_dir, name):
    """tests/phi3_ref.py in fp32 sits on the reference's fp32 logits (padded and unpadded), its bf16 run within the archive's
    tolerance, and each misreading of the fused Linears is at least ten tolerances away."""
    from tests import phi3_ref as PR
    from tests.gen_goldens_phi3 import golden_tolerance

    z, cfg, sd, seqs = load_phi3_golden(golden_dir, name)
    assert cfg["model_type"] == "phi3" and "model.layers.0.self_attn.qkv_proj.weight" in sd
    assert list(z["lens"]) == [37, 5, 64, 1, 20, 130] and float(z["eval_loss"]) == -1.0
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    got = PR.last_logits(sd, cfg, seqs)
    scale = max(1.0, float(np.abs(z["logits_fp32"]).max()))
    assert np.abs(got - z["logits_fp32"]).max() < 1e-4 * scale
    assert np.abs(got - z["logits_fp32_unpadded"]).max() < 1e-4 * scale
    assert np.abs(PR.last_logits(sd, cfg, seqs, torch.bfloat16) - z["logits_bf16"]).max() < tol
    for mutant in ("swap_gate_up", "interleaved_qkv"):
        assert np.abs(PR.last_logits(sd, cfg, seqs, mutant=mutant) - z["logits_fp32"]).max() >= 10 * tol, mutant
    assert np.array_equal(z["scores_fp32"], z["logits_fp32"][:, z["label_ids"]])


def test_phi3_model_type_dispatch_needs_a_complete_config():
    from llamarec_amd.llm import LLAMA2_7B, LLAMA3_ROPE_SCALING, PHI3_MEDIUM, PHI3_MINI, PHI3_REQUIRED_KEYS, LlamaRanker, model_family

    assert model_family(PHI3_MINI) == "phi3" and model_family(PHI3_MEDIUM) == "phi3"
    assert model_family(dict(PHI3_MINI, sliding_window=None)) == "phi3"                 # null: no window
    assert model_family(dict(PHI3_MINI, partial_rotary_factor=1.0)) == "phi3"
    assert model_family(dict(PHI3_MINI, rope_scaling={"rope_type": "default"})) == "phi3"
    assert PHI3_REQUIRED_KEYS == ("hidden_act", "original_max_position_embeddings", "sliding_window")
    for key in PHI3_REQUIRED_KEYS:
        cfg = {k: v for k, v in PHI3_MINI.items() if k != key}
        with pytest.raises(NotImplementedError, match=rf"'phi3'.*{key}.*supported families"):
            model_family(cfg)
        with pytest.raises(NotImplementedError, match=key):
            LlamaRanker(cfg, device="cpu")
    with pytest.raises(NotImplementedError, match=r"'phi3'.*supported families"):        # a Llama config relabelled
        model_family(dict(LLAMA2_7B, model_type="phi3"))
    for bad, pattern in [(dict(hidden_act="gelu"), "hidden_act='gelu'"),
                         (dict(hidden_act=None), "hidden_act"),
                         (dict(rope_scaling={"type": "longrope", "short_factor": [1.0], "long_factor": [1.0]}), "longrope"),
                         (dict(rope_scaling={"type": "su", "short_factor": [1.0], "long_factor": [1.0]}), "'su'"),
                         (dict(rope_scaling=None, rope_parameters={"rope_type": "longrope", "rope_theta": 10000.0}), "longrope"),
                         (dict(rope_scaling=dict(LLAMA3_ROPE_SCALING)), "llama3"),
                         (dict(partial_rotary_factor=0.5), "partial_rotary_factor=0.5"),
                         (dict(sliding_window=0), "sliding_window=0")]:
        with pytest.raises(NotImplementedError, match=pattern) as e:
            model_family(dict(PHI3_MINI, **bad))
        assert "phi3" in str(e.value), bad


def test_phi3_presets():
    from llamarec_amd.llm import PHI3_MEDIUM, PHI3_MINI, LlamaRanker

    mini = LlamaRanker(PHI3_MINI, device="cpu")
    assert mini.family == "phi3" and mini.hd == 96 and mini.max_prompt_len == 2047 and mini.rope_scaling is None
    assert mini.rope_theta == 10000.0
    c = PHI3_MINI
    assert (c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], c["intermediate_size"], c["num_hidden_layers"],
            c["vocab_size"], c["rms_norm_eps"]) == (3072, 32, 32, 8192, 32, 32064, 1e-5)
    # every GEMM shape of Phi-3-mini is a multiple of the 256 x 256 tile
    assert all(n % 256 == 0 for n in (3 * 3072, 3072, 2 * 8192, 8192))
    medium = LlamaRanker(PHI3_MEDIUM, device="cpu")
    assert medium.family == "phi3" and medium.hd == 128
    c = PHI3_MEDIUM
    assert (c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], c["intermediate_size"],
            c["num_hidden_layers"]) == (5120, 40, 10, 17920, 40)
    a = mini.arch()
    assert (a.norm_style, a.mlp_act, a.embed_scale) == (0, 0, 1.0)


def test_phi3_check_lengths_refuses_above_the_window():
    from llamarec_amd.llm import PHI3_MINI, LlamaRanker

    r = LlamaRanker(dict(PHI3_MINI, sliding_window=100), device="cpu")
    with pytest.raises(NotImplementedError, match="Phi-3's sliding window of 100"):
        r._check_lengths(np.array([0, 50, 151], np.int32))
    r._check_lengths(np.array([0, 100, 150], np.int32))
    LlamaRanker(dict(PHI3_MINI, sliding_window=None), device="cpu")._check_lengths(np.array([0, 5000], np.int32))


def _tensors_of(monkeypatch, sd, cfg, **kw):
    from llamarec_amd.llm import LlamaRanker

    monkeypatch.setattr(LlamaRanker, "_create", lambda self: None)
    return LlamaRanker.from_state_dict(sd, cfg, device="cpu", **kw)._tensors


@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 2)])
def test_fused_linears_are_split_like_separate_ones(monkeypatch, nh, nkv):
    """A hand-built state dict: qkv_proj rows carry their own index, so the q | k | v cuts at nh hd, nkv hd, nkv hd and the
    gate | up halves are visible; the packed tensors must equal those of the same weights under Llama's separate names."""
    hd, d, f, L = 96, nh * 96, 64, 2
    cfg = dict(model_type="phi3", vocab_size=32, hidden_size=d, intermediate_size=f, num_hidden_layers=L, num_attention_heads=nh,
               num_key_value_heads=nkv, max_position_embeddings=64, original_max_position_embeddings=64, rms_norm_eps=1e-5,
               rope_theta=10000.0, rope_scaling=None, hidden_act="silu", sliding_window=None, tie_word_embeddings=False)
    rng = np.random.default_rng(0)
    phi, llama = {}, {}
    for name in ("model.embed_tokens.weight", "lm_head.weight"):
        phi[name] = llama[name] = rng.standard_normal((32, d)).astype(np.float32)
    phi["model.norm.weight"] = llama["model.norm.weight"] = np.ones(d, np.float32)
    for i in range(L):
        p = f"model.layers.{i}."
        qkv = rng.standard_normal(((nh + 2 * nkv) * hd, d)).astype(np.float32)
        qkv[:, 0] = np.arange(qkv.shape[0])                 # row r carries r (exact in bf16 up to 256; checked in fp32 below)
        gu = rng.standard_normal((2 * f, d)).astype(np.float32)
        gu[:, 0] = np.arange(2 * f)
        phi[p + "self_attn.qkv_proj.weight"], phi[p + "mlp.gate_up_proj.weight"] = qkv, gu
        llama[p + "self_attn.q_proj.weight"] = qkv[: nh * hd]
        llama[p + "self_attn.k_proj.weight"] = qkv[nh * hd: (nh + nkv) * hd]
        llama[p + "self_attn.v_proj.weight"] = qkv[(nh + nkv) * hd:]
        llama[p + "mlp.gate_proj.weight"], llama[p + "mlp.up_proj.weight"] = gu[:f], gu[f:]
        for n, shape in (("self_attn.o_proj.weight", (d, nh * hd)), ("mlp.down_proj.weight", (d, f))):
            phi[p + n] = llama[p + n] = rng.standard_normal(shape).astype(np.float32)
        for n in ("input_layernorm.weight", "post_attention_layernorm.weight"):
            phi[p + n] = llama[p + n] = np.ones(d, np.float32)
    got = _tensors_of(monkeypatch, phi, cfg)
    want = _tensors_of(monkeypatch, llama, dict(cfg, model_type="llama"))
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    w = got["0.wqkv"].float()
    assert w.shape == ((nh + 2 * nkv) * hd, d)
    # q head 0 after the rotary interleave: rows 0, 48, 1, 49, ...; v rows in order behind q and k
    assert w[:4, 0].tolist() == [0.0, 48.0, 1.0, 49.0] and w[(nh + nkv) * hd, 0] == float((nh + nkv) * hd)
    gu = got["0.wgu"].float()                        # 16 gate rows, then the 16 up rows of the same columns
    assert gu[:16, 0].tolist() == list(range(16)) and gu[16:32, 0].tolist() == list(range(f, f + 16))
    # a wrong row count is an error, not a silent cut
    bad = dict(phi)
    bad["model.layers.0.self_attn.qkv_proj.weight"] = phi["model.layers.0.self_attn.qkv_proj.weight"][:-hd]
    with pytest.raises(ValueError, match="qkv_proj"):
        _tensors_of(monkeypatch, bad, cfg)


def test_phi3_refuses_a_tied_head_and_every_adapter(monkeypatch):
    from llamarec_amd.synth import PHI3_TINY

    cfg = dict(PHI3_TINY, vocab_size=64)
    sd = synth_phi3_state(cfg, 3)
    tied = {k: v for k, v in sd.items() if k != "lm_head.weight"}
    with pytest.raises(NotImplementedError, match="tie_word_embeddings"):
        _tensors_of(monkeypatch, tied, dict(cfg, tie_word_embeddings=True))
    d = cfg["hidden_size"]
    for module, rows in (("qkv_proj", 3 * d), ("q_proj", d)):
        base = f"model.layers.0.self_attn.{module}"
        lora = dict(r=8, alpha=32, weights={base + ".lora_A.weight": np.zeros((8, d), np.float32),
                                            base + ".lora_B.weight": np.zeros((rows, 8), np.float32)})
        with pytest.raises(NotImplementedError, match="map to no Linear"):
            _tensors_of(monkeypatch, sd, cfg, lora=lora)


def test_synth_phi3_state_has_the_fused_names():
    from llamarec_amd.synth import PHI3_TINY, phi3_param_shapes

    names = dict(phi3_param_shapes(PHI3_TINY))
    assert names["model.layers.1.self_attn.qkv_proj.weight"] == (3 * 768, 768)
    assert names["model.layers.1.mlp.gate_up_proj.weight"] == (2 * 1024, 768) and "lm_head.weight" in names
    assert not any("q_proj" in n or "gate_proj" in n for n in names)
    assert PHI3_TINY["hidden_size"] // PHI3_TINY["num_attention_heads"] == 96


def test_train_ranker_refuses_to_train_a_phi3_base(tmp_path):
    import train_ranker

    assert "Phi-3" in train_ranker.TRAIN_LLAMA_ONLY
    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "phi3", "--llm_retrieved_path", str(tmp_path)])
