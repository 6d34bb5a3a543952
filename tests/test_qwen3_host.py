"""Host side of the Qwen3 ranker (--llm qwen3), no GPU: the committed goldens against the fp32 restatement, config dispatch and
its refusals, presets, the q / k norm weights in a head's packed column order, synth_qwen3_state's names, the float64
restatements of the sweep and its backward (tests/qwen3_ref.py) against torch autograd and against their own mutants, the
goldens' regeneration, and the declarations of the three new C calls."""
import json
import os
import re

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_round, hash_uniform, synth_qwen3_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("LLAMAREC_REFERENCE") or "/root/reference"   # tests/gen_goldens_rank_train.py's REF
QWEN3_GOLDENS = ("hd128_gqa", "hd16")
# the shapes of the sweep tests, here and in tests/test_gpu_qwen3.py: (nq, nk, hd)
SWEEP_SHAPES = [(4, 2, 128), (2, 1, 64), (4, 2, 16), (1, 1, 256)]
T_ROPE = 512


def load_qwen3_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"qwen3_tiny_{name}.npz"))
    cfg = json.loads(str(z["config"]))
    sd = synth_qwen3_state(cfg, int(z["weight_seed"]), std=float(z["weight_std"]), qk_norm_spread=float(z["qk_norm_spread"]))
    T = z["input_ids"].shape[1]
    seqs = [z["input_ids"][b, T - n:] for b, n in enumerate(z["lens"])]
    return z, cfg, sd, seqs


def sweep_case(M, nq, nk, hd, seed=0):
    """(x, wq, wk, pos, cos, sin): bf16-valued packed heads of mixed scale (rows 0.05 .. 3 wide), packed norm weights 1 + U(0.75)
    (so some are near zero or negative), ragged positions (test_gpu_qwen2._positions) and HF's bf16 rope table."""
    from tests.stage2_ref import rope_table_hf

    scale = (0.05 * 60.0 ** hash_uniform(seed + 7, (M, 1), 1.0).clip(0, 1)).astype(np.float32)
    x = bf16_round(hash_uniform(seed + M * 131 + hd, (M, (nq + nk) * hd), 1.0) * scale)
    wq = bf16_round(np.float32(1.0) + hash_uniform(seed + hd + 1, (hd,), 0.75))
    wk = bf16_round(np.float32(1.0) + hash_uniform(seed + hd + 2, (hd,), 0.75))
    pos = ((np.arange(M) * 2654435761) % T_ROPE).astype(np.int32)
    pos[0] = T_ROPE - 1
    cos, sin, _, _ = rope_table_hf(T_ROPE, hd, 1e6)
    return x, wq, wk, pos, cos, sin


@pytest.mark.parametrize("name", QWEN3_GOLDENS)
def test_restatement_matches_the_reference_goldens(golden_dir, name):
    """tests/qwen3_ref.py in fp32 sits on HF's fp32 logits (padded and unpadded), its bf16 run within the archive's tolerance,
    and a model with both norm weights of ones is more than ten tolerances away."""
    from tests import qwen3_ref as QR
    from tests.gen_goldens_qwen3 import golden_tolerance

    z, cfg, sd, seqs = load_qwen3_golden(golden_dir, name)
    assert cfg["model_type"] == "qwen3" and sd["model.layers.0.self_attn.q_norm.weight"].shape == (cfg["head_dim"],)
    assert "lm_head.weight" not in sd and cfg["tie_word_embeddings"]
    assert list(z["lens"]) == [37, 5, 64, 1, 20, 130] and float(z["eval_loss"]) == -1.0
    assert sorted(z.files) == sorted(["config", "weight_seed", "weight_std", "qk_norm_spread", "input_ids", "attention_mask", "lens",
                                      "logits_fp32", "logits_fp32_unpadded", "logits_bf16", "eval_loss", "label_ids",
                                      "scores_fp32", "scores_bf16"])
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    got = QR.last_logits(sd, cfg, seqs)
    scale = max(1.0, float(np.abs(z["logits_fp32"]).max()))
    assert np.abs(got - z["logits_fp32"]).max() < 1e-4 * scale
    assert np.abs(got - z["logits_fp32_unpadded"]).max() < 1e-4 * scale
    assert np.abs(QR.last_logits(sd, cfg, seqs, torch.bfloat16) - z["logits_bf16"]).max() < tol
    assert np.abs(QR.last_logits(sd, cfg, seqs, mutant="ones_norm") - z["logits_fp32"]).max() > 10 * tol
    assert np.array_equal(z["scores_fp32"], z["logits_fp32"][:, z["label_ids"]])
    w = np.concatenate([sd[f"model.layers.{i}.self_attn.{n}_norm.weight"] for i in range(2) for n in "qk"])
    assert abs(w.mean() - 1.0) < 0.25 and w.std() > 0.3                     # mean 1 (64 to 512 draws), clearly not ones


def test_qwen3_model_type_dispatch_needs_a_complete_config():
    from llamarec_amd.llm import (LLAMA2_7B, LLAMA3_ROPE_SCALING, QWEN3_0_6B, QWEN3_1_7B, QWEN3_4B, QWEN3_8B, QWEN3_FAMILY,
                                  QWEN3_REQUIRED_KEYS, SUPPORTED_MODEL_TYPES, LlamaRanker, model_family)

    assert QWEN3_FAMILY == ("qwen3",) and "qwen3" in SUPPORTED_MODEL_TYPES and SUPPORTED_MODEL_TYPES[-1] == "gemma2"
    assert SUPPORTED_MODEL_TYPES.index("qwen3") < SUPPORTED_MODEL_TYPES.index("gemma")
    for preset in (QWEN3_0_6B, QWEN3_1_7B, QWEN3_4B, QWEN3_8B):
        assert model_family(preset) == "qwen3"
    assert model_family(dict(QWEN3_0_6B, layer_types=["full_attention"] * 28)) == "qwen3"
    assert model_family(dict(QWEN3_0_6B, rope_scaling={"rope_type": "default"})) == "qwen3"
    assert model_family({k: v for k, v in QWEN3_0_6B.items() if k not in ("use_sliding_window", "sliding_window")}) == "qwen3"
    assert "head_dim" in QWEN3_REQUIRED_KEYS and "hidden_act" in QWEN3_REQUIRED_KEYS and "attention_bias" in QWEN3_REQUIRED_KEYS
    for key in QWEN3_REQUIRED_KEYS:
        cfg = {k: v for k, v in QWEN3_0_6B.items() if k != key}
        with pytest.raises(NotImplementedError, match=rf"'qwen3'.*{key}.*supported families"):
            model_family(cfg)
        with pytest.raises(NotImplementedError, match=key):
            LlamaRanker(cfg, device="cpu")
    with pytest.raises(NotImplementedError, match=r"'qwen3'.*head_dim, hidden_act, attention_bias.*supported families.*gemma2$"):
        model_family(dict(LLAMA2_7B, model_type="qwen3"))                                    # a Llama config relabelled
    for bad, pattern in [(dict(hidden_act="gelu"), "hidden_act='gelu'"),
                         (dict(attention_bias=True), "attention_bias=True"),
                         (dict(head_dim=96), "head_dim=96"),
                         (dict(head_dim=512), "head_dim=512"),
                         (dict(use_sliding_window=True, sliding_window=4096), "use_sliding_window=True"),
                         (dict(layer_types=["full_attention", "sliding_attention"]), "sliding_attention"),
                         (dict(rope_scaling={"type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}), "yarn"),
                         (dict(rope_scaling={"rope_type": "dynamic", "factor": 2.0}), "dynamic"),
                         (dict(rope_scaling=dict(LLAMA3_ROPE_SCALING)), "llama3")]:
        with pytest.raises(NotImplementedError, match=pattern) as e:
            model_family(dict(QWEN3_0_6B, **bad))
        assert "qwen3" in str(e.value) and "supported families" in str(e.value), bad
    with pytest.raises(NotImplementedError, match=r"'qwen3_moe'.*mixture-of-experts"):
        model_family(dict(QWEN3_0_6B, model_type="qwen3_moe", num_experts=128))
    with pytest.raises(NotImplementedError, match=r"'gpt2' is not supported.*qwen3.*gemma2$"):
        model_family(dict(LLAMA2_7B, model_type="gpt2"))


def test_qwen3_presets_and_flags():
    from llamarec_amd import config as cfg
    from llamarec_amd.llm import QWEN3_0_6B, QWEN3_1_7B, QWEN3_4B, QWEN3_8B, LlamaRanker

    want = {"0.6B": (QWEN3_0_6B, 1024, 3072, 28, 16, 8, True), "1.7B": (QWEN3_1_7B, 2048, 6144, 28, 16, 8, True),
            "4B": (QWEN3_4B, 2560, 9728, 36, 32, 8, True), "8B": (QWEN3_8B, 4096, 12288, 36, 32, 8, False)}
    for name, (c, d, f, nl, nh, nkv, tied) in want.items():
        assert (c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["num_attention_heads"],
                c["num_key_value_heads"], c["tie_word_embeddings"]) == (d, f, nl, nh, nkv, tied), name
        assert c["vocab_size"] == 151936 and c["head_dim"] == 128 and c["rope_theta"] == 1e6 and c["rms_norm_eps"] == 1e-6
        r = LlamaRanker(c, device="cpu")
        assert r.family == "qwen3" and r.hd == 128 and r.rope_scaling is None and r.max_prompt_len is None
        assert r.default_gemm_variant == 0
        a = r.arch()
        assert (a.norm_style, a.mlp_act, a.embed_scale) == (0, 0, 1.0)
        # every product of a layer sits on the 256-column GEMM tile
        assert all(n % 256 == 0 for n in ((nh + 2 * nkv) * 128, d, 2 * f)) and d % 64 == 0 and f % 64 == 0
    assert QWEN3_0_6B["num_attention_heads"] * 128 != QWEN3_0_6B["hidden_size"]               # head_dim from the config
    with pytest.raises(NotImplementedError, match="q/k norms"):
        LlamaRanker(QWEN3_0_6B, device="cpu").set_fold_norms(True)
    args = cfg.parse(["--dataset_code", "beauty", "--llm", "qwen3"], model_code="llm")
    assert args.llm == "qwen3" and args.llm_base_model == "Qwen/Qwen3-0.6B" and args.llm_base_tokenizer == "Qwen/Qwen3-0.6B"
    llama2 = cfg.parse(["--dataset_code", "beauty", "--llm", "llama2"], model_code="llm")
    assert (args.train_batch_size, args.lora_micro_batch_size, args.test_batch_size) == (
        llama2.train_batch_size, llama2.lora_micro_batch_size, llama2.test_batch_size)
    assert cfg.LLM_CHOICES[-1] == "qwen3" and cfg.LLM_CHOICES[:7] == ["llama2", "llama3", "phi3", "gemma", "mistral", "gemma2", "qwen2"]
    with pytest.raises(SystemExit):
        cfg.parse(["--dataset_code", "beauty", "--llm", "gpt2"], model_code="llm")


def _tensors_of(monkeypatch, sd, cfg, **kw):
    from llamarec_amd.llm import LlamaRanker

    monkeypatch.setattr(LlamaRanker, "_create", lambda self: None)
    return LlamaRanker.from_state_dict(sd, cfg, device="cpu", **kw)._tensors


def _tiny_cfg():
    from llamarec_amd.synth import QWEN3_TINY

    return dict(QWEN3_TINY, vocab_size=64, intermediate_size=64)


def test_norm_weights_are_stored_in_a_heads_packed_order(monkeypatch):
    """q_norm.weight[i] = i at head_dim 128: the stored weight starts 0, 64, 1, 65 -- _interleave_rope_rows applied to a
    one-head matrix's rows -- and it moves with the rows of wq: row j of every head of wqkv meets entry j of the norm weight."""
    from llamarec_amd.llm import LlamaRanker

    cfg = _tiny_cfg()
    nh, nkv, hd = 4, 2, 128
    sd = synth_qwen3_state(cfg, 3)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}.self_attn."
        sd[p + "q_norm.weight"] = np.arange(hd, dtype=np.float32)
        sd[p + "k_norm.weight"] = 0.5 + np.arange(hd, dtype=np.float32)                      # exact in bf16
        sd[p + "q_proj.weight"] = sd[p + "q_proj.weight"].copy()
        sd[p + "q_proj.weight"][:, 0] = np.tile(np.arange(hd), nh)                             # row r of a head carries r
    T = _tensors_of(monkeypatch, sd, cfg)
    qn, kn = T["0.q_norm"], T["1.k_norm"]
    assert qn.dtype == torch.bfloat16 and qn.shape == (hd,) and qn.is_contiguous() and kn.shape == (hd,)
    assert qn.float()[:4].tolist() == [0.0, 64.0, 1.0, 65.0] and kn.float()[:4].tolist() == [0.5, 64.5, 1.5, 65.5]
    one_head = torch.arange(hd, dtype=torch.float32).reshape(hd, 1)
    want = LlamaRanker(cfg, device="cpu")._interleave_rope_rows(one_head).reshape(-1)
    assert torch.equal(qn.float(), want)
    for h in range(nh):
        assert torch.equal(T["0.wqkv"].float()[h * hd:(h + 1) * hd, 0], qn.float())           # rows and weight: one permutation
    assert "lm_head.weight" not in sd and T["lm_head"] is T["embed"]
    assert T["0.wqkv"].shape == ((nh + 2 * nkv) * hd, 256) and T["0.wo"].shape == (256, nh * hd)
    assert sorted(k for k in T if k.startswith("1.")) == sorted(
        f"1.{n}" for n in ("wqkv", "q_norm", "k_norm", "wo", "wgu", "wdown", "input_norm", "post_norm"))


def test_a_missing_norm_weight_is_an_error_that_names_it(monkeypatch):
    cfg = _tiny_cfg()
    sd = synth_qwen3_state(cfg, 3)
    for n in "qk":
        key = f"model.layers.1.self_attn.{n}_norm.weight"
        with pytest.raises(KeyError, match=re.escape(key)):
            _tensors_of(monkeypatch, {k: v for k, v in sd.items() if k != key}, cfg)
    # the same tensors relabelled llama load without the norms: only the family decides
    llama = _tensors_of(monkeypatch, dict(sd, **{"lm_head.weight": sd["model.embed_tokens.weight"]}),
                        {k: v for k, v in cfg.items() if k != "model_type"})
    assert "0.q_norm" not in llama


def test_an_adapter_merges_into_wqkv_and_leaves_the_norm_weights_alone(monkeypatch):
    cfg = _tiny_cfg()
    d, nh, nkv, hd = 256, 4, 2, 128
    sd = synth_qwen3_state(cfg, 4)
    rng = np.random.default_rng(0)
    w = {}
    for i in range(cfg["num_hidden_layers"]):
        for m, rows in (("q_proj", nh * hd), ("k_proj", nkv * hd)):
            base = f"model.layers.{i}.self_attn.{m}"
            w[base + ".lora_A.weight"] = rng.standard_normal((8, d)).astype(np.float32) * 0.1
            w[base + ".lora_B.weight"] = rng.standard_normal((rows, 8)).astype(np.float32) * 0.1
    plain = _tensors_of(monkeypatch, sd, cfg)
    tuned = _tensors_of(monkeypatch, sd, cfg, lora=dict(r=8, alpha=32, weights=w))
    for i in range(cfg["num_hidden_layers"]):
        assert torch.equal(tuned[f"{i}.q_norm"], plain[f"{i}.q_norm"]) and torch.equal(tuned[f"{i}.k_norm"], plain[f"{i}.k_norm"])
        dq = (tuned[f"{i}.wqkv"].float() - plain[f"{i}.wqkv"].float()).abs().amax(1)
        assert (dq[:(nh + nkv) * hd] > 0).all() and (dq[(nh + nkv) * hd:] == 0).all()          # q and k rows, not v


def test_synth_qwen3_state_has_the_norm_names_and_shapes():
    from llamarec_amd.synth import QWEN3_TINY, qwen3_param_shapes

    c = QWEN3_TINY
    assert (c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"], c["tie_word_embeddings"]) == (
        256, 4, 2, 128, True)
    names = dict(qwen3_param_shapes(c))
    assert names["model.layers.1.self_attn.q_proj.weight"] == (512, 256) and names["model.layers.1.self_attn.o_proj.weight"] == (256, 512)
    assert names["model.layers.1.self_attn.k_proj.weight"] == (256, 256)
    assert names["model.layers.1.self_attn.q_norm.weight"] == (128,) and names["model.layers.1.self_attn.k_norm.weight"] == (128,)
    assert not any(n.endswith("bias") for n in names) and "lm_head.weight" not in names
    assert "lm_head.weight" in dict(qwen3_param_shapes(dict(c, tie_word_embeddings=False)))
    sd = synth_qwen3_state(c, 7)
    assert sorted(sd) == sorted(names) and all(sd[n].shape == s for n, s in names.items())
    qn = np.concatenate([sd[f"model.layers.{i}.self_attn.{n}_norm.weight"] for i in range(2) for n in "qk"])
    assert abs(qn.mean() - 1.0) < 0.15 and qn.std() > 0.5                                    # mean 1, far from ones
    assert abs(sd["model.layers.0.input_layernorm.weight"].std()) < 0.15


@pytest.mark.parametrize("nq,nk,hd", SWEEP_SHAPES)
def test_sweep_restatement_and_its_mutants(nq, nk, hd):
    """The float64 restatement with its two roundings stays within its own bound of the unrounded float64 forward (so the
    bound is no tighter than the roundings it names), the k-only and q-only column groups equal the joint call's columns, and
    each mutant differs from the restatement in more than a tenth of the elements at M = 259 -- by more than the bound."""
    from tests import qwen3_ref as QR

    M = 259
    x, wq, wk, pos, cos, sin = sweep_case(M, nq, nk, hd)
    ref, bound = QR.sweep_ref64(x, pos, cos, sin, nq, nk, hd, wq, wk, 1e-6)
    plain = QR.forward_packed64(torch.from_numpy(x.astype(np.float64)), pos, cos, sin, nq, nk, hd, wq, wk, 1e-6).numpy()
    assert ref.shape == (M, (nq + nk) * hd) and np.isfinite(ref).all() and (bound > 0).all()
    assert (np.abs(ref - plain) <= bound).all()
    assert np.abs(bound).max() < 0.05 * np.abs(ref).max()
    k_only, _ = QR.sweep_ref64(x[:, nq * hd:], pos, cos, sin, 0, nk, hd, None, wk, 1e-6)
    q_only, _ = QR.sweep_ref64(x[:, :nq * hd], pos, cos, sin, nq, 0, hd, wq, None, 1e-6)
    assert np.array_equal(k_only, ref[:, nq * hd:]) and np.array_equal(q_only, ref[:, :nq * hd])
    for m in QR.SWEEP_MUTANTS:
        mut, _ = QR.sweep_ref64(x, pos, cos, sin, nq, nk, hd, wq, wk, 1e-6, mutant=m)
        cols = slice(0, nq * hd) if m == "k_norm_for_q" else slice(None)
        frac = float((np.abs(mut - ref) > bound)[:, cols].mean())
        assert frac > 0.1, (m, frac)


@pytest.mark.parametrize("nq,nk,hd", SWEEP_SHAPES)
def test_backward_restatement_matches_autograd(nq, nk, hd):
    from tests import qwen3_ref as QR

    M = 37
    x, wq, wk, pos, cos, sin = sweep_case(M, nq, nk, hd, seed=5)
    dy = bf16_round(hash_uniform(99 + hd, x.shape, 1.0))
    dx, bound = QR.norm_bwd_ref64(dy, x, nq, nk, hd, wq, wk, 1e-6)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    (QR.normed_packed64(xt, nq, nk, hd, wq, wk, 1e-6) * torch.from_numpy(dy.astype(np.float64))).sum().backward()
    assert np.abs(dx - xt.grad.numpy()).max() < 1e-10 * max(1.0, np.abs(dx).max())
    assert (bound > 0).all() and (bound < 2.0 ** -6 * np.abs(dx) + 2.0 ** -6 * np.abs(dx).max()).all()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "trainer")), reason="the reference tree is not on this machine")
def test_goldens_regenerate_byte_for_byte(golden_dir, tmp_path):
    """Both generators, each in a process of its own with one OpenMP / MKL thread (the thread count a process starts with decides
    the order of torch's CPU sums, and cannot be changed once torch is loaded): the committed archives, byte for byte."""
    import subprocess
    import sys

    pytest.importorskip("transformers")
    env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1", PYTHONDONTWRITEBYTECODE="1")
    for mod in ("tests.gen_goldens_qwen3", "tests.gen_goldens_qwen3_train"):
        subprocess.run([sys.executable, "-m", mod, REFERENCE, str(tmp_path)], cwd=REPO, env=env, check=True, capture_output=True)
    made = sorted(os.listdir(tmp_path))
    assert made == sorted(f for f in os.listdir(golden_dir) if f.startswith("qwen3_"))
    for f in made:
        assert open(os.path.join(tmp_path, f), "rb").read() == open(os.path.join(golden_dir, f), "rb").read(), f


def test_train_goldens_hold_the_k_norm_margin(golden_dir):
    from tests.gen_goldens_qwen3_train import rel

    z = np.load(os.path.join(golden_dir, "qwen3_lora_train_hd128_gqa_qkvo.npz"))
    assert list(z["modules"]) == ["q_proj", "v_proj", "k_proj", "o_proj"]
    names = [n for n in z["param_names"] if str(n).endswith("k_proj.lora_B")]
    assert len(names) == 2
    for n in names:
        assert np.linalg.norm(z["step0/grad/" + n]) > 0 and rel(z["no_k_norm/grad/" + n], z["step0/grad/" + n].astype(np.float64)) > 0.1
    zq = np.load(os.path.join(golden_dir, "qwen3_lora_train_hd128_gqa_qv.npz"))
    assert list(zq["modules"]) == ["q_proj", "v_proj"] and not [f for f in zq.files if f.startswith("no_k_norm")]


def test_train_ranker_trains_qwen3_and_still_refuses_the_other_four(tmp_path):
    import train_ranker

    src = open(os.path.join(REPO, "train_ranker.py")).read()
    assert 'model.family not in ("llama", "qwen3")' in src and '("gemma", "gemma2", "phi3", "qwen2")' in src
    assert "Qwen3" not in train_ranker.TRAIN_LLAMA_ONLY
    for llm in ("gemma", "gemma2", "phi3", "qwen2"):
        with pytest.raises(SystemExit, match="eval_only"):
            train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", llm, "--llm_retrieved_path", str(tmp_path)])
    with pytest.raises(FileNotFoundError):      # qwen3 passes the family gate and goes on to read the retrieved candidates
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "qwen3", "--llm_retrieved_path", str(tmp_path)])


def test_new_symbols_are_declared_and_prototyped():
    import ctypes as C

    from llamarec_amd import _lib

    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    for name in ("lr_llama_set_qk_norm", "lr_qk_norm_rope_bf16", "lr_qk_norm_bwd_bf16"):
        assert name in _lib.PROTOTYPES and re.search(rf"\bint {name}\(", header), name
    assert _lib.PROTOTYPES["lr_llama_set_qk_norm"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert len(_lib.PROTOTYPES["lr_qk_norm_rope_bf16"][1]) == 13 and len(_lib.PROTOTYPES["lr_qk_norm_bwd_bf16"][1]) == 13
    kernels = open(os.path.join(REPO, "llamarec_amd", "csrc", "llama_kernels.h")).read()
    train = open(os.path.join(REPO, "llamarec_amd", "csrc", "llama_train.h")).read()
    assert "int lr_launch_qk_norm_rope(" in kernels and "int lr_launch_qk_norm_bwd(" in train
    if os.path.exists(_lib.LIB_PATH):
        l = _lib.lib()
        assert all(hasattr(l, n) for n in ("lr_llama_set_qk_norm", "lr_qk_norm_rope_bf16", "lr_qk_norm_bwd_bf16"))
        # argument checks run before anything touches a GPU
        assert l.lr_qk_norm_rope_bf16(None, 4, 768, 0, 4, 2, 96, None, None, 1e-6, None, None, None) == -2
        assert b"head_dim 96" in l.lr_last_error()
        assert l.lr_qk_norm_rope_bf16(None, 4, 768, 0, 4, 2, 128, None, None, 1e-6, None, None, None) == -1
        assert l.lr_qk_norm_bwd_bf16(None, 4, 768, 0, None, 768, 4, 2, 96, None, None, 1e-6, None) == -2
        assert l.lr_llama_set_qk_norm(None, None, None) == -1
