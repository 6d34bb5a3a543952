"""GPU: the Qwen3 ranker (--llm qwen3) through the C ABI: the q/k norm + rotation sweep (lr_qk_norm_rope_bf16) and its backward
(lr_qk_norm_bwd_bf16) against the float64 restatements and bounds of tests/qwen3_ref.py, the scoring path on the committed
Qwen3 goldens (tests/gen_goldens_qwen3.py) in every mode, lr_llama_set_qk_norm and the refusals that go with it, and one
full-width case at Qwen3-0.6B's layer shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_round, hash_uniform
from tests import qwen3_ref as QR
from tests.test_gpu_attn_prefix import _prefixed_prompts
from tests.test_gpu_qwen2 import POISON, T_ROPE, _positions, _table
from tests.test_gpu_stage2_bounds import _dev_bf16, _host
from tests.test_qwen3_host import QWEN3_GOLDENS, SWEEP_SHAPES, load_qwen3_golden, sweep_case

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
EPS = 1e-6
MS = [1, 5, 259]


def _sweep(x, M, nq, nk, hd, wq_d, wk_d, pos_d, cs, group="joint", want_rc=0):
    """One lr_qk_norm_rope_bf16 call on a [M + 1][(nq + 2 nk) hd] buffer: q | k columns from x, v columns and the guard row at
    the poison bits. group: joint, q (the first nq heads only) or k (col0 = nq hd, the K | V call of a pruned layer). Returns
    the q | k columns as float32 after checking that every column outside the group and the guard row kept their bits."""
    from llamarec_amd._lib import lib, stream_ptr

    qk, ld = (nq + nk) * hd, (nq + 2 * nk) * hd
    buf = torch.full((M + 1, ld), POISON, dtype=torch.int16, device="cuda")
    buf[:M, :qk] = _dev_bf16(x)
    before = buf.cpu().numpy().view(np.uint16).copy()
    col0, a, b = {"joint": (0, nq, nk), "q": (0, nq, 0), "k": (nq * hd, 0, nk)}[group]
    rc = lib().lr_qk_norm_rope_bf16(buf.data_ptr(), M, ld, col0, a, b, hd, wq_d.data_ptr() if a else None,
                                    wk_d.data_ptr() if b else None, EPS, pos_d.data_ptr(), cs.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, (group, M, nq, nk, hd, rc, lib().lr_last_error())
    bits = buf.cpu().numpy().view(np.uint16)
    lo, hi = col0, col0 + (a + b) * hd
    keep = np.ones(ld, bool)
    if want_rc == 0:
        keep[lo:hi] = False
    assert np.array_equal(bits[:, keep], before[:, keep]), ("a column outside the group or the guard row was written", group)
    assert (bits[M] == POISON).all() and (bits[:M, qk:] == POISON).all()
    return _host(buf[:M, :qk])


@pytest.mark.parametrize("nq,nk,hd", SWEEP_SHAPES)
def test_sweep_within_bound_of_the_float64_restatement(nq, nk, hd):
    cs, cos, sin = _table(hd)
    bad = []
    for M in MS:
        x, wq, wk, _, _, _ = sweep_case(M, nq, nk, hd)
        pos = _positions(M)
        pos_d, wq_d, wk_d = torch.from_numpy(pos).cuda(), _dev_bf16(wq), _dev_bf16(wk)
        ref, bound = QR.sweep_ref64(x, pos, cos, sin, nq, nk, hd, wq, wk, EPS)
        got = _sweep(x, M, nq, nk, hd, wq_d, wk_d, pos_d, cs)
        assert np.isfinite(got).all() and np.array_equal(got, bf16_round(got))
        r = float((np.abs(got - ref) / bound).max())
        print(f"sweep nq={nq} nk={nk} hd={hd} M={M}: err/bound {r:.3f}")
        if r > 1.0:
            bad.append((M, r))
        # the pruned layer's calls: the same bits as the joint call's columns, the other group untouched
        q_only = _sweep(x, M, nq, nk, hd, wq_d, wk_d, pos_d, cs, "q")
        k_only = _sweep(x, M, nq, nk, hd, wq_d, wk_d, pos_d, cs, "k")
        assert np.array_equal(q_only[:, :nq * hd], got[:, :nq * hd]) and np.array_equal(q_only[:, nq * hd:], x[:, nq * hd:])
        assert np.array_equal(k_only[:, nq * hd:], got[:, nq * hd:]) and np.array_equal(k_only[:, :nq * hd], x[:, :nq * hd])
        if M == 259:
            for m in QR.SWEEP_MUTANTS:
                mut, mb = QR.sweep_ref64(x, pos, cos, sin, nq, nk, hd, wq, wk, EPS, mutant=m)
                cols = slice(0, nq * hd) if m == "k_norm_for_q" else slice(None)
                frac = float((np.abs(got - mut) > mb)[:, cols].mean())
                print(f"  mutant {m}: {frac:.2f} of the rotated elements differ")
                assert frac > 0.1, (m, frac)
    assert not bad, bad


def test_sweep_refuses_head_dim_96_and_writes_nothing():
    from llamarec_amd._lib import lib

    nq, nk, hd, M = 4, 2, 96, 5
    cs, _, _ = _table(hd)
    x = bf16_round(hash_uniform(3, (M, (nq + nk) * hd), 1.0))
    w = _dev_bf16(np.ones(hd, np.float32))
    out = _sweep(x, M, nq, nk, hd, w, w, torch.from_numpy(_positions(M)).cuda(), cs, want_rc=LR_EUNSUPPORTED)
    assert np.array_equal(out, x) and b"head_dim 96" in lib().lr_last_error()


def _norm_bwd(dy, x, M, nq, nk, hd, wq_d, wk_d):
    from llamarec_amd._lib import lib, stream_ptr

    qk, ld = (nq + nk) * hd, (nq + 2 * nk) * hd
    buf = torch.full((M + 1, ld), POISON, dtype=torch.int16, device="cuda")
    buf[:M, :qk] = _dev_bf16(dy)
    x_d = _dev_bf16(x)
    rc = lib().lr_qk_norm_bwd_bf16(buf.data_ptr(), M, ld, 0, x_d.data_ptr(), qk, nq, nk, hd, wq_d.data_ptr(), wk_d.data_ptr(), EPS,
                                   stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().lr_last_error()
    bits = buf.cpu().numpy().view(np.uint16)
    assert (bits[M] == POISON).all() and (bits[:M, qk:] == POISON).all()
    return _host(buf[:M, :qk]), bits


@pytest.mark.parametrize("nq,nk,hd", SWEEP_SHAPES)
def test_norm_backward_within_bound_and_deterministic(nq, nk, hd):
    """lr_qk_norm_bwd_bf16 within its bound of the float64 restatement, which is torch autograd's gradient of the float64
    forward without roundings; two runs write the same bits."""
    for M in MS:
        x, wq, wk, _, _, _ = sweep_case(M, nq, nk, hd, seed=5)
        dy = bf16_round(hash_uniform(99 + hd + M, x.shape, 1.0))
        wq_d, wk_d = _dev_bf16(wq), _dev_bf16(wk)
        ref, bound = QR.norm_bwd_ref64(dy, x, nq, nk, hd, wq, wk, EPS)
        xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        (QR.normed_packed64(xt, nq, nk, hd, wq, wk, EPS) * torch.from_numpy(dy.astype(np.float64))).sum().backward()
        auto = xt.grad.numpy()
        assert np.abs(ref - auto).max() < 1e-10 * max(1.0, np.abs(ref).max())
        got, bits = _norm_bwd(dy, x, M, nq, nk, hd, wq_d, wk_d)
        r = float((np.abs(got - ref) / bound).max())
        print(f"norm backward nq={nq} nk={nk} hd={hd} M={M}: err/bound {r:.3f}, vs autograd {float((np.abs(got - auto) / bound).max()):.3f}")
        assert np.isfinite(got).all() and r <= 1.0, (M, r)
        assert (np.abs(got - auto) <= bound + 1e-9 * np.abs(auto).max()).all()
        _, again = _norm_bwd(dy, x, M, nq, nk, hd, wq_d, wk_d)
        assert np.array_equal(bits, again)


# ---- the scoring path on the goldens -----------------------------------------------------------------------------------------
_MODELS = {}
LABELS = list(range(40, 60))
MODEL_TAILS = [1, 7, 40, 90, 130]


def _golden_model(golden_dir, name):
    if name not in _MODELS:
        from llamarec_amd.llm import LlamaRanker
        from tests.gen_goldens_qwen3 import golden_tolerance

        z, cfg, sd, seqs = load_qwen3_golden(golden_dir, name)
        _MODELS[name] = (z, cfg, sd, seqs, golden_tolerance(z["logits_fp32"], z["logits_bf16"]), LlamaRanker.from_state_dict(sd, cfg))
    out = _MODELS[name]
    out[5].set_variants(0, 0).set_last_layer_pruning(True)
    return out


@pytest.mark.parametrize("name", QWEN3_GOLDENS)
@pytest.mark.parametrize("variants", ["default", (1, 1), (4, 2), (0, 0)])
def test_qwen3_prefill_vs_reference_goldens(golden_dir, name, variants):
    """Last-token logits within the archive's own tolerance of HF's fp32 and bf16 logits: the family default, the generic
    kernels, the 256-tile GEMM with the head_dim-128 MFMA attention forced (hd128_gqa; on hd16 the forced pair fails by name and
    the archive is scored with the generic attention behind auto GEMMs instead), and auto."""
    from llamarec_amd._lib import LlamaRecError

    z, cfg, sd, seqs, tol, model = _golden_model(golden_dir, name)
    assert model.family == "qwen3" and model.hd == cfg["head_dim"] and "0.q_norm" in model._tensors
    if variants == "default":
        variants = None
    elif variants == (4, 2) and name == "hd16":
        with pytest.raises(LlamaRecError):
            model.set_variants(4, 2).last_logits(seqs)
        torch.cuda.synchronize()
        variants = (0, 1)
    if variants is not None:
        model.set_variants(*variants)
    got = model.last_logits(seqs).cpu().numpy()
    assert got.shape == z["logits_bf16"].shape and np.array_equal(got, bf16_round(got))
    print(f"{name} {variants}: vs bf16 {np.abs(got - z['logits_bf16']).max():.4f}, vs fp32 {np.abs(got - z['logits_fp32']).max():.4f}, "
          f"tolerance {tol:.4f}")
    assert np.abs(got - z["logits_fp32"]).max() < tol
    assert np.abs(got - z["logits_bf16"]).max() < tol
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])


@pytest.mark.parametrize("name", QWEN3_GOLDENS)
def test_a_model_with_norm_weights_of_ones_is_far_from_the_goldens(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs, tol, _ = _golden_model(golden_dir, name)
    ones = {k: (np.ones_like(v) if k.endswith(("q_norm.weight", "k_norm.weight")) else v) for k, v in sd.items()}
    got = LlamaRanker.from_state_dict(ones, cfg).last_logits(seqs).cpu().numpy()
    assert np.abs(got - z["logits_fp32"]).max() > 10 * tol


@pytest.mark.parametrize("name", QWEN3_GOLDENS)
def test_qwen3_modes_agree(golden_dir, name):
    """Scores with the shared 36-token prefix are bit-identical to the unshared call (pruned last layer on and off: the K | V
    and Q products of the pruned layer are swept separately, the Q rows at last_pos); pruning on and off, and latency mode (GEMM
    variant 5: the split-K reduce stores plainly and the sweep follows) against the default, agree within the golden
    tolerance, which also holds each against the reference's logits."""
    z, cfg, sd, seqs, tol, model = _golden_model(golden_dir, name)
    shared_seqs = _prefixed_prompts(36, MODEL_TAILS, cfg["vocab_size"], 36)
    assert max(len(s) for s in shared_seqs) <= cfg["max_position_embeddings"]
    for prune in (True, False):
        model.set_last_layer_pruning(prune)
        shared = model.prefill_verbalize(shared_seqs, LABELS, share_prefix=True)
        plain = model.prefill_verbalize(shared_seqs, LABELS, share_prefix=False)
        assert torch.isfinite(plain).all() and torch.equal(shared, plain), prune
    pruned = model.set_last_layer_pruning(True).last_logits(seqs).cpu().numpy()
    full = model.set_last_layer_pruning(False).last_logits(seqs).cpu().numpy()
    latency = model.set_last_layer_pruning(True).set_variants(5, 0).last_logits(seqs).cpu().numpy()
    print(f"{name}: pruned-full {np.abs(pruned - full).max():.4f}, latency-default {np.abs(latency - pruned).max():.4f}, tolerance {tol:.4f}")
    assert np.abs(pruned - full).max() < tol and np.abs(full - z["logits_bf16"]).max() < tol
    assert np.abs(latency - pruned).max() < tol
    assert np.abs(latency - z["logits_fp32"]).max() < tol and np.abs(latency - z["logits_bf16"]).max() < tol


def test_set_qk_norm_checks_its_arrays_and_null_restores_the_llama_scores(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd._lib import lib
    from llamarec_amd.llm import LlamaRanker

    L = lib()
    z, cfg, sd, seqs, tol, model = _golden_model(golden_dir, "hd128_gqa")
    nl = cfg["num_hidden_layers"]
    before = model.prefill_verbalize(seqs, LABELS)

    def arrays():
        return ((C.c_void_p * nl)(*[model._tensors[f"{i}.q_norm"].data_ptr() for i in range(nl)]),
                (C.c_void_p * nl)(*[model._tensors[f"{i}.k_norm"].data_ptr() for i in range(nl)]))

    qa, ka = arrays()
    assert L.lr_llama_set_qk_norm(model._h, qa, None) == LR_EINVAL and b"both" in L.lr_last_error()
    assert L.lr_llama_set_qk_norm(model._h, None, ka) == LR_EINVAL
    ka[nl - 1] = None
    assert L.lr_llama_set_qk_norm(model._h, qa, ka) == LR_EINVAL and b"null norm" in L.lr_last_error()
    ka[nl - 1] = model._tensors[f"{nl - 1}.k_norm"].data_ptr() + 2
    assert L.lr_llama_set_qk_norm(model._h, qa, ka) == LR_EINVAL and b"aligned" in L.lr_last_error()
    assert torch.equal(model.prefill_verbalize(seqs, LABELS), before)                  # the handle kept its norms
    # folded norms, biases and a Gemma-2 extension are refused on a handle with q/k norms ...
    w = model._tensors["0.wqkv"]
    fold = (C.c_void_p * nl)(*([w.data_ptr()] * nl))
    assert L.lr_llama_set_folded_norms(model._h, fold, fold) == LR_EUNSUPPORTED and b"q/k norms" in L.lr_last_error()
    assert L.lr_llama_set_qkv_bias(model._h, fold) == LR_EUNSUPPORTED and b"q/k norms" in L.lr_last_error()
    with pytest.raises(NotImplementedError, match="q/k norms"):
        model.set_fold_norms(True)
    assert torch.equal(model.prefill_verbalize(seqs, LABELS), before)
    # NULL / NULL: the scores of the same weights loaded as a Llama (no norms), kernel for kernel
    llama_cfg = {k: v for k, v in cfg.items() if k != "model_type"}
    llama_sd = dict({k: v for k, v in sd.items() if "_norm.weight" not in k or "layernorm" in k},
                    **{"lm_head.weight": sd["model.embed_tokens.weight"]})
    llama = LlamaRanker.from_state_dict(llama_sd, llama_cfg)
    assert llama.family == "llama" and "0.q_norm" not in llama._tensors
    want = llama.prefill_verbalize(seqs, LABELS)
    assert L.lr_llama_set_qk_norm(model._h, None, None) == 0
    bare = model.prefill_verbalize(seqs, LABELS)
    assert torch.equal(bare, want) and not torch.equal(bare, before)
    # ... and in the other order: q/k norms are refused on a handle with folded norms or biases
    good_q, good_k = arrays()
    assert L.lr_llama_set_folded_norms(model._h, fold, fold) == 0
    assert L.lr_llama_set_qk_norm(model._h, good_q, good_k) == LR_EUNSUPPORTED and b"folded" in L.lr_last_error()
    assert L.lr_llama_set_folded_norms(model._h, None, None) == 0
    bias = torch.zeros(w.shape[0], dtype=torch.bfloat16, device="cuda")
    barr = (C.c_void_p * nl)(*([bias.data_ptr()] * nl))
    assert L.lr_llama_set_qkv_bias(model._h, barr) == 0
    assert L.lr_llama_set_qk_norm(model._h, good_q, good_k) == LR_EUNSUPPORTED and b"biases" in L.lr_last_error()
    assert L.lr_llama_set_qkv_bias(model._h, None) == 0
    assert L.lr_llama_set_qk_norm(model._h, good_q, good_k) == 0
    assert torch.equal(model.prefill_verbalize(seqs, LABELS), before)
    model._qk_norm_arrs = (good_q, good_k)
    # Gemma-2: an extension needs the Gemma norm, and on such a handle q/k norms are refused (both orders)
    ext = A.LrGemma2Ext(attn_softcap=0.0, final_softcap=0.0, attn_scale=0.0)
    assert L.lr_llama_set_gemma2(model._h, C.byref(ext)) == LR_EUNSUPPORTED
    from llamarec_amd.synth import synth_gemma2_state

    g2c = dict(model_type="gemma2", vocab_size=64, hidden_size=256, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
               num_key_value_heads=1, head_dim=128, max_position_embeddings=256, rms_norm_eps=1e-6, rope_theta=10000.0,
               hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=128, attn_logit_softcapping=50.0,
               final_logit_softcapping=30.0, sliding_window=4096)
    g2 = LlamaRanker.from_state_dict(synth_gemma2_state(g2c, 1), g2c)
    assert L.lr_llama_set_qk_norm(g2._h, good_q, good_k) == LR_EUNSUPPORTED and b"Gemma-2" in L.lr_last_error()
    assert L.lr_llama_set_gemma2(g2._h, None) == 0 and L.lr_llama_set_qk_norm(g2._h, good_q, good_k) == 0
    ext2, keep = g2.gemma2_ext()
    assert L.lr_llama_set_gemma2(g2._h, C.byref(ext2)) == LR_EUNSUPPORTED and b"q/k norms" in L.lr_last_error()
    assert L.lr_llama_set_qk_norm(g2._h, None, None) == 0 and L.lr_llama_set_gemma2(g2._h, C.byref(ext2)) == 0


def test_full_width_qwen3_fast_vs_generic_and_restatement():
    """Qwen3-0.6B's layer shape (16 heads of 128 on 8 KV heads over a hidden size of 1024), 2 layers, random weights, prompts of
    460 and 1 125 tokens: the fast path (256-tile GEMMs storing plainly, the sweep, attention variant 2, pruned last layer with
    its K | V and last-row Q sweeps) against the generic kernels, and both against the fp32 torch restatement on the GPU; the
    bars of test_full_width_gemma_fast_vs_generic_and_restatement."""
    from llamarec_amd.llm import QWEN3_0_6B, LlamaRanker

    cfg = dict(QWEN3_0_6B, num_hidden_layers=2, vocab_size=32000)
    sd = QR.random_qwen3_state(cfg, seed=7, device="cuda")
    model = LlamaRanker.from_state_dict(sd, cfg)
    rng = np.random.default_rng(2)
    lens = [460, 1125]
    seqs = [np.concatenate([[2], rng.integers(3, 32000, size=n - 1)]).astype(np.int32) for n in lens]
    label_ids = list(range(100, 120))
    fast = model.prefill_verbalize(seqs, label_ids).cpu().numpy()
    gen = model.set_variants(1, 1).prefill_verbalize(seqs, label_ids).cpu().numpy()
    lat = model.set_variants(5, 0).prefill_verbalize(seqs[:1], label_ids).cpu().numpy()
    model.set_variants(0, 0)
    ref = QR.last_logits(sd, cfg, seqs, torch.float32, device="cuda")[:, label_ids]
    ones = QR.last_logits(sd, cfg, seqs, torch.float32, device="cuda", mutant="ones_norm")[:, label_ids]
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"qwen3-0.6b: max |ref| {np.abs(ref).max():.3f}, fast-ref {np.abs(fast - ref).max():.4f}, gen-ref {np.abs(gen - ref).max():.4f}, "
          f"fast-gen {np.abs(fast - gen).max():.4f}, ones-ref {np.abs(ones - ref).max():.4f}")
    assert np.isfinite(fast).all() and float(np.abs(fast).max()) > 0.05
    assert np.abs(fast - gen).max() <= 5e-2 * scale
    assert np.abs(fast - ref).max() <= 1e-1 * scale and np.abs(gen - ref).max() <= 1e-1 * scale
    assert np.abs(lat - fast[:1]).max() <= 5e-2 * scale
    alone = model.prefill_verbalize([seqs[1]], label_ids).cpu().numpy()
    assert np.array_equal(alone[0], fast[1])
