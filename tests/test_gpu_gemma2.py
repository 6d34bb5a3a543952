"""GPU: the Gemma-2 ranker -- soft-capped head_dim-256 MFMA attention (llama_attn_hd256_softcap.hip) and the cap in the generic
kernel, the sandwich-norm kernel, the final soft cap, and the whole scoring path against the reference's goldens and the torch
restatement (tests/gemma2_ref.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llamarec_amd.synth import bf16_round, hash_uniform, synth_gemma2_state
from tests.gen_goldens_gemma2 import golden_tolerance
from tests.test_gemma2_host import GEMMA2_GOLDENS, load_gemma2_golden
from tests.test_gpu_attn_prefix import _bits, _prefix_layout
from tests.test_gpu_llama import dev_bf16, host_f32

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
POISON = 0x7FC0
HD = 256
LENS = [1, 63, 64, 65, 130, 257]      # every side of the 64-key block and the 128-row tile
ATTN_BOUND = 1.5e-2                   # variant 4's own (test_hd256_attention_vs_numpy)
# (name, cap, scale (0 = head_dim ** -0.5), gain on q): rows of unit-variance values give pre-cap scores a standard deviation
# of 16 * scale * gain -- 32 for "cap50" (a good part of them in the knee of the tanh), 1 and 4 for the two small caps
SETTINGS = [("cap50", 50.0, 0.0, 32.0), ("cap0125", 0.125, 0.0, 1.0), ("cap1_scale4th", 1.0, 0.25, 1.0)]


def _lib():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def softcap_call(rows_d, seg, P, nh, nkv, hd, scale, cap, variant, guard=3):
    """lr_attention_varlen_softcap on device rows: (rc, bf16 bits [n + guard][nh * hd])."""
    L, st = _lib()
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    n = int(seg[-1])
    out = torch.full((n + guard, nh * hd), POISON, dtype=torch.int16, device="cuda")
    segd = torch.from_numpy(seg).cuda()
    rc = L.lr_attention_varlen_softcap(rows_d.data_ptr(), out.data_ptr(), segd.data_ptr(), seg.ctypes.data, len(seg) - 1, P, nh,
                                       nkv, hd, scale, cap, variant, st)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def softcap_ref64(qkv, cu, nh, nkv, hd, scale, cap):
    """float64 causal attention with cap * tanh(s * scale / cap) (cap None: none), nothing rounded."""
    n = qkv.shape[0]
    x = qkv.astype(np.float64)
    out = np.zeros((n, nh * hd))
    for b in range(len(cu) - 1):
        s, e = int(cu[b]), int(cu[b + 1])
        T = e - s
        q = x[s:e, : nh * hd].reshape(T, nh, hd)
        k = x[s:e, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd)
        v = x[s:e, (nh + nkv) * hd:].reshape(T, nkv, hd)
        mask = np.tril(np.ones((T, T), bool))
        for h in range(nh):
            sc = (q[:, h] @ k[:, h // (nh // nkv)].T) * scale
            if cap is not None:
                sc = cap * np.tanh(sc / cap)
            sc = np.where(mask, sc, -np.inf)
            p = np.exp(sc - sc.max(-1, keepdims=True))
            out[s:e, h * hd:(h + 1) * hd] = (p @ v[:, h // (nh // nkv)]) / p.sum(-1, keepdims=True)
    return out


_DATA = {}


def _data(nh, nkv, gain, lens=LENS, seed=0):
    key = (nh, nkv, gain, tuple(lens), seed)
    if key not in _DATA:
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        qkv = bf16_round(hash_uniform(7000 + nh * 100 + nkv + seed, (int(cu[-1]), (nh + 2 * nkv) * HD), 1.0))
        qkv[:, : nh * HD] *= gain       # a power of two: still bf16 values
        _DATA[key] = (qkv, cu)
    return _DATA[key]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: s[0])
@pytest.mark.parametrize("nh,nkv", [(8, 4), (16, 8), (4, 1)])
def test_softcap_attention_vs_float64(nh, nkv, setting):
    name, cap, scale, gain = setting
    qkv, cu = _data(nh, nkv, gain)
    s = scale if scale > 0 else HD ** -0.5
    ref = softcap_ref64(qkv, cu, nh, nkv, HD, s, cap)
    uncapped = softcap_ref64(qkv, cu, nh, nkv, HD, s, None)
    moved = np.abs(uncapped - ref).max()
    print(f"softcap attention {name} nh={nh} nkv={nkv}: capped vs uncapped reference {moved:.3f}")
    assert moved > 10 * ATTN_BOUND, moved          # a kernel that ignores the cap fails below
    rows = _bits(qkv)
    n = int(cu[-1])
    for variant in (4, 0, 1):                      # the capped MFMA kernel, auto (the same), the generic kernel with the cap
        rc, got = softcap_call(rows, cu, 0, nh, nkv, HD, scale, cap, variant)
        assert rc == 0, _lib()[0].lr_last_error()
        assert (got[n:].view(np.uint16) == POISON).all(), "guard rows written"
        g = host_f32(torch.from_numpy(got[:n]))
        assert np.isfinite(g).all()
        err = np.abs(g - ref).max()
        print(f"  variant {variant}: max |got - ref| {err:.5f}")
        assert err < ATTN_BOUND, (variant, err)


@pytest.mark.parametrize("P", [63, 64, 65, 129])
def test_softcap_prefix_and_last_row_forms_are_bit_identical_to_the_whole_prompt_kernel(P):
    nh, nkv, cap, scale = 4, 2, 50.0, 1.0 / 12.0
    tails = [1, 4, 70, 130, 61]
    cu = np.concatenate([[0], np.cumsum([P + t for t in tails])]).astype(np.int64)
    qkv = bf16_round(hash_uniform(31 + P, (int(cu[-1]), (nh + 2 * nkv) * HD), 1.0))
    qkv[:, : nh * HD] *= 32.0      # scores of standard deviation 43 under the cap of 50
    for b in range(1, len(tails)):
        qkv[cu[b]:cu[b] + P] = qkv[:P]
    rc, full = softcap_call(_bits(qkv), cu, 0, nh, nkv, HD, scale, cap, 4, guard=0)
    assert rc == 0, _lib()[0].lr_last_error()
    rows, seg, src = _prefix_layout(qkv, cu, P)
    for v in (4, 0):
        rc, got = softcap_call(_bits(rows), seg, P, nh, nkv, HD, scale, cap, v)
        assert rc == 0, _lib()[0].lr_last_error()
        n = int(seg[-1])
        assert (got[n:].view(np.uint16) == POISON).all()
        assert np.array_equal(got[:n], full[src]), (P, v)
    # the last-row form: one query row per prompt, with and without the shared prefix
    L, st = _lib()
    B = len(tails)
    q_last = _bits(np.ascontiguousarray(qkv[cu[1:] - 1, : nh * HD]))
    for rows_np, seg_np, p in ((rows, seg, P), (qkv, cu.astype(np.int32), 0)):
        kv = _bits(np.ascontiguousarray(rows_np[:, nh * HD:]))
        seg_np = np.ascontiguousarray(seg_np, dtype=np.int32)
        segd = torch.from_numpy(seg_np).cuda()
        out = torch.full((B + 3, nh * HD), POISON, dtype=torch.int16, device="cuda")
        rc = L.lr_attention_last_rows_softcap(kv.data_ptr(), q_last.data_ptr(), out.data_ptr(), segd.data_ptr(), seg_np.ctypes.data,
                                              len(seg_np) - 1, p, nh, nkv, HD, scale, cap, 4, st)
        torch.cuda.synchronize()
        assert rc == 0, L.lr_last_error()
        got = out.cpu().numpy()
        assert (got[B:].view(np.uint16) == POISON).all()
        assert np.array_equal(got[:B], full[cu[1:] - 1]), (P, p)


def test_softcap_rows_are_batch_invariant():
    nh, nkv, cap = 8, 4, 50.0
    lens = [300, 129, 5, 257]
    qkv, cu = _data(nh, nkv, 32.0, lens=lens, seed=5)
    rc, full = softcap_call(_bits(qkv), cu, 0, nh, nkv, HD, 0.0, cap, 4, guard=0)
    assert rc == 0
    for b in (0, 2, 3):
        rc, alone = softcap_call(_bits(qkv[cu[b]:cu[b + 1]]), np.array([0, lens[b]]), 0, nh, nkv, HD, 0.0, cap, 4, guard=0)
        assert rc == 0 and np.array_equal(alone, full[cu[b]:cu[b + 1]]), b


@pytest.mark.parametrize("hd,variant,P", [(256, 4, 0), (256, 4, 64), (256, 0, 65), (128, 2, 36), (64, 5, 0)])
def test_cap_zero_is_bit_identical_to_the_uncapped_entry_point(hd, variant, P):
    L, st = _lib()
    nh, nkv = 4, 2
    tails = [3, 70, 130]
    cu = np.concatenate([[0], np.cumsum([P + t for t in tails])]).astype(np.int64)
    qkv = bf16_round(hash_uniform(77 + hd, (int(cu[-1]), (nh + 2 * nkv) * hd), 1.0))
    for b in range(1, len(tails)):
        qkv[cu[b]:cu[b] + P] = qkv[:P]
    rows, seg, _ = _prefix_layout(qkv, cu, P)
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    rows_d, segd = _bits(rows), torch.from_numpy(seg).cuda()
    want = torch.full((int(seg[-1]), nh * hd), POISON, dtype=torch.int16, device="cuda")
    assert L.lr_attention_varlen_prefix(rows_d.data_ptr(), want.data_ptr(), segd.data_ptr(), seg.ctypes.data, len(seg) - 1, P, nh,
                                        nkv, hd, variant, st) == 0, L.lr_last_error()
    for scale in (0.0, float(np.float32(1.0) / np.sqrt(np.float32(hd)))):
        rc, got = softcap_call(rows_d, seg, P, nh, nkv, hd, scale, 0.0, variant, guard=0)
        assert rc == 0, L.lr_last_error()
        assert np.array_equal(got, want.cpu().numpy()), scale
    rc, _ = softcap_call(rows_d, seg, P, nh, nkv, hd, 0.3, 0.0, variant)        # a foreign scale needs the cap
    assert rc == LR_EUNSUPPORTED and b"without a cap" in L.lr_last_error()


def test_softcap_refusals_leave_the_output_untouched():
    L, st = _lib()
    qkv, cu = _data(4, 1, 1.0)
    rows = _bits(qkv)
    for hd, nh, nkv, variant, want in [(256, 4, 1, 2, LR_EUNSUPPORTED), (256, 4, 1, 3, LR_EUNSUPPORTED),
                                       (256, 4, 1, 5, LR_EUNSUPPORTED), (256, 4, 1, 6, LR_EUNSUPPORTED),
                                       (128, 8, 2, 2, LR_EUNSUPPORTED), (64, 16, 4, 5, LR_EUNSUPPORTED),
                                       (256, 4, 1, 7, LR_EINVAL)]:
        rc, got = softcap_call(rows, cu, 0, nh, nkv, hd, 0.0, 50.0, variant)
        assert rc == want, (hd, variant, rc, L.lr_last_error())
        assert (got.view(np.uint16) == POISON).all()
    for scale, cap in [(-1.0, 50.0), (0.0, -50.0), (float("nan"), 50.0), (0.0, float("inf")), (float("inf"), 1.0)]:
        rc, got = softcap_call(rows, cu, 0, 4, 1, 256, scale, cap, 4)
        assert rc == LR_EINVAL and (got.view(np.uint16) == POISON).all(), (scale, cap, rc)
    rc, got = softcap_call(rows, np.array([0, 5, 5, 580]), 0, 4, 1, 256, 0.0, 50.0, 4)      # an empty segment
    assert rc == LR_EINVAL and (got.view(np.uint16) == POISON).all()
    # the generic kernel reads no shared prefix, capped or not
    seg = np.array([0, 64, 100, 580])
    rc, got = softcap_call(rows, seg, 64, 4, 1, 256, 0.0, 50.0, 1)
    assert rc == LR_EUNSUPPORTED and (got.view(np.uint16) == POISON).all()


# ---- the sandwich-norm kernel ------------------------------------------------------------------------------------------
def _gemmanorm(v, w, eps):
    """bf16(v * rstd * (1 + w)) with fp32 arithmetic (torch, on the GPU): v bf16 [rows][d], w bf16 [d]."""
    vf = v.float()
    return (vf * torch.rsqrt(vf.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w.float())).to(torch.bfloat16)


def _close_in_the_project_form(got, want):
    got, want = got.float(), want.float()
    err = (got - want).abs()
    assert (err <= want.abs() * 2 ** -7 + 1e-6).float().mean().item() >= 0.99
    step = torch.exp2(torch.floor(torch.log2(want.abs().amax(-1, keepdim=True))) - 7)      # one bf16 step of the row's largest
    assert bool((err <= step).all()), float((err / step).max())


@pytest.mark.parametrize("rows", [1, 7, 300])
@pytest.mark.parametrize("d", [256, 2304, 3584])
def test_residual_postnorm_kernel(d, rows):
    L, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(d + rows)
    x = (torch.randn(rows, d, generator=g, device="cuda") * 3.0).to(torch.bfloat16)
    h = (torch.randn(rows, d, generator=g, device="cuda") * 0.7).to(torch.bfloat16)
    w_out = (torch.randn(d, generator=g, device="cuda") * 0.3).to(torch.bfloat16)
    w_next = (torch.randn(d, generator=g, device="cuda") * 0.3).to(torch.bfloat16)
    eps = 1e-6
    want_x = (x.float() + _gemmanorm(h, w_out, eps).float()).to(torch.bfloat16)
    outs = {}
    for mode in ("no_next", "next", "in_place"):
        xg, hg = x.clone(), h.clone()
        xn = torch.full((rows + 1, d), float("nan"), dtype=torch.bfloat16, device="cuda")
        xn_arg = None if mode == "no_next" else (hg if mode == "in_place" else xn)
        rc = L.lr_residual_postnorm_bf16(xg.data_ptr(), hg.data_ptr(), w_out.data_ptr(),
                                         None if mode == "no_next" else w_next.data_ptr(),
                                         None if xn_arg is None else xn_arg.data_ptr(), rows, d, eps, st)
        torch.cuda.synchronize()
        assert rc == 0, L.lr_last_error()
        _close_in_the_project_form(xg, want_x)
        if mode == "no_next":
            assert torch.equal(hg, h) and bool(torch.isnan(xn.float()).all())
        else:
            got_xn = hg if mode == "in_place" else xn[:rows]
            _close_in_the_project_form(got_xn, _gemmanorm(xg, w_next, eps))         # the norm of the row the kernel wrote
            assert mode == "in_place" or (torch.equal(hg, h) and bool(torch.isnan(xn[rows].float()).all()))
        outs[mode] = (xg.view(torch.int16).clone(), None if mode == "no_next" else got_xn.view(torch.int16).clone())
    assert torch.equal(outs["no_next"][0], outs["next"][0]) and torch.equal(outs["next"][0], outs["in_place"][0])
    assert torch.equal(outs["next"][1], outs["in_place"][1])
    # the fused second norm carries the bits of the prefill's own RMSNorm pass on the row the kernel wrote
    two = torch.full((rows, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert L.lr_rmsnorm_bf16(outs["no_next"][0].data_ptr(), w_next.data_ptr(), two.data_ptr(), rows, d, eps, 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(two.view(torch.int16), outs["next"][1])


def test_residual_postnorm_refusals():
    L, st = _lib()
    t = torch.zeros(4, 16, dtype=torch.int16, device="cuda")
    p = t.data_ptr()
    assert L.lr_residual_postnorm_bf16(p, p, p, p, None, 4, 16, 1e-6, st) == LR_EINVAL       # w_next without xn
    assert L.lr_residual_postnorm_bf16(p, p, p, None, p, 4, 16, 1e-6, st) == LR_EINVAL
    assert L.lr_residual_postnorm_bf16(None, p, p, None, None, 4, 16, 1e-6, st) == LR_EINVAL
    assert L.lr_residual_postnorm_bf16(p, p, p, None, None, 4, 12, 1e-6, st) == LR_EUNSUPPORTED
    assert L.lr_residual_postnorm_bf16(p, p, p, None, None, 1, 8200, 1e-6, st) == LR_EUNSUPPORTED
    assert L.lr_rmsnorm_bf16(p, p, None, 4, 16, 1e-6, 1, st) == LR_EINVAL
    assert L.lr_rmsnorm_bf16(p, p, p, 4, 12, 1e-6, 1, st) == LR_EINVAL
    assert L.lr_rmsnorm_bf16(p, p, p, 4, 16, 1e-6, 2, st) == LR_EINVAL
    torch.cuda.synchronize()
    assert not t.any()


# ---- the prefill ---------------------------------------------------------------------------------------------------------
_MODELS = {}


def _golden_model(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker

    if name not in _MODELS:
        z, cfg, sd, seqs = load_gemma2_golden(golden_dir, name)
        _MODELS[name] = (z, cfg, sd, seqs, LlamaRanker.from_state_dict(sd, cfg))
    z, cfg, sd, seqs, model = _MODELS[name]
    model.set_variants(0, 0).set_last_layer_pruning(True)
    return z, cfg, sd, seqs, model


@pytest.mark.parametrize("name", GEMMA2_GOLDENS)
@pytest.mark.parametrize("variants", [(0, 0), (1, 1), (4, 4), (5, 0)])
def test_gemma2_prefill_vs_reference_goldens(golden_dir, name, variants):
    z, cfg, sd, seqs, model = _golden_model(golden_dir, name)
    assert model.family == "gemma2"
    # Gemma v1's 3e-2 while the goldens' own two precisions agree to a third of it, otherwise three times their distance
    # (0.13 / 0.20 / 0.13 for the three archives: their logits reach 7.8, where a bf16 step is 0.03)
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    model.set_variants(*variants)
    if variants[0] == 4 and cfg["hidden_size"] % 256:
        # attention variant 4 with a cap at head_dim 16 is the generic kernel, but GEMM variant 4 is "an error if a shape does
        # not fit" (include/llamarec_mi355x.h) and the 64-wide model's products do not: a refusal, as Gemma v1's (4, 4) case
        with pytest.raises(RuntimeError, match="gemm variant 4"):
            model.last_logits(seqs)
        model.set_variants(1, 4)                  # the attention half of the pair alone: the generic kernel with the cap
    got = model.last_logits(seqs).cpu().numpy()
    assert got.shape == z["logits_bf16"].shape and np.array_equal(got, bf16_round(got))
    print(f"gemma2 {name} {variants}: tol {tol:.4f}, vs bf16 {np.abs(got - z['logits_bf16']).max():.4f}, "
          f"vs fp32 {np.abs(got - z['logits_fp32']).max():.4f}")
    assert np.abs(got - z["logits_bf16"]).max() < tol
    assert np.abs(got - z["logits_fp32"]).max() < tol
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])
    assert np.abs(scores - z["scores_bf16"]).max() < tol


@pytest.mark.parametrize("name", ["tiny_hd256_gqa", "tiny_hd256_qpas"])
def test_gemma2_last_layer_pruning_matches_full_last_layer(golden_dir, name):
    z, cfg, sd, seqs, model = _golden_model(golden_dir, name)
    pruned = model.last_logits(seqs).cpu().numpy()
    full = model.set_last_layer_pruning(False).last_logits(seqs).cpu().numpy()
    model.set_last_layer_pruning(True)
    assert np.abs(pruned - full).max() < 2e-2
    assert np.abs(full - z["logits_bf16"]).max() < golden_tolerance(z["logits_fp32"], z["logits_bf16"])


@pytest.mark.parametrize("name", ["tiny_hd256_gqa", "tiny_hd256_qpas"])
@pytest.mark.parametrize("P", [36, 64, 70])
def test_gemma2_shared_prefix_scores_are_bit_identical(golden_dir, name, P):
    from llamarec_amd.llm import common_prefix_len, pack_prompts

    z, cfg, sd, seqs, model = _golden_model(golden_dir, name)
    rng = np.random.default_rng(P)
    head = np.concatenate([[2], rng.integers(3, cfg["vocab_size"], size=P - 1)])
    prompts = [np.concatenate([head, [3 + b], rng.integers(3, cfg["vocab_size"], size=n)]).astype(np.int32)
               for b, n in enumerate([0, 5, 61, 100])]
    assert common_prefix_len(*pack_prompts(prompts)) == P
    label_ids = list(z["label_ids"])
    shared = model.prefill_verbalize(prompts, label_ids, share_prefix=True)
    plain = model.prefill_verbalize(prompts, label_ids, share_prefix=False)
    assert torch.isfinite(shared).all() and torch.equal(shared, plain)
    full = model.set_last_layer_pruning(False).prefill_verbalize(prompts, label_ids, share_prefix=True)
    assert torch.equal(full, model.prefill_verbalize(prompts, label_ids, share_prefix=False))
    model.set_last_layer_pruning(True)


@pytest.mark.parametrize("which,lens", [("2b", [460, 1125, 700, 5]), ("9b", [600, 1000])])
def test_full_width_gemma2_fast_vs_generic_and_restatement(which, lens):
    """Gemma-2-2B (8 / 4 x 256 heads on 2304) and -9B (16 / 8 on 3584) layer shapes, 2 layers, random weights, long prompts:
    the fast path (256-tile GEMMs, the capped MFMA attention, the sandwich-norm kernel, pruned last layer) against the generic
    kernels, both against the fp32 torch restatement on the GPU, and the latency mode against the fast path. The bounds are
    those of test_full_width_gemma_fast_vs_generic_and_restatement."""
    from llamarec_amd.llm import GEMMA2_2B, GEMMA2_9B, LlamaRanker
    from tests import gemma2_ref as G

    cfg = dict(GEMMA2_2B if which == "2b" else GEMMA2_9B, num_hidden_layers=2, vocab_size=32000)
    sd = G.random_gemma2_state(cfg, seed=7, device="cuda")
    model = LlamaRanker.from_state_dict(sd, cfg)
    rng = np.random.default_rng(2)
    seqs = [np.concatenate([[2], rng.integers(3, 32000, size=n - 1)]).astype(np.int32) for n in lens]
    label_ids = list(range(100, 120))
    fast = model.prefill_verbalize(seqs, label_ids).cpu().numpy()
    gen = model.set_variants(1, 1).prefill_verbalize(seqs, label_ids).cpu().numpy()
    lat = model.set_variants(5, 0).prefill_verbalize(seqs[:1], label_ids).cpu().numpy()
    model.set_variants(0, 0)
    ref = G.last_logits(sd, cfg, seqs, torch.float32, device="cuda")[:, label_ids]
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"gemma-2-{which}: max |ref| {np.abs(ref).max():.3f}, fast-ref {np.abs(fast - ref).max():.4f}, "
          f"gen-ref {np.abs(gen - ref).max():.4f}, fast-gen {np.abs(fast - gen).max():.4f}, lat-fast {np.abs(lat - fast[:1]).max():.4f}")
    assert np.isfinite(fast).all() and float(np.abs(fast).max()) > 0.05
    assert np.abs(fast - gen).max() <= 5e-2 * scale
    assert np.abs(fast - ref).max() <= 1e-1 * scale and np.abs(gen - ref).max() <= 1e-1 * scale
    assert np.abs(lat - fast[:1]).max() <= 5e-2 * scale
    alone = model.prefill_verbalize([seqs[1]], label_ids).cpu().numpy()        # a prompt's scores do not depend on the batch
    assert np.array_equal(alone[0], fast[1])


@pytest.mark.parametrize("hd,nh,nkv", [(128, 2, 1), (64, 4, 2)])
def test_capped_handle_at_head_dim_64_and_128_scores_prompts_that_share_a_prefix(hd, nh, nkv):
    """A Gemma-2 config whose head_dim has no capped MFMA kernel (gemma-2-27b's 128; 64) runs the generic kernel with the cap.
    That kernel reads no shared prefix, so the prefill must run every prompt whole although the UNCAPPED kernels of these
    head sizes would share it -- under the default call, where the ranker's prompts always share their template text."""
    from llamarec_amd.llm import LlamaRanker, common_prefix_len, pack_prompts
    from tests import gemma2_ref as G

    cfg = dict(TINY_ONLINE, vocab_size=320, num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd,
               query_pre_attn_scalar=hd)
    sd = synth_gemma2_state(cfg, 21 + hd, std=0.1)
    model = LlamaRanker.from_state_dict(sd, cfg)
    rng = np.random.default_rng(hd)
    head = np.concatenate([[2], rng.integers(3, 320, size=69)])
    prompts = [np.concatenate([head, [3 + b], rng.integers(3, 320, size=n)]).astype(np.int32) for b, n in enumerate([0, 5, 61, 130])]
    assert common_prefix_len(*pack_prompts(prompts)) == 70
    label_ids = list(range(40, 60))
    r32 = G.last_logits(sd, cfg, prompts)[:, label_ids]
    rbf = G.last_logits(sd, cfg, prompts, torch.bfloat16)[:, label_ids]
    nocap = G.last_logits(sd, dict(cfg, attn_logit_softcapping=None), prompts)[:, label_ids]
    tol = golden_tolerance(r32, rbf)                 # the restatement's own two precisions, as for the goldens
    assert np.abs(nocap - r32).max() >= 10 * tol     # the attention cap matters on this model
    got = model.prefill_verbalize(prompts, label_ids)                        # share_prefix defaults to True
    plain = model.prefill_verbalize(prompts, label_ids, share_prefix=False)
    assert torch.equal(got, plain)
    g = got.cpu().numpy()
    print(f"capped hd {hd}: tol {tol:.4f}, vs bf16 {np.abs(g - rbf).max():.4f}, vs fp32 {np.abs(g - r32).max():.4f}, "
          f"uncapped restatement {np.abs(nocap - r32).max():.3f} away")
    assert np.abs(g - rbf).max() < tol and np.abs(g - r32).max() < tol
    for variants in ((1, 1), (0, 4), (5, 0)):                                # generic either way; 4 with a cap off 256 too
        v = model.set_variants(*variants).prefill_verbalize(prompts, label_ids).cpu().numpy()
        assert np.abs(v - rbf).max() < tol and np.abs(v - r32).max() < tol, variants
    for attn in (2, 5) if hd == 128 else (5, 6):                             # kernels without a capped form: refused by name
        with pytest.raises(RuntimeError, match="soft-capped"):
            model.set_variants(0, attn).prefill_verbalize(prompts, label_ids)
    assert torch.equal(model.set_variants(0, 0).prefill_verbalize(prompts, label_ids), got)


def test_a_cap_above_the_mfma_range_runs_the_generic_kernel_at_head_dim_256():
    """The MFMA kernels' tanh has an absolute error that grows with the cap; caps above 256 go to the generic kernel."""
    nh, nkv, cap = 4, 1, 1000.0
    qkv, cu = _data(nh, nkv, 32.0)
    rows, n = _bits(qkv), int(cu[-1])
    ref = softcap_ref64(qkv, cu, nh, nkv, HD, HD ** -0.5, cap)
    rc, gen = softcap_call(rows, cu, 0, nh, nkv, HD, 0.0, cap, 1, guard=0)
    assert rc == 0
    for variant in (0, 4):
        rc, got = softcap_call(rows, cu, 0, nh, nkv, HD, 0.0, cap, variant, guard=0)
        assert rc == 0 and np.array_equal(got, gen), variant
    assert np.abs(host_f32(torch.from_numpy(gen)) - ref).max() < ATTN_BOUND
    rc, at_max = softcap_call(rows, cu, 0, nh, nkv, HD, 0.0, 256.0, 4, guard=0)          # the largest cap the MFMA kernels take
    assert rc == 0 and not np.array_equal(at_max, softcap_call(rows, cu, 0, nh, nkv, HD, 0.0, 256.0, 1, guard=0)[1])
    assert np.abs(host_f32(torch.from_numpy(at_max)) - softcap_ref64(qkv, cu, nh, nkv, HD, HD ** -0.5, 256.0)).max() < ATTN_BOUND
    rc, got = softcap_call(rows, np.array([0, 64, 100, n]), 64, nh, nkv, HD, 0.0, cap, 4)  # ... which reads no shared prefix
    assert rc == LR_EUNSUPPORTED and (got.view(np.uint16) == POISON).all()


def test_sandwich_norm_launches_write_profile_records(golden_dir):
    L, _ = _lib()
    z, cfg, sd, seqs, model = _golden_model(golden_dir, "tiny_hd256_gqa")
    model.last_logits(seqs)
    assert L.lr_profile_start(256) == 0
    model.last_logits(seqs)
    torch.cuda.synchronize()
    assert L.lr_profile_stop() == 0
    ms, work, launches = C.c_double(), C.c_double(), C.c_int64()
    assert L.lr_profile_collect(6, C.byref(ms), C.byref(work), C.byref(launches)) == 0
    nl, d, n, B = cfg["num_hidden_layers"], cfg["hidden_size"], int(sum(z["lens"])), len(seqs)
    assert launches.value == 2 * nl and ms.value > 0
    # five row passes of 2 d bytes with a next norm, three without (after the last layer's MLP); the pruned last layer on B rows
    assert work.value == 2 * d * ((nl - 1) * 2 * 5 * n + (5 + 3) * B)


TINY_ONLINE = dict(model_type="gemma2", vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                   num_attention_heads=2, num_key_value_heads=1, head_dim=256, max_position_embeddings=2048, rms_norm_eps=1e-6,
                   rope_theta=10000.0, hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=144,
                   attn_logit_softcapping=1.0, final_logit_softcapping=4.0, sliding_window=4096)


def test_gemma2_online_single_user_path():
    """demo/inference.py's flow with a Gemma-2 ranker, unchanged callers; the latency mode scores the same prompt."""
    from llamarec_amd import data as D
    from llamarec_amd import inference as I
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.lru import LRURec, init_lru_state_dict
    from llamarec_amd.verb import ManualVerbalizer
    from tests import gemma2_ref as G
    from tests.fake_tokenizer import FakeTokenizer

    ds = D.synthetic_dataset(num_users=5, num_items=400, seed=3)
    retr = LRURec.from_state_dict(init_lru_state_dict(400, seed=9))
    query = ds["train"][1][-7:]
    cands = I.retrieve_candidates(retr, query, top_k=20)
    prompt = I.generate_prompt(query, cands, ds["meta"])
    tok = FakeTokenizer()
    gsd = synth_gemma2_state(TINY_ONLINE, 11, std=0.1)
    ranker = LlamaRanker.from_state_dict(gsd, TINY_ONLINE)
    verb = ManualVerbalizer(tokenizer=tok, classes=list(range(20)), label_words={i: chr(65 + i) for i in range(20)})
    top = I.rank_candidates(ranker, tok, prompt, cands, verb, top_k=10)
    assert len(top) == 10 and set(top) <= set(cands)
    ids = np.asarray(tok(prompt)["input_ids"])
    r32 = G.last_logits(gsd, TINY_ONLINE, [ids])[0][verb.label_token_ids]
    rbf = G.last_logits(gsd, TINY_ONLINE, [ids], torch.bfloat16)[0][verb.label_token_ids]
    tol = golden_tolerance(r32, rbf)                 # the restatement's own two precisions, as for the goldens
    got = ranker.prefill_verbalize([ids], verb.label_token_ids)[0].cpu().numpy()
    lat = ranker.set_variants(5, 0).prefill_verbalize([ids], verb.label_token_ids)[0].cpu().numpy()
    print(f"online: tol {tol:.4f}, got-bf16 {np.abs(got - rbf).max():.4f}, got-fp32 {np.abs(got - r32).max():.4f}, "
          f"latency-fast {np.abs(lat - got).max():.4f}")
    assert np.abs(got - rbf).max() < tol and np.abs(got - r32).max() < tol
    assert np.abs(lat - rbf).max() < tol and np.abs(lat - r32).max() < tol


def test_gemma2_from_pretrained_with_default_args_is_nf4_like_the_reference(golden_dir, tmp_path):
    """As the Gemma v1 test: a local checkpoint directory (config.json with model_type gemma2, four norms per layer) loads
    with the parsed defaults, which include --llm_load_in_4bit; the Linears take the NF4 round trip, the norms do not."""
    from safetensors.torch import save_file

    from llamarec_amd import config as cfgmod
    from llamarec_amd.llm import LlamaRanker

    args = cfgmod.parse(["--dataset_code", "beauty", "--llm", "gemma2", "--eval_only"], model_code="llm")
    assert args.llm_load_in_4bit is True
    z, cfg, sd, seqs = load_gemma2_golden(golden_dir, "tiny_hd256_gqa")
    hf = str(tmp_path / "gemma2")
    os.makedirs(hf)
    json.dump(dict(cfg, architectures=["Gemma2ForCausalLM"], torch_dtype="bfloat16"), open(os.path.join(hf, "config.json"), "w"))
    save_file({n: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for n, v in sd.items()},
              os.path.join(hf, "model.safetensors"), metadata={"format": "pt"})
    loaded = LlamaRanker.from_pretrained(hf, load_in_4bit=args.llm_load_in_4bit)
    assert loaded.family == "gemma2" and loaded.hd == 256
    label_ids = list(z["label_ids"])
    got = loaded.prefill_verbalize(seqs, label_ids)
    direct = LlamaRanker.from_state_dict(sd, cfg, nf4=True).prefill_verbalize(seqs, label_ids)
    plain = LlamaRanker.from_pretrained(hf).prefill_verbalize(seqs, label_ids)
    assert torch.isfinite(got).all() and torch.equal(got, direct)
    assert not torch.equal(got, plain)                                       # the round trip really ran
    assert np.abs(plain.cpu().numpy() - z["scores_bf16"]).max() < golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    for i in range(cfg["num_hidden_layers"]):                                # name mapping: post_norm is the norm in front of the MLP
        assert torch.equal(loaded._tensors[f"{i}.post_norm"].float().cpu(),
                           torch.from_numpy(sd[f"model.layers.{i}.pre_feedforward_layernorm.weight"]))
        assert torch.equal(loaded._tensors[f"{i}.attn_out_norm"].float().cpu(),
                           torch.from_numpy(sd[f"model.layers.{i}.post_attention_layernorm.weight"]))


def test_train_ranker_gemma2_eval_only_end_to_end(tmp_path):
    """`train_ranker.py --llm gemma2 --eval_only` with default flags (NF4 on) scores the retrieved users through the Gemma-2
    ranker and writes the reference's metric files; training a Gemma-2 base is refused."""
    import pickle

    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    r = pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))
    assert r["test_users"], "the synthetic retriever retrieved nobody"
    out = str(tmp_path / "experiments" / "gemma2" / "synthetic")
    metrics, overall = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma2", "--eval_only",
                                          "--llm_retrieved_path", lru_root, "--export_root", out, "--llm_max_history", "5"])
    assert "test_NDCG@10" in metrics and 0.0 <= metrics["test_NDCG@10"] <= 1.0
    assert os.path.exists(os.path.join(out, "subset_metrics.json")) and os.path.exists(os.path.join(out, "overall_metrics.json"))
    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "gemma2", "--llm_retrieved_path", lru_root,
                           "--export_root", out])


def test_gemma2_handle_refuses_lora_folded_norms_and_bad_extension_words(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd.llm import LlamaRanker

    L, _ = _lib()
    z, cfg, sd, seqs, model = _golden_model(golden_dir, "tiny_hd256_gqa")
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    before = model.last_logits(seqs)
    with pytest.raises(NotImplementedError, match="folded"):
        model.set_fold_norms(True)
    nl = cfg["num_hidden_layers"]
    w = model._tensors["0.wqkv"]
    arr = (C.c_void_p * nl)(*([w.data_ptr()] * nl))
    assert L.lr_llama_set_folded_norms(model._h, arr, arr) == LR_EUNSUPPORTED
    assert L.lr_llama_set_folded_norms(model._h, None, None) == 0
    lc = A.LrLoraTrainConfig(r=8, alpha=32.0, dropout=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, seed=1)
    layers = (A.LrLlamaLayerWeightsT * nl)()
    wt = A.LrLlamaWeightsTDesc(layers=layers, lm_head_t=None)
    h = C.c_void_p()
    assert L.lr_llama_lora_create(model._h, C.byref(wt), C.byref(lc), None, 0, None, C.byref(h)) == LR_EUNSUPPORTED
    assert b"Llama base" in L.lr_last_error()
    # bad extension words: LR_EINVAL with a message, and the handle keeps scoring what it scored
    good, arrs = model.gemma2_ext()

    def ext(**kw):
        e = A.LrGemma2Ext(attn_softcap=good.attn_softcap, final_softcap=good.final_softcap, attn_scale=good.attn_scale)
        e.attn_out_norm, e.mlp_out_norm = arrs
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    null_layer = (C.c_void_p * nl)(*([arrs[0][0]] + [None] * (nl - 1)))
    one_reserved = (C.c_int32 * 5)(0, 0, 1, 0, 0)
    bad = [ext(attn_softcap=-1.0), ext(final_softcap=float("nan")), ext(attn_scale=float("inf")), ext(attn_scale=-0.5),
           ext(reserved=one_reserved), ext(attn_out_norm=None), ext(mlp_out_norm=None), ext(attn_out_norm=null_layer)]
    for e in bad:
        assert L.lr_llama_set_gemma2(model._h, C.byref(e)) == LR_EINVAL and L.lr_last_error()
        assert torch.equal(model.last_logits(seqs), before)
    assert L.lr_llama_set_gemma2(None, C.byref(good)) == LR_EINVAL
    # a foreign scale without a cap has no kernel; out-norms need the Gemma norm
    assert L.lr_llama_set_gemma2(model._h, C.byref(ext(attn_softcap=0.0, attn_scale=0.3))) == LR_EUNSUPPORTED
    assert torch.equal(model.last_logits(seqs), before)
    from llamarec_amd.synth import synth_llama_state

    lcfg = dict(vocab_size=320, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=2, max_position_embeddings=256, rms_norm_eps=1e-5, rope_theta=10000.0)
    llama = LlamaRanker.from_state_dict(synth_llama_state(lcfg, 5), lcfg)
    assert L.lr_llama_set_gemma2(llama._h, C.byref(good)) == LR_EUNSUPPORTED and b"Gemma norm" in L.lr_last_error()
    # ... and so does a cap alone: a Llama handle may have LoRA engines, whose training attention would stay uncapped
    llama_before = llama.last_logits(seqs[:2])
    assert L.lr_llama_set_gemma2(llama._h, C.byref(A.LrGemma2Ext(attn_softcap=50.0))) == LR_EUNSUPPORTED
    assert L.lr_llama_set_gemma2(llama._h, C.byref(A.LrGemma2Ext(final_softcap=30.0))) == LR_EUNSUPPORTED
    assert L.lr_llama_set_gemma2(llama._h, None) == 0
    assert torch.equal(llama.last_logits(seqs[:2]), llama_before)
    # NULL: back to the plain (Gemma v1) layer -- far from the goldens; the extension again: the same bits as before
    assert L.lr_llama_set_gemma2(model._h, None) == 0
    assert np.abs(model.last_logits(seqs).cpu().numpy() - z["logits_bf16"]).max() > 10 * tol
    assert L.lr_llama_set_gemma2(model._h, C.byref(good)) == 0
    assert torch.equal(model.last_logits(seqs), before)
