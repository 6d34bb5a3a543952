"""GPU: the Phi-3 ranker (--llm phi3) and attention variant 7, the head_dim-96 MFMA flash attention (llama_attn_hd96.hip,
llama_attn_hd96_prefix.hip), through the C ABI: the float64 bound of tests/stage2_ref.py, batch invariance, forced maximum
jumps, bit identity of the shared-prefix and last-row modes with the whole-prompt kernel, refusals, the 256-tile GEMM's rotary
epilogue at head_dim 96, and the scoring path on the committed Phi-3 goldens (tests/gen_goldens_phi3.py)."""
import json
import os

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, hash_uniform
from tests import stage2_ref as R
from tests.test_gpu_attn_prefix import GUARD, POISON, _bits, _full, _gemm_rows, _lib, _prefix_call, _prefix_layout, _prefixed_prompts, _whole_prompts
from tests.test_gpu_llama import attention
from tests.test_gpu_stage2_bounds import _bf16_ulp, _dev_bf16, _epi, _mutant_check, _operands, _report, _rope_table
from tests.test_phi3_host import PHI3_GOLDENS, load_phi3_golden

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
HD = 96
LENS = [1, 63, 64, 65, 127, 128, 129, 256, 257, 300, 600, 1125]
REGIMES = ("flat", "peaked", "large_v", "last_block")


def _attn96(qkv_d, cu, nh, nkv, variant, prefill_auto=False):
    """Whole prompts at head_dim 96 on NaN-poisoned outputs. prefill_auto: variant 0 as the prefill resolves it
    (lr_attention_varlen_prefix with prefix_len 0); stand-alone auto without a prefix keeps the generic kernel."""
    if not prefill_auto:
        return bf16_bits_to_f32(_full(qkv_d, cu, nh, nkv, HD, variant).view(np.uint16))
    seg = np.ascontiguousarray(cu, dtype=np.int32)
    rc, out = _prefix_call(qkv_d, seg, 0, nh, nkv, HD, 0)
    assert rc == 0, _lib()[0].lr_last_error()
    assert (out[int(seg[-1]):].view(np.uint16) == POISON).all()
    return bf16_bits_to_f32(out[: int(seg[-1])].view(np.uint16))


# ---- attention variant 7 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 2), (8, 1)])
def test_attention_hd96_within_bound(regime, nh, nkv):
    cu = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    qkv = R.attention_data(regime, cu, nh, nkv, HD)
    ref, _, bound, _ = R.attention_ref64(qkv, cu, nh, nkv, HD)
    qkv_d = _dev_bf16(qkv)
    bad = []
    outs = {}
    for what in ("v7", "prefill-auto", "v1"):
        got = _attn96(qkv_d, cu, nh, nkv, {"v7": 7, "v1": 1}.get(what, 0), prefill_auto=what == "prefill-auto")
        assert np.isfinite(got).all(), what
        r = R.ratio(got, ref, bound)
        print(f"attention {regime} hd=96 nh={nh} nkv={nkv} {what}: err/bound {r:.3f}")
        if not r <= 1.0:
            bad.append((what, r))
        outs[what] = got
    assert np.array_equal(outs["v7"], outs["prefill-auto"])   # the prefill's auto at head_dim 96 is variant 7
    _mutant_check(qkv, cu, nh, nkv, HD, ref, bound)
    assert not bad, bad


def test_attention_hd96_rows_are_batch_invariant():
    nh, nkv = 8, 2
    rng = np.random.default_rng(1)
    lens = [700, 129, 1125, 5]
    cu = np.concatenate([[0], np.cumsum(lens)])
    qkv = bf16_round(rng.standard_normal((cu[-1], (nh + 2 * nkv) * HD)).astype(np.float32))
    full = attention(qkv, cu, nh, nkv, HD, 7)
    for b in (0, 2, 3):
        alone = attention(qkv[cu[b]:cu[b + 1]], np.array([0, lens[b]]), nh, nkv, HD, 7)
        assert np.array_equal(alone, full[cu[b]:cu[b + 1]]), b
    order = [2, 0, 3, 1]                                    # the same prompts packed in another order
    cu2 = np.concatenate([[0], np.cumsum([lens[b] for b in order])])
    perm = attention(np.concatenate([qkv[cu[b]:cu[b + 1]] for b in order]), cu2, nh, nkv, HD, 7)
    for i, b in enumerate(order):
        assert np.array_equal(perm[cu2[i]:cu2[i + 1]], full[cu[b]:cu[b + 1]]), b


def test_hd96_online_softmax_with_forced_maximum_jumps():
    """test_hd64_online_softmax_with_forced_maximum_jumps (tests/test_gpu_llama3.py) at head_dim 96: keys far into a prompt copy
    the direction of chosen queries at large gains, so some rows' maximum jumps past the deferral threshold at chosen
    (off-diagonal, first, diagonal) blocks; a float64 reference. A spiked score is gain |q|^2 / sqrt(hd) with |q|^2 ~ 0.09 hd,
    i.e. proportional to sqrt(hd): the hd-256 test's gains g at 256 and 2 g at 64 give the same scores, and so does
    sqrt(256 / 96) g here."""
    nh = nkv = 2
    hd = HD
    lens = [700, 333]
    cu = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(3)
    n = int(cu[-1])
    qkv = (rng.standard_normal((n, 3 * nh * hd)) * 0.3).astype(np.float32)
    q = qkv[:, : nh * hd].reshape(n, nh, hd)
    k = qkv[:, nh * hd: 2 * nh * hd].reshape(n, nh, hd)
    spikes = [(200, [450, 460, 699], 9.0), (330, [600, 601], 25.0), (70, [500], 3.0), (5, [40, 300], 12.0),
              (640, [650, 690], 14.0), (700 + 100, [700 + 250, 700 + 332], 20.0)]
    for key, qs, gain in spikes:
        for h in range(nh):
            k[key, h] = np.sqrt(256.0 / hd) * gain * np.mean([q[j, h] for j in qs], axis=0)
    qkv = bf16_round(qkv)
    got = attention(qkv, cu, nh, nkv, hd, 7)
    qq = qkv[:, : nh * hd].reshape(n, nh, hd).astype(np.float64)
    kk = qkv[:, nh * hd: 2 * nh * hd].reshape(n, nh, hd).astype(np.float64)
    vv = qkv[:, 2 * nh * hd:].reshape(n, nh, hd).astype(np.float64)
    ref = np.zeros((n, nh * hd))
    jumps = 0
    for b in range(len(lens)):
        s, e = cu[b], cu[b + 1]
        T = e - s
        mask = np.tril(np.ones((T, T), bool))
        for h in range(nh):
            sc = np.where(mask, (qq[s:e, h] @ kk[s:e, h].T) / np.sqrt(hd), -np.inf)
            for blk in range(1, (T + 63) // 64):   # a later block's maximum past everything before it by > 2^8
                before = sc[:, : blk * 64].max(-1)
                here = sc[:, blk * 64: (blk + 1) * 64].max(-1)
                jumps += int((((here - before) * 1.4426950408889634) > 8.0).sum())
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[s:e, h * hd:(h + 1) * hd] = (p @ vv[s:e, h]) / p.sum(-1, keepdims=True)
    print(f"hd96 forced jumps: {jumps} rows, max err {np.abs(got - ref).max():.5f}, max |ref| {np.abs(ref).max():.3f}")
    assert jumps > 10
    assert np.isfinite(got).all()
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() < 2.0e-2 * max(1.0, scale), (np.abs(got - ref).max(), scale)


# ---- shared prefix and last row --------------------------------------------------------------------------------------
TAILS = [1, 4, 70, 130, 61]
SHAPES96 = [(4, 2), (8, 1), (2, 2)]


@pytest.mark.parametrize("nh,nkv", SHAPES96)
def test_hd96_prefix_kernel_is_bit_identical_to_the_whole_prompt_kernel(nh, nkv):
    for P in (36, 63, 64, 65, 129):
        qkv, cu = _whole_prompts("flat", P, TAILS, nh, nkv, HD)
        full = _full(_bits(qkv), cu, nh, nkv, HD, 7)
        ref, _, bound, _ = R.attention_ref64(qkv, cu, nh, nkv, HD)
        rows, seg, src = _prefix_layout(qkv, cu, P)
        for v in (7, 0):
            rc, got = _prefix_call(_bits(rows), seg, P, nh, nkv, HD, v)
            assert rc == 0, (P, v, _lib()[0].lr_last_error())
            n = int(seg[-1])
            assert (got[n:].view(np.uint16) == POISON).all(), (P, v, "guard rows written")
            diff = np.flatnonzero((got[:n] != full[src]).any(axis=1))
            assert diff.size == 0, (P, v, "rows differ from variant 7", diff[:8], np.searchsorted(seg, diff[:8], "right") - 1)
            r = R.ratio(bf16_bits_to_f32(got[:n].view(np.uint16)), ref[src], bound[src])
            assert r <= 1.0, (P, v, r)


LAST_T = [1, 2, 63, 64, 65, 128, 129, 200]


@pytest.mark.parametrize("P", [0, 36, 64, 129])
@pytest.mark.parametrize("nh,nkv", SHAPES96)
def test_hd96_last_row_kernel_equals_row_T_minus_1_of_the_whole_prompt_kernel(nh, nkv, P):
    L, st = _lib()
    qkv, cu = _whole_prompts("flat", P, LAST_T, nh, nkv, HD)
    full = _full(_bits(qkv), cu, nh, nkv, HD, 7)
    rows, seg, _ = _prefix_layout(qkv, cu, P)
    B = len(LAST_T)
    kv = np.ascontiguousarray(rows[:, nh * HD:])
    q_last = np.ascontiguousarray(qkv[cu[1:] - 1, :nh * HD])
    kv_d, q_d, segd = _bits(kv), _bits(q_last), torch.from_numpy(seg).cuda()
    for v in (7, 0):
        out = torch.full((B + GUARD, nh * HD), POISON, dtype=torch.int16, device="cuda")
        rc = L.lr_attention_last_rows(kv_d.data_ptr(), q_d.data_ptr(), out.data_ptr(), segd.data_ptr(), seg.ctypes.data, len(seg) - 1,
                                      P, nh, nkv, HD, v, st)
        torch.cuda.synchronize()
        assert rc == 0, L.lr_last_error()
        got = out.cpu().numpy()
        assert (got[B:].view(np.uint16) == POISON).all(), "rows past the prompts written"
        bad = np.flatnonzero((got[:B] != full[cu[1:] - 1]).any(axis=1))
        assert bad.size == 0, (v, "prompts whose last row differs", bad, [LAST_T[i] for i in bad])


def test_hd96_refusals_leave_outputs_untouched():
    L, st = _lib()
    nh, nkv = 4, 2

    def whole(hd, variant, want, api="plain", cap=0.0):
        cu = np.array([0, 10, 90], np.int32)
        cud = torch.from_numpy(cu).cuda()
        qkv = torch.zeros((90, (nh + 2 * nkv) * hd), dtype=torch.int16, device="cuda")
        out = torch.full((90, nh * hd), 0x1234, dtype=torch.int16, device="cuda")
        lse = torch.full((90, nh), 7.0, dtype=torch.float32, device="cuda")
        if api == "plain":
            rc = L.lr_attention_varlen(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, 2, nh, nkv, hd, variant, st)
        elif api == "lse":
            rc = L.lr_attention_varlen_lse(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu.ctypes.data, 2, nh,
                                           nkv, hd, variant, st)
        elif api == "ws":
            rc = L.lr_attention_varlen_ws(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu.ctypes.data, 2, nh,
                                          nkv, hd, variant, None, 0, st)
        else:
            rc = L.lr_attention_varlen_softcap(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, 2, 0, nh, nkv, hd,
                                               float(hd) ** -0.5, cap, variant, st)
        torch.cuda.synchronize()
        assert rc == want, (hd, variant, api, rc, L.lr_last_error())
        assert (out.cpu().numpy() == 0x1234).all() and (lse.cpu().numpy() == 7.0).all(), (hd, variant, api)
        return L.lr_last_error()

    for hd in (64, 128, 256):
        assert b"head_dim 96" in whole(hd, 7, LR_EUNSUPPORTED)          # variant 7 off head_dim 96
    for v in (2, 4, 5):
        whole(HD, v, LR_EUNSUPPORTED)                                    # the other MFMA kernels at head_dim 96
    assert b"lse" in whole(HD, 7, LR_EINVAL, "lse")                      # variant 7 writes no statistics
    assert b"lse" in whole(HD, 7, LR_EINVAL, "ws")
    assert b"soft" in whole(HD, 7, LR_EUNSUPPORTED, "cap", 50.0)         # and has no capped form

    def both(seg, P, hd, variant, want):
        seg = np.asarray(seg, dtype=np.int32)
        n = max(int(seg.max()), 1)
        rows = torch.zeros((n, (nh + 2 * nkv) * hd), dtype=torch.int16, device="cuda")
        rc, out = _prefix_call(rows, seg, P, nh, nkv, hd, variant, fill=0x1234)
        assert rc == want, (seg, P, hd, variant, rc, L.lr_last_error())
        assert (out == 0x1234).all()
        S = len(seg) - 1
        q = torch.zeros((S, nh * hd), dtype=torch.int16, device="cuda")
        o = torch.full((S, nh * hd), 0x1234, dtype=torch.int16, device="cuda")
        segd = torch.from_numpy(seg).cuda()
        rc = L.lr_attention_last_rows(rows.data_ptr(), q.data_ptr(), o.data_ptr(), segd.data_ptr(), seg.ctypes.data, S, P, nh, nkv,
                                      hd, variant, st)
        torch.cuda.synchronize()
        assert rc == want, (seg, P, hd, variant, rc, L.lr_last_error())
        assert (o.cpu().numpy() == 0x1234).all()

    for v in (7, 0):                                     # the malformed segment lists of tests/test_gpu_attn_prefix.py
        both([0, 35, 70, 90], 36, HD, v, LR_EINVAL)        # segment 0 != prefix_len
        both([0, 37, 70, 90], 36, HD, v, LR_EINVAL)
        both([0, 36, 36, 90], 36, HD, v, LR_EINVAL)        # an empty segment
        both([0, 36, 90, 80], 36, HD, v, LR_EINVAL)        # decreasing starts
        both([1, 37, 90], 36, HD, v, LR_EINVAL)            # starts[0] != 0
        both([0, 36], 36, HD, v, LR_EINVAL)                # a prefix and no prompt
        both([0, 36, 90], -1, HD, v, LR_EINVAL)
    both([0, 36, 90], 36, HD, 1, LR_EUNSUPPORTED)          # the generic kernel reads no prefix
    for hd in (64, 128, 256):
        both([0, 36, 90], 36, hd, 7, LR_EUNSUPPORTED)
    for v in (2, 4, 5):
        both([0, 36, 90], 36, HD, v, LR_EUNSUPPORTED)


# ---- the 256-tile GEMM's rotary epilogue at Phi-3-mini's qkv width ----------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_qkv_epilogue_store_and_rope_at_hd96(kind):
    """N = 9216 = 96 heads' worth of columns in 36 tiles of 256: a head straddles a tile edge in two tiles of three. rot_cols
    = 6144 (q | k). The fast GEMM (variant 4) is bit-identical to the generic one (1) and within stage2_ref's bound."""
    N, rot_cols, T, K = 9216, 6144, 2048, 256
    cs = _rope_table(T, HD)
    cs_h = cs[: T * HD].view(T, HD // 2, 2).cpu().numpy()
    cos, sin = cs_h[..., 0], cs_h[..., 1]
    bad = []
    for M in (1, 7, 255, 257, 517):
        A, B, acc = _operands(kind, M, N, K, M + N)
        A_d, B_d = _dev_bf16(A), _dev_bf16(B)
        pos = ((np.arange(M) * 2654435761) % T).astype(np.int32)
        pos[0] = T - 1
        pos_d = torch.from_numpy(pos).cuda()
        outs = {}
        for variant in (1, 4):
            tag = f"phi3-mini {kind} M={M} v{variant}"
            got_s = _epi(A_d, B_d, M, N, K, 0, variant)
            got_r = _epi(A_d, B_d, M, N, K, 3, variant, pos_d=pos_d, cs=cs, rope_positions=T, hd=HD, rot_cols=rot_cols)
            outs[variant] = (got_s, got_r)
            want_s, want_r = R.epi_store(acc), R.epi_rope(acc, pos, cos, sin, HD, rot_cols)
            if kind == "exact":
                if not np.array_equal(got_s, want_s):
                    bad.append(("store", tag, _report(f"store {tag}", got_s, want_s, None)))
                if not np.array_equal(got_r, want_r):
                    bad.append(("rope", tag, _report(f"rope {tag}", got_r, want_r, None)))
                if variant == 1 and M == 517:
                    for m in R.ROPE_MUTANTS:
                        assert (R.epi_rope(acc, pos, cos, sin, HD, rot_cols, m) != got_r).mean() > 0.1, m
            else:
                absum = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T
                acc_err = K * 2.0 ** -24 * absum
                x_ulp = _bf16_ulp(acc) + acc_err
                if _report(f"store {tag}", got_s, acc, x_ulp) > 1:
                    bad.append(("store", tag))
                pair = 2 * np.maximum(x_ulp, np.maximum(np.roll(x_ulp, -1, axis=1), np.roll(x_ulp, 1, axis=1))) + _bf16_ulp(want_r)
                if _report(f"rope {tag}", got_r, want_r, pair) > 1:
                    bad.append(("rope", tag))
        if kind == "exact":   # exact operands: every partial sum is exact, so the two kernels must agree to the bit
            assert np.array_equal(outs[1][0], outs[4][0]) and np.array_equal(outs[1][1], outs[4][1]), M
    assert not bad, bad[:10]


# ---- the scoring path on the reference's goldens ------------------------------------------------------------------------
@pytest.mark.parametrize("name", PHI3_GOLDENS)
@pytest.mark.parametrize("variants", [(0, 0), (1, 1), (4, 7), (5, 0)])
def test_phi3_prefill_vs_reference_goldens(golden_dir, name, variants):
    from llamarec_amd.llm import LlamaRanker
    from tests.gen_goldens_phi3 import golden_tolerance

    z, cfg, sd, seqs = load_phi3_golden(golden_dir, name)
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    model = LlamaRanker.from_state_dict(sd, cfg)
    assert model.family == "phi3" and model.hd == cfg["hidden_size"] // cfg["num_attention_heads"]
    if variants == (4, 7):
        # The forced pair runs as given on hd96_mha alone. GEMM variant 4 refuses a shape off its 256 x 256 x 64 tile (hd96_gqa's
        # hidden 384, hd16's 64) and attention variant 7 a head_dim other than 96: both refusals are asserted here, and the
        # archive is then scored with whatever of the pair its shapes admit (auto GEMMs; the generic attention at hd16).
        d, f, qkv_w = cfg["hidden_size"], cfg["intermediate_size"], (cfg["num_attention_heads"] + 2 * cfg["num_key_value_heads"]) * model.hd
        fits = all(n % 256 == 0 for n in (d, 2 * f, qkv_w)) and all(k % 64 == 0 for k in (d, f))
        assert fits == (name == "hd96_mha")
        if not fits or model.hd != HD:
            from llamarec_amd._lib import LlamaRecError

            with pytest.raises(LlamaRecError, match="gemm variant 4|head_dim 96"):
                model.set_variants(4, 7 if model.hd == HD else 1).last_logits(seqs)
            torch.cuda.synchronize()
            variants = (4 if fits else 0, 7 if model.hd == HD else 1)
    model.set_variants(*variants)
    got = model.last_logits(seqs).cpu().numpy()
    assert got.shape == z["logits_bf16"].shape and np.array_equal(got, bf16_round(got))
    print(f"{name} {variants}: vs bf16 {np.abs(got - z['logits_bf16']).max():.4f}, vs fp32 {np.abs(got - z['logits_fp32']).max():.4f}, "
          f"tolerance {tol:.4f}")
    assert np.abs(got - z["logits_fp32"]).max() < tol
    assert np.abs(got - z["logits_bf16"]).max() < tol
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])


@pytest.mark.parametrize("name", PHI3_GOLDENS)
def test_phi3_last_layer_pruning_matches_full_last_layer(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker
    from tests.gen_goldens_phi3 import golden_tolerance

    z, cfg, sd, seqs = load_phi3_golden(golden_dir, name)
    tol = golden_tolerance(z["logits_fp32"], z["logits_bf16"])
    model = LlamaRanker.from_state_dict(sd, cfg)
    pruned = model.last_logits(seqs).cpu().numpy()
    full = model.set_last_layer_pruning(False).last_logits(seqs).cpu().numpy()
    assert np.abs(pruned - full).max() < tol
    assert np.abs(full - z["logits_bf16"]).max() < tol


MODEL_TAILS = [1, 7, 40, 90]
LABELS = list(range(40, 60))


@pytest.mark.parametrize("name", ["hd96_mha", "hd96_gqa"])
def test_phi3_shared_prefix_is_bit_identical_and_executed(golden_dir, name):
    """Shared-prefix scores equal share_prefix=False to the bit, and the profile of one shared call shows the prefix and
    last-row launches: the first layer's qkv product runs on n - (B - 1) P rows, the pruned last layer runs a K | V product
    over all rows and a Q product over the B last rows (tests/test_gpu_attn_prefix.py)."""
    from llamarec_amd.llm import LlamaRanker

    L, _ = _lib()
    z, cfg, sd, _ = load_phi3_golden(golden_dir, name)
    cfg = dict(cfg, sliding_window=None)                       # prompts of up to 130 + 90 tokens, past the archives' window of 192
    assert cfg["max_position_embeddings"] >= 130 + 90
    model = LlamaRanker.from_state_dict(sd, cfg)
    for P in (36, 64, 130):
        seqs = _prefixed_prompts(P, MODEL_TAILS, cfg["vocab_size"], P)
        for prune in (True, False):
            for v in (0, 7):
                model.set_variants(0, v).set_last_layer_pruning(prune)
                shared = model.prefill_verbalize(seqs, LABELS, share_prefix=True)
                plain = model.prefill_verbalize(seqs, LABELS, share_prefix=False)
                assert torch.isfinite(plain).all() and torch.equal(shared, plain), (P, prune, v)
    P, B = 36, len(MODEL_TAILS)
    seqs = _prefixed_prompts(P, MODEL_TAILS, cfg["vocab_size"], 7)
    n_in = sum(len(s) for s in seqs)
    n = n_in - (B - 1) * P
    d, nh, nkv = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    q_w, kv_w = nh * HD, 2 * nkv * HD
    model.set_variants(0, 0).set_last_layer_pruning(True)
    model.prefill_verbalize(seqs, LABELS, share_prefix=True)   # warm (workspace allocation outside the profiled call)
    assert L.lr_profile_start(4096) == 0
    model.prefill_verbalize(seqs, LABELS, share_prefix=True)
    torch.cuda.synchronize()
    assert L.lr_profile_stop() == 0
    recs = _gemm_rows(L)
    rope = sorted((N, rows) for epi, N, K, rows in recs if epi == 3 and K == d)   # the qkv products (rotary epilogue)
    want = sorted([(q_w + kv_w, n)] * (cfg["num_hidden_layers"] - 1) + [(kv_w, n), (q_w, B)])
    assert rope == want, (rope, want, n_in)
    assert L.lr_profile_records(2, None, None, None, 0) == cfg["num_hidden_layers"]   # MFMA attention launches, one per layer
    assert L.lr_profile_records(3, None, None, None, 0) <= 0                          # and no generic one


def test_full_width_phi3_mini_fast_vs_generic_and_restatement():
    """Phi-3-mini layer shapes (32 x 96 heads on 3072, d_ff 8192, untied head), 2 layers, random weights, long prompts: the
    fast path (256-tile GEMMs with the hd-96 RoPE epilogue, attention variant 7, pruned last layer) against the generic
    kernels (1, 1), and both against the fp32 torch restatement on the GPU. Bounds as
    test_full_width_llama32_fast_vs_generic_and_restatement derives them: the generic path's distance to the restatement is
    measured in the run (and held to 1e-1 x scale); the fast path is allowed that plus the fast-vs-generic gap of 5e-2 x scale."""
    from llamarec_amd.llm import PHI3_MINI, LlamaRanker
    from tests import phi3_ref as PR

    cfg = dict(PHI3_MINI, num_hidden_layers=2)
    sd = PR.random_phi3_state(cfg, seed=7, device="cuda")
    model = LlamaRanker.from_state_dict(sd, cfg)
    assert model.hd == 96 and model.family == "phi3"
    rng = np.random.default_rng(2)
    lens = [460, 1125, 700, 5]
    seqs = [np.concatenate([[1], rng.integers(3, cfg["vocab_size"], size=n - 1)]).astype(np.int32) for n in lens]
    label_ids = list(range(100, 120))
    fast = model.prefill_verbalize(seqs, label_ids).cpu().numpy()
    gen = model.set_variants(1, 1).prefill_verbalize(seqs, label_ids).cpu().numpy()
    forced = model.set_variants(0, 7).prefill_verbalize(seqs, label_ids).cpu().numpy()
    model.set_variants(0, 0)
    ref = PR.last_logits(sd, cfg, seqs, torch.float32, device="cuda")[:, label_ids]
    scale = max(1.0, float(np.abs(ref).max()))
    gen_err = float(np.abs(gen - ref).max())
    print(f"phi-3-mini: max |ref| {np.abs(ref).max():.3f}, fast-ref {np.abs(fast - ref).max():.4f}, gen-ref {gen_err:.4f}, "
          f"fast-gen {np.abs(fast - gen).max():.4f}")
    assert np.isfinite(fast).all() and float(np.abs(fast).max()) > 0.05
    assert np.array_equal(forced, fast)                       # the prefill's auto is variant 7 at head_dim 96
    assert gen_err <= 1e-1 * scale
    assert np.abs(fast - gen).max() <= 5e-2 * scale
    assert np.abs(fast - ref).max() <= gen_err + 5e-2 * scale
    alone = model.prefill_verbalize([seqs[1]], label_ids).cpu().numpy()   # a prompt's scores do not depend on the batch
    assert np.array_equal(alone[0], fast[1])


@pytest.mark.parametrize("load_in_4bit", [False, True])
def test_phi3_from_pretrained_reads_fused_names(golden_dir, tmp_path, load_in_4bit):
    """A local checkpoint directory with Phi-3's fused tensor names scores like from_state_dict, also behind the NF4 round
    trip (which acts on the fused Linears as stored)."""
    from safetensors.torch import save_file

    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_phi3_golden(golden_dir, "hd96_gqa")
    hf = str(tmp_path / "phi3")
    os.makedirs(hf)
    assert "model.layers.0.self_attn.qkv_proj.weight" in sd and "model.layers.0.self_attn.q_proj.weight" not in sd
    json.dump(dict(cfg, architectures=["Phi3ForCausalLM"], torch_dtype="bfloat16"), open(os.path.join(hf, "config.json"), "w"))
    save_file({n: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for n, v in sd.items()},
              os.path.join(hf, "model.safetensors"), metadata={"format": "pt"})
    loaded = LlamaRanker.from_pretrained(hf, load_in_4bit=load_in_4bit)
    assert loaded.hd == 96 and loaded.family == "phi3" and loaded.max_prompt_len == cfg["sliding_window"]
    label_ids = list(z["label_ids"])
    got = loaded.prefill_verbalize(seqs, label_ids)
    want = LlamaRanker.from_state_dict(sd, cfg, nf4=load_in_4bit).prefill_verbalize(seqs, label_ids)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    if load_in_4bit:   # the round trip moved the weights: not the unquantised scores
        assert not torch.equal(got, LlamaRanker.from_state_dict(sd, cfg).prefill_verbalize(seqs, label_ids))


def test_train_ranker_synthetic_phi3_eval_only(tmp_path):
    """`train_ranker.py --synthetic --llm phi3 --eval_only` with default flags (NF4 on) scores the retrieved users through a
    tiny Phi-3 ranker (fused names, head_dim 96) and writes the reference's metric files; training a Phi-3 base is refused."""
    import pickle

    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    r = pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))
    assert r["test_users"], "the synthetic retriever retrieved nobody"
    out = str(tmp_path / "experiments" / "phi3" / "synthetic")
    metrics, overall = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "phi3", "--eval_only",
                                          "--llm_retrieved_path", lru_root, "--export_root", out, "--llm_max_history", "5"])
    assert "test_NDCG@10" in metrics and 0.0 <= metrics["test_NDCG@10"] <= 1.0
    assert os.path.exists(os.path.join(out, "subset_metrics.json")) and os.path.exists(os.path.join(out, "overall_metrics.json"))
    with pytest.raises(SystemExit, match="eval_only"):
        train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "phi3", "--llm_retrieved_path", lru_root,
                           "--export_root", out])
