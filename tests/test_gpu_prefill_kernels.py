"""GPU: the kernels every scored prompt passes through between the GEMMs and the attention passes (csrc/llama_elem.hip) and the
folded-RMSNorm arm of the GEMM epilogues, one at a time through their stand-alone entry points, against the float64 references
of tests/prefill_kernels_ref.py, element by element within the bounds derived there. The shapes are that module's lists: the
smallest at which each code path changes. Outputs start NaN-poisoned, guard rows behind every output must keep their bits,
exact kinds must come back bit for bit, every bound test prints max(err / bound) and shows on the kernel's own output that the
reference's mutants (one plausible kernel bug each) exceed the bound."""
import ctypes

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, f32_to_bf16_bits
from tests import prefill_kernels_ref as P
from tests import stage2_ref as R

pytestmark = pytest.mark.gpu

POISON = 0x7FC0          # a bf16 NaN
GUARD32 = 12345.5        # fp32 guard value
LR_EINVAL, LR_EUNSUPPORTED = -1, -2
EPS_N = P.NORM_EPS


def _L():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def _ok(rc):
    from llamarec_amd._lib import lib

    assert rc == 0, (rc, lib().lr_last_error())


def _dev(x):
    """bf16 device copy of a bf16-valued array"""
    return torch.from_numpy(f32_to_bf16_bits(np.ascontiguousarray(x, dtype=np.float32)).view(np.int16)).cuda()


def _poisoned(rows, cols, guard_rows=1):
    return torch.full((rows + guard_rows, cols), POISON, dtype=torch.int16, device="cuda")


def _take(t, rows):
    """(values of the first rows, guard rows untouched)"""
    b = t.cpu().numpy().view(np.uint16)
    return bf16_bits_to_f32(b[:rows]), bool((b[rows:] == POISON).all())


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def outside(got, ref, bound):
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound)).any())


# ---- RMSNorm, both styles ----------------------------------------------------------------------------------------------------
def test_rmsnorm_both_styles_within_bound_two_pass_branch_included():
    l, st = _L()
    worst, bad = {}, []
    seen = {(s, m): False for s in (0, 1) for m in P.MUTANTS["norm"] if not (s == 1 and m == "inner_rounding_missing")}
    for style in (0, 1):
        for d in P.ROW_DS + (P.TWO_PASS_D,):
            for rows in P.ROW_ROWS:
                x, w = P.norm_data(rows, d)
                out, xd, wd = _poisoned(rows, d), _dev(x), _dev(w)
                _ok(l.lr_rmsnorm_bf16(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), rows, d, EPS_N, style, st))
                torch.cuda.synchronize()
                got, kept = _take(out, rows)
                assert kept, ("guard row written", style, d, rows)
                ref, bound = P.rmsnorm_ref64(x, w, EPS_N, style)
                r = P.ratio(got, ref, bound)
                worst[(style, d)] = max(worst.get((style, d), 0.0), r)
                if not r <= 1.0:
                    bad.append((style, d, rows, r))
                for key in seen:
                    if key[0] == style:
                        seen[key] |= outside(got, P.rmsnorm_ref64(x, w, EPS_N, style, mutant=key[1])[0], bound)
    for (style, d), r in sorted(worst.items()):
        print(f"rmsnorm style {style} d={d}: max err/bound {r:.3f}")
    assert not bad, bad
    assert all(seen.values()), [k for k, v in seen.items() if not v]


def test_rms_rstd_within_bound():
    l, st = _L()
    bad = []
    for d in P.ROW_DS:
        x5, _ = P.norm_data(5, d)
        for rows in P.RSTD_ROWS:
            x = x5[:rows] if rows != 4 else x5[1:5]
            out = torch.full((rows + 8,), GUARD32, dtype=torch.float32, device="cuda")
            out[:rows] = float("nan")
            xd = _dev(x)
            _ok(l.lr_rms_rstd_f32(xd.data_ptr(), out.data_ptr(), rows, d, EPS_N, st))
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            assert (o[rows:] == np.float32(GUARD32)).all(), ("guard floats written", d, rows)
            ref, bound = P.rstd_ref64(x, EPS_N)
            r = P.ratio(o[:rows, None], ref, bound)
            print(f"rms_rstd d={d} rows={rows}: err/bound {r:.3f}")
            if not r <= 1.0:
                bad.append((d, rows, r))
            if rows >= 4:
                for m in ("eps_missing", "mean_over_chunks", "second_piece_dropped"):
                    if m != "second_piece_dropped" or d > 2048:
                        assert outside(o[:rows, None], P.rstd_ref64(x, EPS_N, mutant=m)[0], bound), (m, d)
    assert not bad, bad


# ---- split-K reduce + residual + norm ----------------------------------------------------------------------------------------
def _residual_rmsnorm(l, st, A_, B_, Rr, w, style, ws):
    """In place (C aliasing R). Returns (C, xn, was_fused)."""
    M, K = A_.shape
    N = B_.shape[0]
    c = torch.full((M + 1, N), POISON, dtype=torch.int16, device="cuda")
    c[:M] = _dev(Rr)
    xn = _poisoned(M, N)
    fused = ctypes.c_int32(-1)
    A_d, B_d, w_d = _dev(A_), _dev(B_), _dev(w)
    _ok(l.lr_gemm_bf16_nt_residual_rmsnorm_ex(A_d.data_ptr(), B_d.data_ptr(), c.data_ptr(), c.data_ptr(), M, N, K, 5,
                                              w_d.data_ptr(), xn.data_ptr(), EPS_N, style, 1, ctypes.byref(fused),
                                              ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    C, kept_c = _take(c, M)
    X, kept_x = _take(xn, M)
    assert kept_c and kept_x, ("guard row written", M, N)
    return C, X, fused.value


def _check_residual_rmsnorm(tag, A_, B_, Rr, w, style, C, X, bad, seen=None):
    p64, absum = P.split_planes64(A_, B_, 2)
    ref, bound = P.reduce_ref64(p64, Rr, extra=A_.shape[1] * P.EPS * absum)
    r_c = P.ratio(C, ref, bound)
    nref, nb = P.rmsnorm_ref64(C, w, EPS_N, style)          # the norm of the kernel's own C
    r_x = P.ratio(X, nref, nb)
    print(f"{tag}: C err/bound {r_c:.3f}, xn err/bound {r_x:.3f}")
    if not (r_c <= 1.0 and r_x <= 1.0):
        bad.append((tag, r_c, r_x))
    if seen is not None:
        for m in P.MUTANTS["reduce"]:
            seen[m] |= outside(C, P.reduce_ref64(p64, Rr, extra=A_.shape[1] * P.EPS * absum, mutant=m)[0], bound)
        for m in ("mean_over_chunks", "style_swapped", "weight_of_next_chunk"):
            seen[m] |= outside(X, P.rmsnorm_ref64(C, w, EPS_N, style, mutant=m)[0], nb)


def test_fused_reduce_residual_rmsnorm_within_bound_in_place():
    l, st = _L()
    ws = torch.empty(32 << 20, dtype=torch.uint8, device="cuda")
    bad = []
    seen = dict.fromkeys(P.MUTANTS["reduce"] + ("mean_over_chunks", "style_swapped", "weight_of_next_chunk"), False)
    for N in P.REDUCE_NS:
        for M in P.REDUCE_MS:
            A_, B_, Rr, w = P.reduce_data(M, N)
            for style in (0, 1):
                C, X, fused = _residual_rmsnorm(l, st, A_, B_, Rr, w, style, ws)
                assert fused == 1, (M, N, fused)
                _check_residual_rmsnorm(f"fused reduce N={N} M={M} style {style}", A_, B_, Rr, w, style, C, X, bad, seen)
    assert not bad, bad
    assert all(seen.values()), seen


def test_unfused_past_the_keep_limit_reports_it_and_stays_within_bound():
    l, st = _L()
    ws = torch.empty(32 << 20, dtype=torch.uint8, device="cuda")
    bad = []
    A_, B_, Rr, w = P.reduce_data(7, P.UNFUSED_N)
    for style in (0, 1):
        C, X, fused = _residual_rmsnorm(l, st, A_, B_, Rr, w, style, ws)
        assert fused == 0, fused
        _check_residual_rmsnorm(f"two launches N={P.UNFUSED_N} M=7 style {style}", A_, B_, Rr, w, style, C, X, bad)
    assert not bad, bad


# ---- sandwich norm -----------------------------------------------------------------------------------------------------------
def test_sandwich_norm_within_bound_with_and_without_next_and_aliased():
    l, st = _L()
    worst, bad, seen = [0.0, 0.0], [], False
    for d in P.ROW_DS:
        for rows in P.ROW_ROWS:
            h, w_out = P.norm_data(rows, d)
            x, w_next = P.norm_data(rows, d, seed=1)
            x[rows - 1] = bf16_round(x[rows - 1] * np.float32(0.01))
            ref, bound = P.sandwich_ref64(x, h, w_out, EPS_N)
            wo_d, wn_d = _dev(w_out), _dev(w_next)
            for mode in ("no_next", "next", "aliased"):
                xd = _poisoned(rows, d)
                xd[:rows] = _dev(x)
                hd_ = _poisoned(rows, d)
                hd_[:rows] = _dev(h)
                xn = hd_ if mode == "aliased" else _poisoned(rows, d)
                nxt = mode != "no_next"
                _ok(l.lr_residual_postnorm_bf16(xd.data_ptr(), hd_.data_ptr(), wo_d.data_ptr(),
                                                wn_d.data_ptr() if nxt else None, xn.data_ptr() if nxt else None, rows, d,
                                                EPS_N, st))
                torch.cuda.synchronize()
                xp, kept = _take(xd, rows)
                assert kept, ("guard row written", d, rows, mode)
                r = P.ratio(xp, ref, bound)
                worst[0] = max(worst[0], r)
                if not r <= 1.0:
                    bad.append(("x'", d, rows, mode, r))
                seen |= outside(xp, P.sandwich_ref64(x, h, w_out, EPS_N, mutant="norm_after_add")[0], bound)
                got, kept = _take(xn, rows)
                assert kept, ("guard row written", d, rows, mode)
                if nxt:
                    nref, nb = P.rmsnorm_ref64(xp, w_next, EPS_N, 1)      # the norm of the kernel's own x'
                    r = P.ratio(got, nref, nb)
                    worst[1] = max(worst[1], r)
                    if not r <= 1.0:
                        bad.append(("xn", d, rows, mode, r))
                else:
                    assert np.isnan(got).all(), "xn written without w_next"
    print(f"sandwich norm: x' max err/bound {worst[0]:.3f}, xn max err/bound {worst[1]:.3f}")
    assert not bad, bad
    assert seen


# ---- head --------------------------------------------------------------------------------------------------------------------
NAN_FILL = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]     # a NaN the kernel does not write


def _head(l, st, x, rows, nw, W, ids, c, poison=None, fill=NAN_FILL):
    B, C = c["B"], c["C"]
    out = torch.full((B * C + 8,), GUARD32, dtype=torch.float32, device="cuda")
    out[:B * C] = torch.from_numpy(np.full(B * C, fill, np.float32)).cuda()
    xd, nd, Wd = _dev(x), _dev(nw), _dev(W)
    rd, idd = (_i32(rows) if rows is not None else None), (_i32(ids) if ids is not None else None)
    rc = l.lr_llama_head_bf16(xd.data_ptr(), rd.data_ptr() if rd is not None else None, nd.data_ptr(),
                              Wd.data_ptr(), idd.data_ptr() if idd is not None else None, B, C, c["d"], EPS_N,
                              out.data_ptr(), P.HEAD_VOCAB, poison.data_ptr() if poison is not None else None, c["style"], c["cap"],
                              st)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[B * C:] == np.float32(GUARD32)).all(), ("guard floats written", c)
    return rc, o[:B * C].reshape(B, C)


def test_head_within_bound_nan_exactly_where_ids_leave_the_vocabulary():
    l, st = _L()
    worst, bad = {}, []
    seen = dict.fromkeys(P.MUTANTS["head"], False)
    for c in P.head_cases():
        x, rows, nw, W, ids = P.head_data(c)
        rc, got = _head(l, st, x, rows, nw, W, ids, c)
        _ok(rc)
        ref, bound, nan = P.head_ref64(x, rows, nw, W, ids, c["B"], c["C"], EPS_N, c["style"], c["cap"])
        written = got.view(np.uint32) != np.array([NAN_FILL]).view(np.uint32)[0]
        assert written.all(), ("scores not written", c)
        assert np.array_equal(np.isnan(got), nan), ("NaN somewhere else than at the ids outside the vocabulary", c)
        r = P.ratio(np.where(nan, 0.0, got), ref, bound)
        key = (c["d"], "cap" if c["cap"] > 0 else f"style {c['style']}")
        worst[key] = max(worst.get(key, 0.0), r)
        if not r <= 1.0:
            bad.append((c, r))
        for m in seen:
            mref, _, mnan = P.head_ref64(x, rows, nw, W, ids, c["B"], c["C"], EPS_N, c["style"], c["cap"], mutant=m)
            seen[m] |= bool((mnan != nan).any()) or outside(np.where(nan, 0.0, got), np.where(nan, 0.0, mref), bound)
    for key, r in sorted(worst.items()):
        print(f"head d={key[0]} {key[1]}: max err/bound {r:.3f}")
    assert not bad, bad[:5]
    assert all(seen.values()), seen


def test_head_poison_word_gives_all_nan_and_cap_with_style_0_is_refused():
    l, st = _L()
    c = dict(d=512, B=3, C=33, style=1, perm=True, ids=True, cap=P.HEAD_CAP, seed=3)
    x, rows, nw, W, ids = P.head_data(c)
    for word, want_nan in ((1, True), (0, False)):
        rc, got = _head(l, st, x, rows, nw, W, ids, c, poison=_i32([word]), fill=np.float32(GUARD32))
        _ok(rc)
        _, _, nan = P.head_ref64(x, rows, nw, W, ids, 3, 33, EPS_N, 1, P.HEAD_CAP, poison=word)
        assert nan.all() == want_nan and np.array_equal(np.isnan(got), nan), word
    rc, got = _head(l, st, x, rows, nw, W, ids, dict(c, style=0), fill=np.float32(GUARD32))
    assert rc == LR_EUNSUPPORTED and (got == np.float32(GUARD32)).all()


# ---- bit-exact kernels -------------------------------------------------------------------------------------------------------
def test_embed_is_bit_exact():
    l, st = _L()
    for d in P.EMBED_DS:
        ids, src, table = P.embed_data(d)
        for tok_src in (None, src):
            for scale in (1.0, P.EMBED_SCALE):
                n = len(ids)
                out, idd, td = _poisoned(n, d), _i32(ids), _dev(table)
                sd = _i32(tok_src) if tok_src is not None else None
                _ok(l.lr_llama_embed_bf16(idd.data_ptr(), sd.data_ptr() if sd is not None else None,
                                          td.data_ptr(), P.EMBED_VOCAB, d, out.data_ptr(), n, scale, st))
                torch.cuda.synchronize()
                got, kept = _take(out, n)
                assert kept, ("guard row written", d)
                assert np.array_equal(got, P.embed_ref(ids, tok_src, table, scale)), (d, tok_src is not None, scale)
                if scale != 1.0:
                    assert not np.array_equal(got, P.embed_ref(ids, tok_src, table, scale, mutant="scale_dropped"))
    print("embed: bit-exact")


def test_token_meta_every_array_exact():
    l, st = _L()
    seen = dict.fromkeys(P.MUTANTS["token_meta"], False)
    for c in P.meta_cases():
        Pn, B = c["P"], c["B"]
        ref = P.token_meta_ref(c["cu"], Pn, c["ids"])
        total, S = len(ref["tok_pos"]), len(ref["seg_start"]) - 1
        sizes = dict(seg_start=S + 1, tok_pos=total, tok_src=total, last_rows=B, last_pos=B, prefix_bad=1)
        bufs = {k: torch.full((n + 4,), -77, dtype=torch.int32, device="cuda") for k, n in sizes.items()}
        cud, idd = _i32(c["cu"]), _i32(c["ids"])
        _ok(l.lr_llama_token_meta(cud.data_ptr(), B, Pn, idd.data_ptr(), bufs["seg_start"].data_ptr(),
                                  bufs["tok_pos"].data_ptr(), bufs["tok_src"].data_ptr(), bufs["last_rows"].data_ptr(),
                                  bufs["last_pos"].data_ptr(), bufs["prefix_bad"].data_ptr(), st))
        torch.cuda.synchronize()
        got = {}
        for k, n in sizes.items():
            o = bufs[k].cpu().numpy()
            assert (o[n:] == -77).all(), ("guard words written", k, Pn, B)
            got[k] = o[:n]
            assert np.array_equal(got[k], np.atleast_1d(ref[k])), (k, Pn, B, c["brk"])
        assert int(got["prefix_bad"][0]) == (1 if c["brk"] else 0)
        for m in seen:
            mut = P.token_meta_ref(c["cu"], Pn, c["ids"], mutant=m)
            seen[m] |= any(not np.array_equal(got[k], np.atleast_1d(mut[k])) for k in got)
        # the optional outputs may be absent
        pos2 = torch.full((total + 4,), -77, dtype=torch.int32, device="cuda")
        seg2 = torch.full((S + 5,), -77, dtype=torch.int32, device="cuda")
        _ok(l.lr_llama_token_meta(cud.data_ptr(), B, Pn, None, seg2.data_ptr(), pos2.data_ptr(), None, None, None, None, st))
        torch.cuda.synchronize()
        assert np.array_equal(pos2.cpu().numpy()[:total], ref["tok_pos"]) and np.array_equal(seg2.cpu().numpy()[:S + 1], ref["seg_start"])
    assert all(seen.values()), seen
    print("token meta: every array exact")


def test_gather_rows_and_fold_norm_are_bit_exact():
    l, st = _L()
    for d in P.GATHER_DS:
        x, _ = P.norm_data(5, d)
        rows = np.array([4, 3, 2, 1, 0, 2, 2, 4], np.int32)           # reversed, then repeated
        out, xd, rd = _poisoned(len(rows), d), _dev(x), _i32(rows)
        _ok(l.lr_gather_rows_bf16(xd.data_ptr(), rd.data_ptr(), len(rows), d, out.data_ptr(), st))
        torch.cuda.synchronize()
        got, kept = _take(out, len(rows))
        assert kept and np.array_equal(got, x[rows]), d
    for rows, cols in P.FOLD_SHAPES:
        w = bf16_round(P.hash_uniform(7600 + rows, (rows, cols), 0.05))
        nw = P.norm_data(1, cols, seed=3)[1]
        out, wd, nd = _poisoned(rows, cols), _dev(w), _dev(nw)
        _ok(l.lr_fold_norm_bf16(wd.data_ptr(), nd.data_ptr(), rows, cols, out.data_ptr(), st))
        torch.cuda.synchronize()
        got, kept = _take(out, rows)
        assert kept and np.array_equal(got, P.fold_norm_ref(w, nw)), (rows, cols)
        if cols > 8:
            assert not np.array_equal(got, P.fold_norm_ref(w, np.roll(nw, -8)))     # the weight of the next chunk
    print("gather rows, fold norm: bit-exact")


# ---- row-scaled epilogues ----------------------------------------------------------------------------------------------------
def _rope_table(T, hd):
    l, st = _L()
    cs = torch.full((l.lr_rope_table_bytes(T, hd) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    _ok(l.lr_rope_table(cs.data_ptr(), T, hd, 10000.0, st))
    torch.cuda.synchronize()
    h = cs[: T * hd].view(T, hd // 2, 2).cpu().numpy()
    return cs, h[..., 0].copy(), h[..., 1].copy()


def _rs_gemm(l, st, A_d, B_d, M, N, K, epi, variant, rs_d, ws, pos_d=None, cs=None, rope_positions=0, hd=0, rot_cols=0, plain=False):
    n_out = N // 2 if epi in (2, 5) else N
    C = _poisoned(M, n_out)
    args = (A_d.data_ptr(), B_d.data_ptr(), C.data_ptr(), None, M, N, K, epi, variant, pos_d.data_ptr() if pos_d is not None else None,
            cs.data_ptr() if cs is not None else None, rope_positions, hd, rot_cols, ws.data_ptr() if variant == 5 else None,
            ws.numel() if variant == 5 else 0)
    if plain:
        rc = l.lr_gemm_bf16_nt_epi(*args, st)
    else:
        rc = l.lr_gemm_bf16_nt_rowscale_epi(*args, rs_d.data_ptr() if rs_d is not None else None, st)
    torch.cuda.synchronize()
    got, kept = _take(C, M)
    assert kept, ("guard row written", epi, variant, M)
    return rc, got, C


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_rowscale_epilogues_within_bound_exact_bit_for_bit(kind):
    from tests.test_gpu_stage2_bounds import gated_ratio

    l, st = _L()
    s = P.ROPE_SHAPE
    cs, cos, sin = _rope_table(s["T"], s["hd"])
    ws = torch.empty(16 << 20, dtype=torch.uint8, device="cuda")
    bad, worst = [], {}
    seen = {(e, m): False for e in ("rope", "swiglu") for m in P.MUTANTS["rowscale"]}
    for K in (256, 2048):
        variants = (1, 4) if K == 256 else ((4, 5) if kind == "exact" else (5,))   # exact: variant 4 again beside 5, for the bits
        for M in P.ROWSCALE_MS:
            rs = P.row_scales(kind, M, K, M)
            rs_d = torch.from_numpy(rs).cuda()
            pos = ((np.arange(M) * 2654435761) % s["T"]).astype(np.int32)
            pos[0] = s["T"] - 1
            pos_d = _i32(pos)
            # rope
            A_, B_, acc, absum = P.rowscale_operands(kind, M, s["N"], K, M + s["N"])
            A_d, B_d = _dev(A_), _dev(B_)
            ref, bound = P.rope_rowscale_ref64(acc, absum, K, rs, pos, cos, sin, s["hd"], s["rot_cols"])
            want = R.epi_rope(P.rowscale_value(acc, absum, K, rs)[0], pos, cos, sin, s["hd"], s["rot_cols"])
            for variant in variants:
                for rp in (s["T"], 0):          # the packed-table LDS path and the fp32-table path
                    rc, got, _ = _rs_gemm(l, st, A_d, B_d, M, s["N"], K, 3, variant, rs_d, ws, pos_d, cs, rp, s["hd"], s["rot_cols"])
                    _ok(rc)
                    r = P.ratio(got, ref, bound)
                    worst[("rope", variant)] = max(worst.get(("rope", variant), 0.0), r)
                    if not r <= 1.0 or (kind == "exact" and not np.array_equal(got, want)):
                        bad.append(("rope", kind, variant, M, rp, r))
                    if kind == "random":
                        for m in P.MUTANTS["rowscale"]:
                            seen[("rope", m)] |= outside(got, P.rope_rowscale_ref64(acc, absum, K, rs, pos, cos, sin, s["hd"],
                                                                                   s["rot_cols"], mutant=m)[0], bound)
            # swiglu
            A_, B_, acc, absum = P.rowscale_operands(kind, M, P.SWIGLU_N, K, M + 7)
            A_d, B_d = _dev(A_), _dev(B_)
            v, u = P.rowscale_value(acc, absum, K, rs)
            first = None
            for variant in variants:
                rc, got, _ = _rs_gemm(l, st, A_d, B_d, M, P.SWIGLU_N, K, 2, variant, rs_d, ws)
                _ok(rc)
                r = gated_ratio(2, v, u * 2.0 ** 24, 1, got)
                worst[("swiglu", variant)] = max(worst.get(("swiglu", variant), 0.0), r)
                if not r <= 1.0:
                    bad.append(("swiglu", kind, variant, M, r))
                if kind == "exact":
                    first = got if first is None else first
                    if not np.array_equal(got, first):
                        bad.append(("swiglu bits differ between variants", variants, M))
                else:
                    for m in P.MUTANTS["rowscale"]:
                        vm, um = P.rowscale_value(acc, absum, K, rs, mutant=m)      # the kernel's output judged as the mutant's
                        seen[("swiglu", m)] |= gated_ratio(2, vm, um * 2.0 ** 24, 1, got) > 1.0
    for key, r in sorted(worst.items()):
        print(f"row-scaled {key[0]} {kind} v{key[1]}: max err/bound {r:.3f}")
    assert not bad, bad[:10]
    if kind == "random":
        assert all(seen.values()), seen


def test_null_row_scale_is_the_plain_entry_point_and_other_epilogues_are_refused():
    l, st = _L()
    s = P.ROPE_SHAPE
    cs, _, _ = _rope_table(s["T"], s["hd"])
    ws = torch.empty(16 << 20, dtype=torch.uint8, device="cuda")
    M = 257
    pos_d = _i32((np.arange(M) * 7) % s["T"])
    for variant in P.ROWSCALE_VARIANTS:
        K = P.rowscale_K(variant)
        for epi, N, extra in ((3, s["N"], (pos_d, cs, s["T"], s["hd"], s["rot_cols"])), (2, P.SWIGLU_N, ())):
            A_, B_, _, _ = P.rowscale_operands("random", M, N, K, M + N)
            A_d, B_d = _dev(A_), _dev(B_)
            rc1, a, _ = _rs_gemm(l, st, A_d, B_d, M, N, K, epi, variant, None, ws, *extra)
            rc2, b, _ = _rs_gemm(l, st, A_d, B_d, M, N, K, epi, variant, None, ws, *extra, plain=True)
            _ok(rc1), _ok(rc2)
            assert np.isfinite(a).all() and np.array_equal(a, b), (epi, variant)
    # a row scale with the store, residual or GeGLU epilogue: refused, nothing written
    A_, B_, _, _ = P.rowscale_operands("random", M, 512, 256, 1)
    A_d, B_d, rs_d = _dev(A_), _dev(B_), torch.ones(M, dtype=torch.float32, device="cuda")
    for epi in (0, 1, 5):
        for variant in P.ROWSCALE_VARIANTS:
            n_out = 256 if epi == 5 else 512
            C = _poisoned(M, n_out)
            rc = l.lr_gemm_bf16_nt_rowscale_epi(A_d.data_ptr(), B_d.data_ptr(), C.data_ptr(), C.data_ptr() if epi == 1 else None, M,
                                                512, 256, epi, variant, None, None, 0, 0, 0, ws.data_ptr(), ws.numel(),
                                                rs_d.data_ptr(), st)
            torch.cuda.synchronize()
            assert rc == LR_EINVAL and b"row scale" in l.lr_last_error(), (epi, variant, rc)
            assert bool((C.cpu().numpy().view(np.uint16) == POISON).all()), (epi, variant)
