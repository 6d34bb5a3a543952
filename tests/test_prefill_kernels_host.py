"""CPU: the stand-alone entry points of the prefill's norm, head, embedding and metadata kernels (header, prototypes, every
host-side refusal through the library loaded without a GPU) and tests/prefill_kernels_ref.py itself: on the data the GPU tests
use, every fp32 emulation sits inside its derived bound, every mutant outside on at least one listed case, and exact-kind data
are reproduced bit for bit."""
import os
import re

import numpy as np

from llamarec_amd.synth import bf16_round
from tests import prefill_kernels_ref as P
from tests import stage2_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_EINVAL, LR_EUNSUPPORTED = -1, -2
NEW_SYMBOLS = ("lr_llama_head_bf16", "lr_llama_embed_bf16", "lr_llama_token_meta", "lr_gather_rows_bf16", "lr_rms_rstd_f32",
               "lr_gemm_bf16_nt_rowscale_epi")


def outside(got, ref, bound):
    """some element of got is farther from ref than bound (a NaN on either side counts as outside)"""
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound)).any())


def test_header_prototypes_library_and_integration_table_agree():
    from llamarec_amd import _lib

    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    section = header[header.index("The prefill's norm, head, embedding and metadata kernels alone (exposed for parity tests)"):]
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    l = _lib.lib()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, section, flags=re.S)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert n_args == len(_lib.PROTOTYPES[name][1]), (name, n_args)
        assert hasattr(l, name)
        assert "void* hip_stream" in decl.group(1).split(",")[-1], name   # flat C arguments, the stream last
        assert "`%s`" % name in integration, name


A, B, ODD = 0x10000, 0x20000, 0x10004     # fake device addresses: the refusals come before anything dereferences or launches


def _refused(rc, code, *words):
    from llamarec_amd import _lib

    msg = _lib.lib().lr_last_error()
    assert rc == code, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_every_wrapper_refuses_what_its_kernel_assumes():
    from llamarec_amd import _lib

    l = _lib.lib()
    nan, inf = float("nan"), float("inf")

    def head(x=A, rows=None, nw=A, lm=B, ids=None, Bn=2, C=4, d=64, eps=1e-5, out=A, vocab=10, poison=None, style=0, cap=0.0):
        return l.lr_llama_head_bf16(x, rows, nw, lm, ids, Bn, C, d, eps, out, vocab, poison, style, cap, None)

    _refused(head(x=None), LR_EINVAL, "null")
    _refused(head(out=None), LR_EINVAL, "null")
    _refused(head(Bn=-1), LR_EINVAL, "B -1")
    _refused(head(C=-3), LR_EINVAL, "C -3")
    _refused(head(vocab=0), LR_EINVAL, "vocab 0")
    _refused(head(d=12), LR_EINVAL, "d 12")
    _refused(head(d=0), LR_EINVAL, "d 0")
    _refused(head(eps=-1.0), LR_EINVAL, "eps")
    _refused(head(eps=nan), LR_EINVAL, "eps")
    _refused(head(eps=inf), LR_EINVAL, "eps")
    _refused(head(style=2), LR_EINVAL, "norm_style 2")
    _refused(head(cap=-1.0), LR_EINVAL, "final_softcap")
    _refused(head(cap=nan), LR_EINVAL, "final_softcap")
    _refused(head(cap=30.0, style=0), LR_EUNSUPPORTED, "Gemma norm")
    _refused(head(d=40000), LR_EUNSUPPORTED, "LDS")
    _refused(head(lm=ODD), LR_EUNSUPPORTED, "16-byte aligned")
    assert head(Bn=0) == 0 and head(C=0) == 0     # nothing to do, nothing launched

    def embed(ids=A, src=None, table=B, vocab=10, d=64, out=A, n=4, scale=1.0):
        return l.lr_llama_embed_bf16(ids, src, table, vocab, d, out, n, scale, None)

    _refused(embed(ids=None), LR_EINVAL, "null")
    _refused(embed(table=None), LR_EINVAL, "null")
    _refused(embed(n=-1), LR_EINVAL, "n -1")
    _refused(embed(vocab=0), LR_EINVAL, "vocab 0")
    _refused(embed(d=20), LR_EINVAL, "d 20")
    _refused(embed(scale=inf), LR_EINVAL, "scale")
    _refused(embed(scale=nan), LR_EINVAL, "scale")
    _refused(embed(table=ODD), LR_EUNSUPPORTED, "16-byte aligned")
    _refused(embed(out=ODD), LR_EUNSUPPORTED, "16-byte aligned")
    assert embed(n=0) == 0

    def meta(cu=A, Bn=2, P_=0, ids=None, seg=A, pos=A, src=None, lr=None, lp=None, bad=None):
        return l.lr_llama_token_meta(cu, Bn, P_, ids, seg, pos, src, lr, lp, bad, None)

    _refused(meta(cu=None), LR_EINVAL, "null")
    _refused(meta(seg=None), LR_EINVAL, "null")
    _refused(meta(pos=None), LR_EINVAL, "null")
    _refused(meta(Bn=-1), LR_EINVAL, "B -1")
    _refused(meta(P_=-2), LR_EINVAL, "prefix_len -2")
    _refused(meta(P_=4, bad=A), LR_EINVAL, "without ids")
    assert meta(Bn=0) == 0

    _refused(l.lr_gather_rows_bf16(None, A, 2, 64, B, None), LR_EINVAL, "null")
    _refused(l.lr_gather_rows_bf16(A, None, 2, 64, B, None), LR_EINVAL, "null")
    _refused(l.lr_gather_rows_bf16(A, A, -1, 64, B, None), LR_EINVAL, "n_rows -1")
    _refused(l.lr_gather_rows_bf16(A, A, 2, 60, B, None), LR_EINVAL, "d 60")
    _refused(l.lr_gather_rows_bf16(ODD, A, 2, 64, B, None), LR_EUNSUPPORTED, "16-byte aligned")
    _refused(l.lr_gather_rows_bf16(A, A, 2, 64, ODD, None), LR_EUNSUPPORTED, "16-byte aligned")
    assert l.lr_gather_rows_bf16(A, A, 0, 64, B, None) == 0

    _refused(l.lr_rms_rstd_f32(None, A, 2, 64, 1e-5, None), LR_EINVAL, "null")
    _refused(l.lr_rms_rstd_f32(A, None, 2, 64, 1e-5, None), LR_EINVAL, "null")
    _refused(l.lr_rms_rstd_f32(A, B, -1, 64, 1e-5, None), LR_EINVAL, "rows -1")
    _refused(l.lr_rms_rstd_f32(A, B, 2, 4, 1e-5, None), LR_EINVAL, "d 4")
    _refused(l.lr_rms_rstd_f32(A, B, 2, 64, -1e-5, None), LR_EINVAL, "eps")
    _refused(l.lr_rms_rstd_f32(A, B, 2, 64, nan, None), LR_EINVAL, "eps")
    _refused(l.lr_rms_rstd_f32(ODD, B, 2, 64, 1e-5, None), LR_EUNSUPPORTED, "16-byte aligned")
    assert l.lr_rms_rstd_f32(A, B, 0, 64, 1e-5, None) == 0

    def gemm(a=A, epi=3, rs=A, M=8):
        return l.lr_gemm_bf16_nt_rowscale_epi(a, B, A, None, M, 256, 64, epi, 4, A, A, 0, 128, 256, None, 0, rs, None)

    _refused(gemm(a=None), LR_EINVAL, "null")
    _refused(gemm(epi=4), LR_EINVAL, "epilogue 4")
    for epi in (0, 5):
        _refused(gemm(epi=epi), LR_EINVAL, "row scale")
    assert gemm(M=0) == 0


# ---- norms -------------------------------------------------------------------------------------------------------------------
def test_norm_data_holds_the_rows_that_make_the_mutants_visible():
    for d in P.ROW_DS + (P.TWO_PASS_D,):
        x, w = P.norm_data(5, d)
        assert not x[1].any()
        ms = float((x[2].astype(np.float64) ** 2).mean())
        assert 0.2 * P.NORM_EPS < ms < 5 * P.NORM_EPS, (d, ms)
        assert x[3, d - 1] == 1e4 or x[3, d - 1] == bf16_round(np.array([1e4], np.float32))[0]
        assert np.abs(x[3, :d - 1]).max() < 10
        if d >= 16:
            chunks = w.reshape(-1, 8)
            assert (np.abs(chunks[1:] - chunks[:-1]).max(-1) > 0.05).all(), d    # every chunk differs from its neighbour


def test_norm_emulations_inside_every_mutant_outside():
    seen = {(s, m): False for s in (0, 1) for m in P.MUTANTS["norm"]}
    worst = 0.0
    for style in (0, 1):
        for d in P.ROW_DS + (P.TWO_PASS_D,):
            for rows in P.ROW_ROWS:
                x, w = P.norm_data(rows, d)
                ref, bound = P.rmsnorm_ref64(x, w, P.NORM_EPS, style)
                em = P.rmsnorm_emul32(x, w, P.NORM_EPS, style)
                r = P.ratio(em, ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (style, d, rows, r)
                for m in P.MUTANTS["norm"]:
                    seen[(style, m)] |= outside(em, P.rmsnorm_ref64(x, w, P.NORM_EPS, style, mutant=m)[0], bound)
    print(f"norm emulation: max err/bound {worst:.3f}")
    seen.pop((1, "inner_rounding_missing"))     # style 1 has no inner rounding
    assert all(seen.values()), [k for k, v in seen.items() if not v]
    # the mutants the special rows are there for, each on its own row
    x, w = P.norm_data(5, 4096)
    ref, bound = P.rmsnorm_ref64(x, w, P.NORM_EPS, 0)
    assert outside(ref[2], P.rmsnorm_ref64(x, w, P.NORM_EPS, 0, mutant="eps_missing")[0][2], bound[2])
    assert outside(ref[3], P.rmsnorm_ref64(x, w, P.NORM_EPS, 0, mutant="second_piece_dropped")[0][3], bound[3])


def test_rstd_emulation_inside_its_bound():
    for d in P.ROW_DS:
        for rows in P.RSTD_ROWS:
            x, _ = P.norm_data(5, d)
            x = x[:rows] if rows != 4 else x[1:5]
            ref, bound = P.rstd_ref64(x, P.NORM_EPS)
            assert P.ratio(P.rstd_emul32(x, P.NORM_EPS), ref, bound) <= 1.0, (d, rows)
            for m in ("eps_missing", "mean_over_chunks"):
                if rows >= 4:
                    assert outside(P.rstd_emul32(x, P.NORM_EPS), P.rstd_ref64(x, P.NORM_EPS, mutant=m)[0], bound), (m, d)


# ---- head --------------------------------------------------------------------------------------------------------------------
def test_head_emulations_inside_every_mutant_outside():
    seen = dict.fromkeys(P.MUTANTS["head"], False)
    worst, capped_span = 0.0, [np.inf, 0.0]
    for c in P.head_cases():
        x, rows, nw, W, ids = P.head_data(c)
        args = (x, rows, nw, W, ids, c["B"], c["C"], P.NORM_EPS, c["style"], c["cap"])
        ref, bound, nan = P.head_ref64(*args)
        em = np.where(nan, 0.0, P.head_emul32(*args))
        r = P.ratio(em, ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (c, r)
        assert nan.any() == (ids is not None and c["C"] >= 20)
        assert P.head_ref64(*args, poison=1)[2].all()
        if c["cap"] > 0:
            a = np.abs(ref[~nan])
            capped_span = [min(capped_span[0], a.min()), max(capped_span[1], a.max())]
            if c["C"] >= 20:      # every capped case with a full set of classes runs from small logits into the cap's flat end
                assert a.min() < 1.0 and a.max() == P.HEAD_CAP, (c, a.min(), a.max())
        for m in seen:
            mref, _, mnan = P.head_ref64(*args, mutant=m)
            seen[m] |= outside(em, np.where(nan, 0.0, mref), bound) or bool((mnan != nan).any())
    print(f"head emulation: max err/bound {worst:.3f}; capped |logit| from {capped_span[0]:.3g} to {capped_span[1]:.3g}")
    assert all(seen.values()), seen
    assert capped_span[0] < 0.1 and capped_span[1] == P.HEAD_CAP      # from small logits to the cap itself
    assert {c["d"] for c in P.head_cases() if c["cap"] > 0} == set(P.HEAD_DS)
    for key, vals in (("style", (0, 1)), ("perm", (False, True)), ("ids", (False, True))):
        for d in P.HEAD_DS:
            assert {c[key] for c in P.head_cases() if c["d"] == d} == set(vals), (key, d)


# ---- split-K reduce + residual + norm ----------------------------------------------------------------------------------------
def test_reduce_emulation_inside_every_mutant_outside():
    seen = dict.fromkeys(P.MUTANTS["reduce"], False)
    for N in P.REDUCE_NS:
        for M in P.REDUCE_MS:
            A_, B_, Rr, w = P.reduce_data(M, N)
            half = P.REDUCE_K // 2
            planes = np.stack([A_[:, :half] @ B_[:, :half].T, A_[:, half:] @ B_[:, half:].T]).astype(np.float32)
            ref, bound = P.reduce_ref64(planes, Rr)
            em = P.reduce_emul32(planes, Rr)
            assert P.ratio(em, ref, bound) <= 1.0, (M, N)
            for m in seen:
                seen[m] |= outside(em, P.reduce_ref64(planes, Rr, mutant=m)[0], bound)
            # the same statement with float64 planes and the GEMM's own error, as the GPU test makes it
            p64, absum = P.split_planes64(A_, B_, 2)
            ref, bound = P.reduce_ref64(p64, Rr, extra=P.REDUCE_K * P.EPS * absum)
            assert P.ratio(em, ref, bound) <= 1.0, (M, N)
            for style in (0, 1):       # the norm of the emulation's own C
                nref, nb = P.rmsnorm_ref64(em, w, P.NORM_EPS, style)
                assert P.ratio(P.rmsnorm_emul32(em, w, P.NORM_EPS, style), nref, nb) <= 1.0, (M, N, style)
    assert all(seen.values()), seen


# ---- sandwich norm -----------------------------------------------------------------------------------------------------------
def test_sandwich_emulation_inside_mutant_outside():
    seen = False
    for d in P.ROW_DS:
        for rows in P.ROW_ROWS:
            h, w_out = P.norm_data(rows, d)
            x, w_next = P.norm_data(rows, d, seed=1)
            x[rows - 1] = bf16_round(x[rows - 1] * np.float32(0.01))     # a residual row far below the normalised h
            ref, bound = P.sandwich_ref64(x, h, w_out, P.NORM_EPS)
            xp, xn = P.sandwich_emul32(x, h, w_out, w_next, P.NORM_EPS)
            assert P.ratio(xp, ref, bound) <= 1.0, (d, rows)
            nref, nb = P.rmsnorm_ref64(xp, w_next, P.NORM_EPS, 1)
            assert P.ratio(xn, nref, nb) <= 1.0, (d, rows)
            seen |= outside(xp, P.sandwich_ref64(x, h, w_out, P.NORM_EPS, mutant="norm_after_add")[0], bound)
    assert seen


# ---- row-scaled epilogues ----------------------------------------------------------------------------------------------------
def test_rowscale_emulations_inside_exact_bit_for_bit_every_mutant_outside():
    from tests.test_gpu_stage2_bounds import gated_ratio

    s = P.ROPE_SHAPE
    cos, sin, _, _ = R.rope_table_hf(s["T"], s["hd"], 1e4)
    seen = {(e, m): False for e in ("rope", "swiglu") for m in P.MUTANTS["rowscale"]}
    for kind in ("exact", "random"):
        for variant in (1, 5):
            K = P.rowscale_K(variant)
            for M in P.ROWSCALE_MS:
                rs = P.row_scales(kind, M, K, M)
                if kind == "exact":
                    assert set(np.log2(rs)) <= set(range(-3, 4)) and (M < 7 or len(set(rs)) == 7)
                pos = ((np.arange(M) * 2654435761) % s["T"]).astype(np.int32)
                # rope
                A_, B_, acc, absum = P.rowscale_operands(kind, M, s["N"], K, M + s["N"])
                em = R.epi_rope(P.rowscale_emul32(A_, B_, rs), pos, cos, sin, s["hd"], s["rot_cols"])
                ref, bound = P.rope_rowscale_ref64(acc, absum, K, rs, pos, cos, sin, s["hd"], s["rot_cols"])
                if kind == "exact":    # every fp32 sum and the scaling are exact: the fp32 restatement is reproduced bit for bit
                    assert np.array_equal(em, R.epi_rope(P.rowscale_value(acc, absum, K, rs)[0], pos, cos, sin, s["hd"], s["rot_cols"]))
                assert P.ratio(em, ref, bound) <= 1.0, (kind, M, K)
                for m in P.MUTANTS["rowscale"]:
                    seen[("rope", m)] |= outside(em, P.rope_rowscale_ref64(acc, absum, K, rs, pos, cos, sin, s["hd"], s["rot_cols"],
                                                                          mutant=m)[0], bound)
                # swiglu
                A_, B_, acc, absum = P.rowscale_operands(kind, M, P.SWIGLU_N, K, M + 7)
                v, u = P.rowscale_value(acc, absum, K, rs)
                em = R.epi_swiglu(P.rowscale_emul32(A_, B_, rs))
                assert gated_ratio(2, v, u * 2.0 ** 24, 1, em) <= 1.0, (kind, M, K)
                for m in P.MUTANTS["rowscale"]:
                    vm, _ = P.rowscale_value(acc, absum, K, rs, mutant=m)
                    seen[("swiglu", m)] |= gated_ratio(2, v, u * 2.0 ** 24, 1, R.epi_swiglu(vm)) > 1.0
    assert all(seen.values()), seen


# ---- bit-exact kernels -------------------------------------------------------------------------------------------------------
def test_exact_references_and_their_mutants():
    for d in P.EMBED_DS:
        ids, src, table = P.embed_data(d)
        plain = P.embed_ref(ids, None, table)
        assert np.array_equal(plain[3], table[0]) and np.array_equal(plain[4], table[0]) and np.array_equal(plain[9], table[0])
        assert np.array_equal(P.embed_ref(ids, src, table), plain[src])
        scaled = P.embed_ref(ids, src, table, P.EMBED_SCALE)
        assert np.array_equal(scaled, bf16_round(scaled)) and not np.array_equal(scaled, P.embed_ref(ids, src, table, P.EMBED_SCALE,
                                                                                                        mutant="scale_dropped"))
        # a bf16 value times a bf16-valued scale is exact in fp32: float64 and fp32 round to the same bits
        assert np.array_equal(scaled, P.r64(plain[src].astype(np.float64) * P.EMBED_SCALE).astype(np.float32))
    for rows, cols in P.FOLD_SHAPES:
        w, nw = P.norm_data(1, cols)[0].repeat(min(rows, 5), 0), P.norm_data(1, cols, seed=3)[1]
        assert np.array_equal(P.fold_norm_ref(w, nw), P.r64(w.astype(np.float64) * nw.astype(np.float64)[None]).astype(np.float32))
    seen = dict.fromkeys(P.MUTANTS["token_meta"], False)
    kinds = set()
    for c in P.meta_cases():
        ref = P.token_meta_ref(c["cu"], c["P"], c["ids"])
        lens = np.diff(c["cu"])
        kinds.add((c["P"], c["B"], c["brk"]))
        assert ref["prefix_bad"] == (1 if c["brk"] else 0), c
        assert (lens > c["P"]).all() and (lens - c["P"] > 256).any()       # one prompt past the block stride of 256
        assert c["B"] == 1 or (lens == c["P"] + 1).any()                   # and one of a single token behind the prefix
        total = len(ref["tok_pos"])
        assert total == int(c["cu"][-1]) - (c["B"] - 1) * c["P"] and ref["seg_start"][-1] == total
        # the restatement against the layout's definition: every internal row maps to one packed token, each prompt's last row
        # to its last token at its last position, and the ids seen through the map are every prompt's ids from the prefix on
        assert len(set(ref["tok_src"])) == total
        for b in range(c["B"]):
            r, p = ref["last_rows"][b], ref["last_pos"][b]
            assert p == lens[b] - 1 and ref["tok_pos"][r] == p and ref["tok_src"][r] == c["cu"][b + 1] - 1
            seg = b + 1 if c["P"] > 0 else b
            rows = slice(ref["seg_start"][seg], ref["seg_start"][seg + 1])
            assert np.array_equal(ref["tok_src"][rows], np.arange(c["cu"][b] + c["P"], c["cu"][b + 1]))
            assert np.array_equal(ref["tok_pos"][rows], np.arange(c["P"], lens[b]))
        for m in seen:
            mut = P.token_meta_ref(c["cu"], c["P"], c["ids"], mutant=m)
            seen[m] |= any(not np.array_equal(mut[k], ref[k]) for k in ref)
    assert all(seen.values()), seen
    assert {k[2] for k in kinds} == {None, "first", "last"}
