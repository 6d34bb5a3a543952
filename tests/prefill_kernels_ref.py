"""Float64 references, element-wise error bounds, fp32 emulations and mutants for the kernels every scored prompt passes through
between the GEMMs and the attention passes (csrc/llama_elem.hip) and for the folded-RMSNorm arm of the GEMM epilogues
(csrc/llama_gemm.hip), reached one at a time through the "exposed for parity tests" entry points of include/llamarec_mi355x.h.
Test infrastructure only: tests/test_prefill_kernels_host.py pins it on the CPU (every emulation inside its bound, every mutant
outside, on the data the GPU tests use), tests/test_gpu_prefill_kernels.py compares the HIP kernels with it.

Conventions: those of tests/lora_kernels_ref.py, whose ulp, ulp32, EPS, r64, ratio are used here. eps = 2^-24 is one fp32
operation; a *reference* is float64 with the kernel's bf16 rounding points restated and nothing else rounded; a *bound* is derived
from the fp32 operations that remain, never fitted to a kernel's output; an *emulation* does the kernel's arithmetic in fp32 numpy
with another summation order; a *mutant* is the reference with one plausible bug. Where a rounding follows a sum the bound is
"the chain evaluated at value +- its fp32 error" (the roundings are monotone), so most elements get a bound of zero beyond the
carried error, which is what lets a mutant that differs by one rounding show.

square sum      ss = sum x^2, x bf16 (x^2 is exact in fp32), one fma per term: a thread of rmsnorm_kernel /
                reduce_residual_rmsnorm_kernel / residual_postnorm_kernel takes the 8-column chunks t + 256 k, so at most
                n_t = 8 ceil(d / 2048) <= 8 RMS_KEEP steps (the two-pass branch past 8192 columns: the same count, d / 256),
                then the 6-step butterfly and the 4-way add of block_sum_256: 9 more. head_kernel's threads take single columns:
                n_t = ceil(d / 256), + 9. rms_rstd_kernel's lanes take chunks lane + 64 k: n_t = 8 ceil(d / 512), + 6 (no
                4-way add). All terms are positive, so the error is relative: e_ss = (n_t + tree) eps.
rstd            1 / sqrtf(ss / d + eps_n): e_r = e_ss / 2 + 6 eps. The division and the add sit under the root and count half;
                the division, the root and the reciprocal are taken at 1 ulp = 2 eps each, which holds whether or not the
                compiler emits the correctly rounded forms: (2 + 1) / 2 + 2 + 2 = 5.5, rounded up. d is exact.
                lr_rms_rstd_f32 returns it: bound = e_r rstd.
style 0         bf16(w bf16(x rstd)): t = x rstd is one fp32 product, relative e = e_r + eps; the inner rounding is evaluated
                at t (1 +- e); w times a bf16 value is exact in fp32, so the outer rounding is the only other one.
style 1         bf16(x rstd (1 + w)): three fp32 operations (1 + w may round), e = e_r + 3 eps, then one rounding.
head            xn as above (style's chain) with head_kernel's n_t. acc = sum_k xn[k] W[id_c][k]: products exact, d fma terms
                in lane-strided order and the butterfly: d eps sum|xn||W|; where xn[k]'s interval straddles a rounding boundary
                its width D_k is carried as sum|W_k| D_k. Then bf16(acc) as a chain. With a cap the kernel computes
                bf16(bf16(tanhf(bf16(bf16(acc) / cap))) cap): four roundings around one fp32 division (eps), tanhf and one fp32
                product (eps). tanhf: the HIP math API's accuracy table gives 2 ulp for tanhf; 2^-21 relative is taken, the
                figure tests/test_gpu_stage2_bounds.py's gated_ratio uses for the same function in GeGLU. Every step is
                monotone in acc (cap > 0), so the chain is walked once with every error pushed down and once up.
                An id outside [0, vocab) is NaN exactly there; *poison != 0 is NaN everywhere.
fused reduce    C = bf16(bf16(sum_s plane_s) + R): planes added in split order, S - 1 additions: S eps sum|plane_s| (+ what the
                planes themselves carry when they come out of an fp32 GEMM: K eps sum|a||b|, the residual-epilogue bound of
                tests/test_gpu_stage2_bounds.py); the chain at sum +- that. xn = norm(C) is judged against the norm of THE
                KERNEL'S OWN C (the attention backward's convention): the two outputs are tested as what they are, a sum and
                a norm of the stored row.
sandwich norm   x' = bf16(x + bf16(h rstd_h (1 + w_out))): style 1's chain, then an fp32 add of two bf16 values, which may
                round (eps), then one rounding: walked down and up. xn = style 1 of the kernel's own x' with w_next.
row scale       v = fp32(acc rs): |rs| E_acc + eps |acc rs| where E_acc = K eps sum|a||b| is the accumulator's own error (0 on
                exact operands), then the rope epilogue as a chain (x = bf16(v) at v +- u; the rotation of bf16 values by
                bf16 (cos, sin) has exact products and one fp32 addition; one rounding, at both ends) or
                tests/test_gpu_stage2_bounds.py's gated_ratio with that uncertainty on gate and up. rs is an input, any fp32.
bit-exact       embed (bf16(e scale), scale a bf16 value: exact product, one rounding; ids outside [0, vocab) read row 0),
                fold_norm (bf16(w nw): the same), gather_rows, token_meta (integers): the reference is matched bit for bit.
"""
from __future__ import annotations

import numpy as np

from llamarec_amd.synth import bf16_round, hash_uniform, splitmix64
from tests import stage2_ref as R
from tests.lora_kernels_ref import EPS, TINY, f32, r64, ratio, ulp, ulp32  # noqa: F401  (re-exported to the two test files)

TANH_REL = 2.0 ** -21

MUTANTS = {
    "norm": ("eps_missing", "mean_over_chunks", "style_swapped", "inner_rounding_missing", "weight_of_next_chunk",
             "second_piece_dropped"),
    "head": ("row_b_not_rows_b", "class_index_not_id", "last_partial_k_step_dropped", "cap_one_rounding"),
    "reduce": ("plane_dropped", "residual_before_rounding"),
    "sandwich": ("norm_after_add",),
    "rowscale": ("scale_of_next_row", "scale_after_rounding"),
    "token_meta": ("positions_restart_after_prefix", "last_pos_off_by_one"),
    "embed": ("scale_dropped",),
}


# ---- square sum, rstd --------------------------------------------------------------------------------------------------------
def steps(kernel, d):
    """fp32 additions behind one row's square sum (see the module docstring)."""
    if kernel == "head":
        return -(-d // 256) + 9
    if kernel == "rstd":
        return 8 * -(-d // 512) + 6
    return 8 * -(-d // 2048) + 9


def e_rstd(kernel, d):
    return steps(kernel, d) * EPS / 2 + 6 * EPS


def rstd_ref64(x, eps, kernel="rstd", mutant=None):
    """(rstd [rows][1], bound) float64."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[-1]
    xs = x[..., :2048] if mutant == "second_piece_dropped" else x
    dn = d / 8.0 if mutant == "mean_over_chunks" else float(d)
    e = 0.0 if mutant == "eps_missing" else float(np.float32(eps))
    with np.errstate(divide="ignore"):
        rstd = 1.0 / np.sqrt((xs * xs).sum(-1, keepdims=True) / dn + e)
    return rstd, e_rstd(kernel, d) * rstd + TINY


def rstd_emul32(x, eps):
    x = f32(x)
    ss = (x * x)[..., ::-1].sum(-1, dtype=np.float32, keepdims=True)
    return np.float32(1) / np.sqrt(ss / np.float32(x.shape[-1]) + np.float32(eps))


# ---- RMSNorm, both styles ----------------------------------------------------------------------------------------------------
def _apply(t, w, style, inner=True):
    if style == 0:
        return r64(w * (r64(t) if inner else t))
    return r64(t * (1.0 + w))


def rmsnorm_ref64(x, w, eps, style, kernel="norm", mutant=None):
    """x [rows][d], w [d] bf16 values. Returns (out, bound) float64 [rows][d]; out carries the kernel's roundings."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    d = x.shape[-1]
    rstd, _ = rstd_ref64(x, eps, kernel, mutant)
    if mutant == "style_swapped":
        style = 1 - style
    if mutant == "weight_of_next_chunk":
        w = np.roll(w, -8)
    e = e_rstd(kernel, d) + (EPS if style == 0 else 3 * EPS)
    with np.errstate(invalid="ignore"):
        t = x * rstd
        out = _apply(t, w, style, inner=mutant != "inner_rounding_missing")
        lo, hi = _apply(t * (1 - e), w, style), _apply(t * (1 + e), w, style)
    return out, np.maximum(np.abs(lo - out), np.abs(hi - out)) + TINY


def rmsnorm_emul32(x, w, eps, style):
    x, w = f32(x), f32(w)
    rstd = rstd_emul32(x, eps)
    if style == 0:
        return bf16_round(w * bf16_round(x * rstd))
    return bf16_round(x * rstd * (np.float32(1) + w))


def norm_data(rows, d, seed=0):
    """(x [rows][d], w [d]) bf16 values. Row 0 is unit-scale random; with 5 rows: row 1 all zero, row 2 of magnitude
    sqrt(NORM_EPS) (so that a dropped eps shows), row 3 random with one 1e4 outlier in its LAST column (so that a dropped second
    register piece shows), row 4 random at 2^6. w: random, scaled by a factor that changes from one 8-column chunk to the next."""
    x = hash_uniform(7001 + 13 * d + seed, (rows, d), 1.0)
    if rows >= 5:
        x[1] = 0.0
        x[2] *= np.float32(np.sqrt(NORM_EPS))
        x[3, d - 1] = 1.0e4
        x[4] *= np.float32(64.0)
    chunk = (np.arange(d) // 8) % 5
    w = hash_uniform(7002 + 13 * d + seed, (d,), 0.5) + np.float32(0.25) * chunk.astype(np.float32)
    return bf16_round(x), bf16_round(w)


NORM_EPS = 1e-5
ROW_DS = (8, 64, 2040, 2048, 2056, 4096, 8192)      # below a chunk per thread, exactly 256 chunks, the second register piece, the keep limit
ROW_ROWS = (1, 5)
TWO_PASS_D = 8200                                   # rmsnorm_kernel's two-pass branch (the others refuse it)
RSTD_ROWS = (1, 4, 5)                               # rms_rstd_kernel handles 4 rows per workgroup


# ---- head --------------------------------------------------------------------------------------------------------------------
def _down(v, rel):
    return v - np.abs(v) * rel


def _up(v, rel):
    return v + np.abs(v) * rel


def _cap_chain(acc, cap, direction):
    """bf16(bf16(tanhf(bf16(bf16(acc) / cap))) cap) with every fp32 error pushed down (-1), up (+1) or absent (0)."""
    push = (lambda v, rel: v) if direction == 0 else (_down if direction < 0 else _up)
    q = r64(push(r64(acc) / cap, EPS))
    t = r64(push(np.tanh(q), TANH_REL))
    return r64(push(t * cap, EPS))


def head_ref64(x, rows, norm_w, lm_head, class_ids, B, C, eps, style, cap=0.0, poison=0, mutant=None):
    """x [n][d], norm_w [d], lm_head [vocab][d] bf16 values; rows [B] / class_ids [C] int or None. Returns (out, bound, nan):
    out / bound float64 [B][C], nan bool [B][C] = where the kernel must write NaN (out is 0 there)."""
    x, W = np.asarray(x, dtype=np.float64), np.asarray(lm_head, dtype=np.float64)
    vocab, d = W.shape
    rr = np.arange(B) if (rows is None or mutant == "row_b_not_rows_b") else np.asarray(rows, dtype=np.int64)
    ids = np.arange(C) if (class_ids is None or mutant == "class_index_not_id") else np.asarray(class_ids, dtype=np.int64)
    nan = np.broadcast_to(((ids < 0) | (ids >= vocab))[None, :], (B, C)).copy()
    if poison:
        nan[:] = True
    xn, D = rmsnorm_ref64(x[rr], norm_w, eps, style, kernel="head")
    Wc = W[np.clip(ids, 0, vocab - 1)]
    if mutant == "last_partial_k_step_dropped":
        Wc = Wc.copy()
        Wc[:, d // 512 * 512:] = 0.0
    acc = xn @ Wc.T
    E = d * EPS * ((np.abs(xn) + D) @ np.abs(Wc).T) + D @ np.abs(Wc).T
    if cap > 0:
        c = float(np.float32(cap))
        out = r64(c * np.tanh(acc / c)) if mutant == "cap_one_rounding" else _cap_chain(acc, c, 0)
        lo, hi = _cap_chain(acc - E, c, -1), _cap_chain(acc + E, c, +1)
    else:
        out, lo, hi = r64(acc), r64(acc - E), r64(acc + E)
    bound = np.maximum(np.abs(lo - out), np.abs(hi - out)) + TINY
    return np.where(nan, 0.0, out), bound, nan


def head_emul32(x, rows, norm_w, lm_head, class_ids, B, C, eps, style, cap=0.0):
    """fp32 values of the live columns (the caller masks the NaN ones)."""
    W = f32(lm_head)
    vocab = W.shape[0]
    rr = np.arange(B) if rows is None else np.asarray(rows, dtype=np.int64)
    ids = np.arange(C) if class_ids is None else np.asarray(class_ids, dtype=np.int64)
    xn = rmsnorm_emul32(f32(x)[rr], norm_w, eps, style)
    Wc = W[np.clip(ids, 0, vocab - 1)]
    acc = (xn[:, None, :] * Wc[None, :, :])[..., ::-1].sum(-1, dtype=np.float32)
    if cap > 0:
        c = np.float32(cap)
        q = bf16_round(bf16_round(acc) / c)
        t = bf16_round(np.tanh(q.astype(np.float64)).astype(np.float32))
        return bf16_round(t * c)
    return bf16_round(acc)


HEAD_VOCAB = 300
HEAD_DS = (64, 512, 520, 4096)          # one partial k step, one whole, one whole + a partial one, eight
HEAD_BS = (1, 3)
HEAD_CS = (1, 20, 32, 33, 70)           # one class, a part-full / full / just-over-full group of 32, three groups
HEAD_CAP = 30.0


def head_cases():
    """Every (d, B, C) once; style, rows (None / a permutation), class_ids (None / given) and the cap rotate on the indices so
    that each value meets each d, B and C. A cap goes with style 1 only."""
    for a, d in enumerate(HEAD_DS):
        for b, B in enumerate(HEAD_BS):
            for c, C in enumerate(HEAD_CS):
                capped = (a + b + c) % 3 == 0
                yield dict(d=d, B=B, C=C, style=1 if capped else (a + c) % 2, perm=bool((a + b + c // 2) % 2),
                           ids=bool((b + c + a // 2) % 2), cap=HEAD_CAP if capped else 0.0, seed=10 * (5 * a + c) + b)


def head_data(c):
    """(x [B + 2][d], rows or None, norm_w, lm_head [300][d], class_ids or None). With class ids: distinct in-vocabulary rows, and
    -1 and vocab at two positions once C allows. With a cap the lm_head rows are scaled so that the logits run from about 0.1 to
    beyond 20 x cap."""
    d, B, C, s = c["d"], c["B"], c["C"], c["seed"]
    x = bf16_round(hash_uniform(7100 + s, (B + 2, d), 1.0))
    norm_w = bf16_round(hash_uniform(7101 + s, (d,), 0.5) + np.float32(0.25) * ((np.arange(d) // 8) % 5).astype(np.float32))
    W = hash_uniform(7102 + s, (HEAD_VOCAB, d), 1.0 / np.sqrt(d))
    if c["cap"] > 0:
        W *= np.geomspace(0.1, 40.0 * c["cap"], 20).astype(np.float32)[np.arange(HEAD_VOCAB) % 20, None]   # any 20 rows span it
    rows = (np.arange(B)[::-1] + 2).astype(np.int32) if c["perm"] else None
    ids = None
    if c["ids"]:
        ids = ((np.arange(C) * 37 + 11) % HEAD_VOCAB).astype(np.int32)
        if C >= 20:
            ids[3], ids[C - 1] = -1, HEAD_VOCAB
    return x, rows, norm_w, bf16_round(W), ids


# ---- split-K reduce + residual + norm ----------------------------------------------------------------------------------------
def reduce_ref64(planes, Rr, extra=0.0, mutant=None):
    """planes [S][M][N] (fp32 values, or float64 exact partial products with `extra` = the fp32 GEMM's own error on their sum),
    Rr [M][N] bf16 values. Returns (C, bound): the chain bf16(bf16(sum) + R) at sum +- (S eps sum|plane| + extra)."""
    p = np.asarray(planes, dtype=np.float64)
    S = p.shape[0]
    Rr = np.asarray(Rr, dtype=np.float64)
    E = S * EPS * np.abs(p).sum(0) + extra
    tot = (p[:-1] if mutant == "plane_dropped" else p).sum(0)

    def chain(v):
        return r64(r64(v) + Rr)

    out = r64(tot + Rr) if mutant == "residual_before_rounding" else chain(tot)
    return out, np.maximum(np.abs(chain(tot - E) - out), np.abs(chain(tot + E) - out)) + TINY


def reduce_emul32(planes, Rr):
    p = f32(planes)
    tot = p[-1]
    for s in reversed(range(p.shape[0] - 1)):     # last to first
        tot = tot + p[s]
    return bf16_round(bf16_round(tot) + f32(Rr))


REDUCE_NS = (256, 2048, 2304)
REDUCE_MS = (1, 7, 257)
REDUCE_K = 2048
UNFUSED_N = 8448                        # past the keep limit: the reduce pass and the norm stay two launches


def reduce_data(M, N, K=REDUCE_K, seed=0):
    """(A [M][K], B [N][K], R [M][N], w [N]) bf16 values at the scales of tests/test_gpu_stage2_bounds.py's random operands."""
    A = bf16_round(hash_uniform(7200 + M + seed, (M, K), 1.0))
    B = bf16_round(hash_uniform(7201 + N + seed, (N, K), 0.05))
    Rr = bf16_round(hash_uniform(7202 + M * 3 + N + seed, (M, N), 4.0))
    w = bf16_round(hash_uniform(7203 + N + seed, (N,), 0.5) + np.float32(0.25) * ((np.arange(N) // 8) % 5).astype(np.float32))
    return A, B, Rr, w


def split_planes64(A, B, S):
    """float64 partial products of S contiguous K ranges, and sum|a||b| over all of K."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    K = A.shape[1]
    cuts = [K * s // S for s in range(S + 1)]
    planes = np.stack([A[:, cuts[s]:cuts[s + 1]] @ B[:, cuts[s]:cuts[s + 1]].T for s in range(S)])
    return planes, np.abs(A) @ np.abs(B).T


# ---- sandwich norm -----------------------------------------------------------------------------------------------------------
def sandwich_ref64(x, h, w_out, eps, mutant=None):
    """x' = bf16(x + bf16(gemmanorm(h, w_out))). Returns (x', bound) float64."""
    x, h, w = (np.asarray(v, dtype=np.float64) for v in (x, h, w_out))
    d = x.shape[-1]
    if mutant == "norm_after_add":
        return rmsnorm_ref64(r64(x + h), w, eps, 1)[0], None
    rstd, _ = rstd_ref64(h, eps, "norm")
    t = h * rstd
    e = e_rstd("norm", d) + 3 * EPS
    n, n_lo, n_hi = (r64(v * (1.0 + w)) for v in (t, t * (1 - e), t * (1 + e)))
    n_lo, n_hi = np.minimum(n_lo, n_hi), np.maximum(n_lo, n_hi)
    out = r64(x + n)
    lo, hi = r64(_down(x + n_lo, EPS)), r64(_up(x + n_hi, EPS))
    return out, np.maximum(np.abs(lo - out), np.abs(hi - out)) + TINY


def sandwich_emul32(x, h, w_out, w_next, eps):
    xp = bf16_round(f32(x) + rmsnorm_emul32(h, w_out, eps, 1))
    return xp, (rmsnorm_emul32(xp, w_next, eps, 1) if w_next is not None else None)


# ---- row-scaled epilogues ----------------------------------------------------------------------------------------------------
ROWSCALE_MS = (1, 7, 255, 257, 517)
ROWSCALE_VARIANTS = (1, 4, 5)
ROPE_SHAPE = dict(N=768, rot_cols=512, hd=128, T=512)
SWIGLU_N = 512


def rowscale_K(variant):
    return 2048 if variant == 5 else 256      # variant 5 must really split: at least 32 K tiles


def rowscale_operands(kind, M, N, K, seed):
    """tests/test_gpu_stage2_bounds.py's _operands, with sum|a||b| (zero for the exact kind, whose fp32 sums are exact)."""
    if kind == "exact":
        A = np.round(hash_uniform(seed + M, (M, K), 2.0)) * np.float32(0.25)
        B = np.round(hash_uniform(seed + N, (N, K), 3.0)) * np.float32(0.125)
        A[M // 2] = 0.0
    else:
        A = bf16_round(hash_uniform(seed + M, (M, K), 1.0))
        B = bf16_round(hash_uniform(seed + N, (N, K), 0.05))
    acc = A.astype(np.float64) @ B.astype(np.float64).T
    absum = np.zeros_like(acc) if kind == "exact" else np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T
    return A.astype(np.float32), B.astype(np.float32), acc, absum


def row_scales(kind, M, K, seed):
    """fp32 [M]. exact: powers of two from 2^-3 to 2^3 varying per row; random: 1 / rms of a random row of K values whose scale
    varies per row (what rms_rstd_kernel hands the epilogue)."""
    if kind == "exact":
        return (2.0 ** ((np.arange(M) * 5 + seed) % 7 - 3)).astype(np.float32)
    x = hash_uniform(7300 + seed + M, (M, K), 1.0) * (1.0 + (np.arange(M) % 9)[:, None]).astype(np.float32)
    return rstd_emul32(bf16_round(x), NORM_EPS)[:, 0].astype(np.float32)


def rowscale_value(acc, absum, K, rs, mutant=None):
    """(v, u): the scaled accumulator in float64 and its fp32 uncertainty |rs| K eps sum|a||b| + eps |v|."""
    rs = np.asarray(rs, dtype=np.float64)
    if mutant == "scale_of_next_row":
        rs = np.roll(rs, -1)
    v = (r64(acc) if mutant == "scale_after_rounding" else acc) * rs[:, None]
    return v, np.abs(rs)[:, None] * K * EPS * absum + EPS * np.abs(v)


def rope_rowscale_ref64(acc, absum, K, rs, pos, cos, sin, hd, rot_cols, mutant=None):
    """(out, bound) float64 [M][N]: the rope epilogue on the scaled accumulator as a chain. x = bf16(v) is evaluated at v +- u
    (D = how far it moves: zero unless the interval straddles a rounding boundary); the rotation a c - b s, b c + a s of bf16
    values has exact products and one fp32 addition, eps (|a c| + |b s|), and carries the operands' moves as |c| D_a + |s| D_b;
    then one rounding, evaluated at both ends. Columns from rot_cols on are bf16(v) itself."""
    v, u = rowscale_value(acc, absum, K, rs, mutant)
    x = r64(v)
    D = np.maximum(np.abs(r64(v - u) - x), np.abs(r64(v + u) - x))
    M = x.shape[0]
    xh, Dh = x[:, :rot_cols].reshape(M, -1, hd), D[:, :rot_cols].reshape(M, -1, hd)
    o = R.rope_rotate64(xh, pos, cos, sin)
    p = np.asarray(pos, dtype=np.int64)
    c, s = np.abs(np.asarray(cos, dtype=np.float64))[p][:, None, :], np.abs(np.asarray(sin, dtype=np.float64))[p][:, None, :]
    a, b, Da, Db = np.abs(xh[..., 0::2]), np.abs(xh[..., 1::2]), Dh[..., 0::2], Dh[..., 1::2]
    U = np.empty_like(o)
    U[..., 0::2] = c * Da + s * Db + EPS * (a * c + b * s)
    U[..., 1::2] = c * Db + s * Da + EPS * (b * c + a * s)
    rot = r64(o)
    rb = np.maximum(np.abs(r64(o - U) - rot), np.abs(r64(o + U) - rot))
    out = np.concatenate([rot.reshape(M, -1), x[:, rot_cols:]], 1)
    return out, np.concatenate([rb.reshape(M, -1), D[:, rot_cols:]], 1) + TINY


def rowscale_emul32(A, B, rs):
    """fp32 accumulator (numpy's blocked order) times the row scale in fp32."""
    return (f32(A) @ f32(B).T) * f32(rs)[:, None]


# ---- bit-exact kernels -------------------------------------------------------------------------------------------------------
def embed_ref(ids, tok_src, table, scale=1.0, mutant=None):
    ids = np.asarray(ids, dtype=np.int64)
    table = f32(table)
    src = np.arange(len(ids) if tok_src is None else len(tok_src)) if tok_src is None else np.asarray(tok_src, dtype=np.int64)
    i = ids[src]
    i = np.where((i < 0) | (i >= table.shape[0]), 0, i)
    e = table[i]
    if scale == 1.0 or mutant == "scale_dropped":
        return e
    return bf16_round(e * np.float32(scale))


def fold_norm_ref(w, nw):
    return bf16_round(f32(w) * f32(nw)[None, :])


def token_meta_ref(cu, P, ids=None, mutant=None):
    """numpy restatement of token_meta_kernel. Returns dict seg_start, tok_pos, tok_src, last_rows, last_pos, prefix_bad."""
    cu = np.asarray(cu, dtype=np.int64)
    B = len(cu) - 1
    total = int(cu[B] - cu[0]) - (B - 1) * P if P > 0 else int(cu[B])
    tok_pos, tok_src = np.zeros(total, np.int32), np.zeros(total, np.int32)
    seg_start, last_rows, last_pos, bad = [], np.zeros(B, np.int32), np.zeros(B, np.int32), 0
    if P > 0:
        seg_start.append(0)
        tok_pos[:P], tok_src[:P] = np.arange(P), cu[0] + np.arange(P)
    for b in range(B):
        s, e = int(cu[b]), int(cu[b + 1])
        start, n, pos0 = (P + s - b * P, e - s - P, P) if P > 0 else (s, e - s, 0)
        if P > 0 and mutant == "positions_restart_after_prefix":
            pos0 = 0
        seg_start.append(start)
        tok_pos[start:start + n], tok_src[start:start + n] = pos0 + np.arange(n), s + P + np.arange(n)
        last_rows[b], last_pos[b] = start + n - 1, pos0 + n - 1 + (1 if mutant == "last_pos_off_by_one" else 0)
        if P > 0 and b > 0 and ids is not None:
            bad |= int(np.any(np.asarray(ids)[s:s + P] != np.asarray(ids)[cu[0]:cu[0] + P]))
    seg_start.append(seg_start[-1] + n)
    return dict(seg_start=np.array(seg_start, np.int32), tok_pos=tok_pos, tok_src=tok_src, last_rows=last_rows, last_pos=last_pos,
                prefix_bad=bad)


META_PS = (0, 1, 36)
META_BS = (1, 2, 5)


def meta_cases():
    """(P, B, lens, ids, break_at): lengths include P + 1 and one above 256 (the block stride). break_at None: every prompt keeps
    the prefix; "first" / "last": one prompt differs at the prefix's first / last position."""
    for P in META_PS:
        for B in META_BS:
            lens = [P + 1, P + 300, P + 17, P + 256, P + 2][:B]
            if B == 1:
                lens = [P + 300]
            elif B == 2:
                lens = [P + 1, P + 300]
            for brk in ((None, "first", "last") if (P > 0 and B > 1) else (None,)):
                cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
                ids = (splitmix64(7400 + P + B, int(cu[-1])) % np.uint64(1000)).astype(np.int32) + 5
                for b in range(1, B):
                    ids[cu[b]:cu[b] + P] = ids[:P]
                if brk:
                    b = B - 1 if brk == "first" else 1
                    ids[cu[b] + (0 if brk == "first" else P - 1)] += 1
                yield dict(P=P, B=B, cu=cu, ids=ids, brk=brk)


EMBED_DS = (8, 2048, 2056)
EMBED_VOCAB = 50
EMBED_SCALE = float(bf16_round(np.array([np.sqrt(2048.0)], np.float32))[0])
FOLD_SHAPES = ((1, 8), (5, 2056), (300, 4096))
GATHER_DS = (8, 4096)


def embed_data(d, seed=0):
    """(ids [11] with -1 and vocab among them, a permutation tok_src, table [50][d])."""
    table = bf16_round(hash_uniform(7500 + d + seed, (EMBED_VOCAB, d), 0.02))
    ids = np.array([3, 0, 49, -1, 50, 17, 17, 1, 48, 10 ** 6, 2], np.int32)
    src = np.array([10, 3, 4, 0, 9, 6, 5, 1, 2, 8, 7], np.int32)
    return ids, src, table
