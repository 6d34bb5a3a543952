"""Float64 references, element-wise error bounds, fp32 emulations and mutants for the small kernels of the ranker's LoRA step
(csrc/llama_train.hip), reached one at a time through the "exposed for parity tests" entry points of include/llamarec_mi355x.h.
Test infrastructure only: tests/test_lora_kernels_host.py pins it on the CPU (every emulation inside its bound, every mutant
outside, on the data the GPU tests use), tests/test_gpu_lora_kernels.py compares the HIP kernels with it.

Conventions (those of tests/stage2_ref.py and tests/qwen3_ref.py). eps = 2^-24, the relative error of one fp32 operation.
ulp(v) is the bf16 step at 1.01 |v| (a value just below a power of two gets the step above it), ulp32 the fp32 one. r64 is a
rounding to bf16 (through fp32, as the kernels round). A *reference* is float64 with the kernel's bf16 rounding points restated
and nothing else rounded; a *bound* is derived from the fp32 operations that remain and is never fitted to a kernel's output; an
*emulation* performs the kernel's arithmetic in fp32 / bf16 numpy with another summation order; a *mutant* is the reference
with one plausible kernel bug. Where a rounding follows a sum, the bound is "the chain evaluated at sum +- its fp32 error": the
roundings are monotone, so the kernel's value lies between the two evaluations, and most elements get a bound of zero beyond
the carried error -- which is what lets a mutant that differs by one rounding show.

Dropout. keep(stream, row, col) restates lt_keep for any 32-bit stream; the threshold is uint32(float32(p) 2^32) and the scale
ds = fp32(1 / fp32(1 - p)), both as the launchers compute them. A dropped operand is x' = bf16(fp32(x ds)) where kept, else 0:
one operation per element, so references and emulations share it bit for bit (dropped()).

skinny          out = bf16(scale acc), acc = sum_k x'[k] w[k] by MFMA (fp32 accumulate; 4 waves' partial tiles added through
                LDS). No wave adds more than K / 4 + 3 terms (its share of the K steps, then the
                four tiles), and the product by scale is one more operation: |acc' - acc| <= K eps sum|x'||w| for every K >= 64;
                bound = ulp(scale acc) + K eps |scale| sum|x'||w|.
token reduction out += scale sum_tok t[tok][j] x'[tok][c]: fp32 MFMA sums over a chunk's tokens, one multiply by scale, then one
                fp32 atomic per chunk or a fold in chunk order, onto an output that holds a value already:
                bound = (tokens + chunks + 2) eps |scale| sum|t||x'| + ulp32(result), tokens = those of one chunk (every
                chunk's sum carries at most that many additions, and sum|t||x'| runs over all of them). Layouts 1 and 2 take one
                tile, layout 0 one or two, layout 3 two. tn_chunk restates the launcher's chunk policy (32 tokens below 512, 128 below 4096, else 256).
expand          y' = bf16(y + bf16(bf16(l) s)) where kept, l an fp32 fma chain over r: the chain at l +- r eps sum|t||w|.
swiglu backward sg = 1 / (1 + __expf(-g)); dg = bf16(dy u (sg (1 + g (1 - sg)))); du = bf16(dy (g sg)).
                __expf(x) = v_exp_f32(x log2e): the product's rounding is |x| eps in the exponent, the instruction 1 ulp:
                relative (|g| + 1) 2^-23; the add and the division one eps each: e_s = (|g| + 3) 2^-23 relative on sg.
                F = 1 + g (1 - sg) cancels at g ~ -1.2785, so its error is absolute: e_F = |g| (sg e_s + 2 eps) + eps (1 + |g|).
                |dg' - dg| <= ulp + |dy u| sg (e_F + |F| (e_s + 3 eps)); |du' - du| <= ulp + |dy g| sg (e_s + 2 eps).
                For g < -87 e^-g leaves fp32's range and sg becomes 0: there the whole value may vanish (bound += |ref|); a
                result below 2^-126 may be flushed (bound += 2^-126).
rmsnorm backward g = w dy; rstd = 1 / sqrt(sum x^2 / d + eps_n); coef = (sum x g / d) rstd^3; dx = rstd g - x coef, fp32, rounded
                once; with res: bf16(bf16(dx) + res). Sums of d terms, products rounded (no contraction): relative (d + 1) eps
                of sum|.|. e_r = (d / 2 + 5) eps relative on rstd (half the sum's, the division, the add, the root, the
                reciprocal). |dx' - dx| <= E = |rstd g| (e_r + 3 eps) + |x| rstd^3 (d + 1) eps sum|x g| / d
                + |x coef| (3 e_r + 6 eps). Without res: bound = ulp(dx) + E. With res: the chain v -> bf16(bf16(v) + res) at
                dx +- E. LoRA arm: dy = bf16(dy + bf16(fp32(l ds))) where kept, l an fma chain over 2r terms: evaluated at
                l +- (2r + 1) eps sum|t||a|; a change D of dy there is carried as rstd |w| D + |x| rstd^3 sum(|x||w| D) / d.
cross-entropy   p = __expf(x - mx) / se: e_j = (|x_j - mx| + 2) 2^-23 on each exponential (the subtraction of two bf16 values
                may round), se of V terms in V / 256 steps per thread and a 9-step tree: (V / 256 + 10) eps + sum p_j e_j;
                the division and the product 3 eps. d logits = bf16((p - onehot) gscale): |gscale| (p e_p + 2 eps |p - 1|) +
                ulp -- absolute at the target column, where p - 1 cancels. Below e^-86 the exponential underflows (+= p).
                loss_i = logf(se) + mx - x[target]: the sum's relative error, logf at 2^-22 |log se| + eps, two additions
                eps (|log se + mx| + |loss_i|) -- with logits near -3e4 that is 2e-3 absolute, and the bound says so. out[0] =
                sum_i loss_i / m over ALL m rows (the kernel documents the mean over the rows it is given; a row without a token
                id adds 0): (m + 2) eps sum|loss_i| / m on top. out[1] = m, out[2] = rows without a token id, exact.
rowdot          hd eps sum|o||do| (hd products, hd - 1 additions in some order).
AdamW           torch.optim.AdamW after clip_grad_norm_, oracle/llama_train_oracle.py's clip_and_adamw with the hyper-parameters
                at their fp32 values. sum g^2: relative e_ss = (n / (256 blocks) + blocks + 32) eps (thread chains, trees, one
                atomic per block; the one-workgroup deterministic sum is shorter); norm e_n = e_ss / 2 + eps; the clip
                coefficient, when active, e_c = e_n + 3 eps; g coef: e_g = e_c + eps.
                m' = b1 m + (1 - b1) g: E_m = eps |b1 m| + |(1 - b1) g| (e_g + eps) + eps |m'|  (1 - b1 is exact in fp32)
                v' = b2 v + (1 - b2) g^2: E_v = eps |b2 v| + (1 - b2) g^2 (2 e_g + 2 eps) + eps v'
                bc = 1 - powf(b, step): powf relative (|step log2 b| + 1) 2^-22 (covers exp2(y log2 x) as well as a correctly
                rounded powf), absolute on bc: at step 1 and b2 = 0.999 that is 2.4e-7 against 1e-3 -- the largest term of
                the first steps. r_bc = E_bc / bc.
                upd = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps_a): relative r_bc1 + 4 eps + (E_v / (2 v') + r_bc2 / 2 +
                4 eps) and (lr / bc1) E_m / denominator; p' = p (1 - lr wd) - upd: 3 eps |p| + E_upd + eps |p'|.
                out_norm: e_n |norm| + ulp32.

forward sweep   q, v (and k with its adapter) get expand's delta chain; then, with Qwen3's norms, tests/qwen3_ref.py's sweep_ref64
                and its bound unchanged (two roundings of the norm, the rotation's three fp32 operations, one rounding); without
                them its rotation alone. A move D of a post-delta value is carried through the norm as
                |w| (rstd D + |x| rstd^3 sum(|x| D) / hd) and through the rotation as |c| D_a + |s| D_b. v is the delta alone.
                xsave is the post-delta q | k exactly.
rope backward   a c + b s, b c - a s: two fp32 products and a sum (2^-22 (|a c| + |b s|)), one rounding. Nothing to reorder: the
                fp32 numpy restatement is the kernel bit for bit.
swiglu + lora   gate and up each get expand's delta chain and are written back; h is swiglu_bf16 of the sums, judged by
                tests/test_gpu_stage2_bounds.py's gated_ratio with the chains' moves as the operands' uncertainty.
swiglu forward  swiglu_bf16 on bf16 inputs: gated_ratio with no uncertainty.
prep, transpose bit-exact: one rounding of an fp32 master per element, each element placed once.

Exact operand kinds: small integers times powers of two with power-of-two scales make every fp32 sum exact, so the kernel must
return the restated rounding chain bit for bit whatever the order of its additions and atomics.
"""
from __future__ import annotations

import numpy as np

from llamarec_amd.synth import bf16_round, hash_uniform, splitmix64

EPS = 2.0 ** -24
TINY = 2.0 ** -100

MUTANTS = {
    "skinny": ("k_step_dropped", "wrong_tile"),
    "tn": ("last_partial_step_dropped", "tail_rows_not_zeroed", "no_deinterleave", "gate_up_swapped", "assign_not_add"),
    "expand": ("scale_missing", "mask_of_next_row", "product_not_rounded"),
    "swiglu_bwd": ("dg_du_swapped", "no_g_term"),
    "rmsnorm_bwd": ("coef_missing", "mean_over_chunks", "res_before_rounding", "mask_of_next_row"),
    "ce": ("no_onehot", "gscale_missing", "mean_over_live_rows"),
    "rowdot": ("second_step_missing",),
    "adamw": ("no_clip", "bias_step_minus_one"),
    "rope_fwd": ("delta_after_rotation", "norm_before_delta"),
    "rope_bwd": ("forward_rotation",),
    "swiglu_lora": ("gate_up_ranks_swapped",),
}


# ---- number formats ----------------------------------------------------------------------------------------------------------
def ulp(v):
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)) * 1.01, 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def ulp32(v):
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)) * 1.01, 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def r64(v):
    with np.errstate(over="ignore"):
        return bf16_round(np.asarray(v, dtype=np.float64).astype(np.float32)).astype(np.float64)


def f32(v):
    return np.asarray(v, dtype=np.float32)


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - np.asarray(ref, dtype=np.float64)) / bound).max())


# ---- dropout -----------------------------------------------------------------------------------------------------------------
def _mix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h = (h * np.uint32(0x85EBCA6B)).astype(np.uint32)
    h ^= h >> np.uint32(13)
    h = (h * np.uint32(0xC2B2AE35)).astype(np.uint32)
    h ^= h >> np.uint32(16)
    return h


def drop_thresh(p):
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    return min(int(p * 4294967296.0), 0xFFFFFFFF)


def drop_scale(p):
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p > 0 else np.float32(1.0)


def keep(stream, n_rows, n_cols, p, row0=0):
    """bool [n_rows][n_cols]: lt_keep(stream, row0 + row, col) under drop probability p (all True at p = 0)."""
    th = drop_thresh(p)
    if th == 0:
        return np.ones((n_rows, n_cols), bool)
    with np.errstate(over="ignore"):
        rows = (np.arange(n_rows, dtype=np.uint32) + np.uint32(row0))[:, None]
        cols = np.arange(n_cols, dtype=np.uint32)[None, :]
        h = _mix32(_mix32(np.uint32(stream) ^ (rows * np.uint32(0x9E3779B9))) + cols * np.uint32(0x7F4A7C15))
    return h >= np.uint32(th)


def dropped(x, stream, p):
    """x' = bf16(fp32(x ds)) where kept, else 0 (float32, bf16 values)."""
    x = f32(x)
    if drop_thresh(p) == 0:
        return x
    return np.where(keep(stream, x.shape[0], x.shape[1], p), bf16_round(x * drop_scale(p)), np.float32(0))


# ---- operands ----------------------------------------------------------------------------------------------------------------
def operands(kind, seed, shape, std=1.0):
    """bf16-valued float32. random: uniform with standard deviation std. exact: integers in [-4, 4] times 2^-2, so that sums of
    thousands of pairwise products stay exact in fp32."""
    if kind == "exact":
        n = int(np.prod(shape))
        k = (splitmix64(seed, n) >> np.uint64(33)).astype(np.int64) % 9 - 4
        return (k.astype(np.float32) * np.float32(0.25)).reshape(shape)
    return bf16_round(hash_uniform(seed, shape, std))


# ---- rank-r product ----------------------------------------------------------------------------------------------------------
def skinny_ref64(x, w, scale, stream=0, p=0.0, mutant=None):
    """x [n][K], w [16 nt][K] bf16 values. Returns (out [n][16 nt], bound) float64."""
    xd = dropped(x, stream, p).astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    K = xd.shape[1]
    if mutant == "k_step_dropped":   # wave 1's first step, or the only one
        xd = xd.copy()
        xd[:, 64:128] = 0.0
        if K == 64:
            xd[:] = 0.0
    if mutant == "wrong_tile":
        w = np.roll(w, 16, axis=0) if w.shape[0] == 32 else w[::-1]
    acc = xd @ w.T
    bound = ulp(scale * acc) + K * EPS * abs(scale) * (np.abs(xd) @ np.abs(w).T) + TINY
    return r64(scale * acc), bound


def skinny_emul32(x, w, scale, stream=0, p=0.0):
    xd = dropped(x, stream, p)
    n, K = xd.shape
    prod = xd[:, None, :] * f32(w)[None, :, :]
    acc = prod.reshape(n, -1, K // 32, 32).sum(-1, dtype=np.float32)[..., ::-1].sum(-1, dtype=np.float32)
    return bf16_round(acc * np.float32(scale))


# ---- token reduction ---------------------------------------------------------------------------------------------------------
def tn_chunk(n):
    return 256 if n >= 4096 else (128 if n >= 512 else 32)


def _orig_cols(cols, hd):
    c = np.arange(cols)
    within = c % hd
    return c // hd * hd + (within & 1) * (hd // 2) + (within >> 1)


def _tn_place(G, a, r, layout, hd):
    """[r][cols] tile a -> the output it lands in, in that output's shape (None: the tile writes nothing)."""
    cols = G.shape[1]
    if layout == 0:
        return G
    if layout == 1:
        return np.ascontiguousarray(G.T)
    if layout == 2:
        out = np.empty((cols, r))
        out[_orig_cols(cols, hd)] = G.T
        return out
    c = np.arange(cols)
    mine = ((c >> 4) & 1) == a
    out = np.empty((cols // 2, r))
    out[(c[mine] >> 5) * 16 + (c[mine] & 15)] = G[:, mine].T
    return out


def tn_ref64(t, x, scale, r, layout, hd=0, stream=0, p=0.0, init=(None, None), mutant=None):
    """t: list of nj arrays [n][16] (the tiles' columns of T), x [n][cols]; init: the outputs' earlier contents (None: that output
    is not written). Returns ([out0, out1], [bound0, bound1]) float64, None where not written."""
    xd = dropped(x, stream, p).astype(np.float64)
    n, cols = xd.shape
    chunk = tn_chunk(n)
    chunks = -(-n // chunk)
    if mutant == "no_deinterleave" and layout == 2:
        layout = 1
    if mutant == "gate_up_swapped" and layout == 3:
        t = t[::-1]
    outs, bounds = [], []
    for a in range(len(t)):
        ini = init[a]
        if ini is None:
            outs.append(None)
            bounds.append(None)
            continue
        ta = np.asarray(t[a], dtype=np.float64)[:, :r]
        xa = xd
        if mutant == "last_partial_step_dropped":
            live = np.ones(n, bool)
            for t0 in range(0, n, chunk):
                t1 = min(n, t0 + chunk)
                live[t0 + (t1 - t0) // 32 * 32:t1] = False
            ta = ta * live[:, None]
        G = scale * (ta.T @ xa)
        if mutant == "tail_rows_not_zeroed" and n % 32:
            G = G + scale * (32 - n % 32) * np.outer(ta[n - 1], xa[n - 1])
        A = abs(scale) * (np.abs(ta).T @ np.abs(xa))
        G, A = _tn_place(G, a, r, layout, hd), _tn_place(A, a, r, layout, hd)
        base = np.zeros_like(G) if mutant == "assign_not_add" else np.asarray(ini, dtype=np.float64).reshape(G.shape)
        out = base + G
        outs.append(out)
        bounds.append((chunk + chunks + 2) * EPS * A + ulp32(out) + TINY)
    while len(outs) < 2:
        outs.append(None)
        bounds.append(None)
    return outs, bounds


def tn_emul32(t, x, scale, r, layout, hd=0, stream=0, p=0.0, init=(None, None)):
    """fp32: a chunk's tokens summed last to first, the chunks added to the output last to first."""
    xd = dropped(x, stream, p)
    n, cols = xd.shape
    chunk = tn_chunk(n)
    outs = []
    for a in range(len(t)):
        ini = init[a]
        if ini is None:
            outs.append(None)
            continue
        ta = f32(t[a])[:, :r]
        out = None
        for t0 in reversed(range(0, n, chunk)):
            t1 = min(n, t0 + chunk)
            part = np.zeros((r, cols), np.float32)
            for k in reversed(range(t0, t1)):
                part = part + ta[k][:, None] * xd[k][None, :]
            part = _tn_place((part * np.float32(scale)).astype(np.float64), a, r, layout, hd).astype(np.float32)
            out = (f32(ini).reshape(part.shape) if out is None else out) + part
        outs.append(out)
    while len(outs) < 2:
        outs.append(None)
    return outs


# ---- expand-add --------------------------------------------------------------------------------------------------------------
def _delta_chain(y, l, s, round_product=True):
    d = r64(l) * float(np.float32(s))
    return y + (r64(d) if round_product else d)


def expand_ref64(y, t, w, r, s, stream=0, p=0.0, mutant=None):
    """y [n][cols], t [n][16], w [16][cols] bf16 values. Returns (out, bound): the rounded chain where kept, y itself (bound 0)
    where dropped."""
    y = np.asarray(y, dtype=np.float64)
    t64, w64 = np.asarray(t, dtype=np.float64)[:, :r], np.asarray(w, dtype=np.float64)[:r]
    l = t64 @ w64
    e = r * EPS * (np.abs(t64) @ np.abs(w64))
    if mutant == "scale_missing":
        s = 1.0
    pre = _delta_chain(y, l, s, mutant != "product_not_rounded")   # the mutant differs only where s is no power of two
    out = r64(pre)
    bound = np.maximum(np.abs(r64(_delta_chain(y, l + e, s)) - out), np.abs(r64(_delta_chain(y, l - e, s)) - out)) + TINY
    k = keep(stream, y.shape[0], y.shape[1], p, row0=1 if mutant == "mask_of_next_row" else 0)
    return np.where(k, out, y), np.where(k, bound, TINY)


def expand_emul32(y, t, w, r, s, stream=0, p=0.0):
    l = np.zeros(np.shape(y), np.float32)
    for j in reversed(range(r)):
        l = l + f32(t)[:, j:j + 1] * f32(w)[j][None, :]
    d = bf16_round(bf16_round(l) * np.float32(s))
    return np.where(keep(stream, l.shape[0], l.shape[1], p), bf16_round(f32(y) + d), f32(y))


# ---- SwiGLU backward ---------------------------------------------------------------------------------------------------------
def swiglu_bwd_ref64(g, u, dy, mutant=None):
    """Element-wise on bf16 values. Returns (dg, du, bound_dg, bound_du) float64; dg / du carry the final rounding."""
    g, u, dy = (np.asarray(v, dtype=np.float64) for v in (g, u, dy))
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-g))
    F = 1.0 if mutant == "no_g_term" else 1.0 + g * (1.0 - sg)
    dg, du = dy * u * (sg * F), dy * (g * sg)
    ag = np.abs(g)
    e_s = (ag + 3) * 2.0 ** -23
    e_F = ag * (sg * e_s + 2 * EPS) + EPS * (1 + ag)
    out_of_range = g < -87.0
    bg = ulp(dg) + np.abs(dy * u) * sg * (e_F + np.abs(F) * (e_s + 3 * EPS)) + np.where(out_of_range, np.abs(dg), 0.0) + 2.0 ** -126
    bu = ulp(du) + np.abs(dy * g) * sg * (e_s + 2 * EPS) + np.where(out_of_range, np.abs(du), 0.0) + 2.0 ** -126
    if mutant == "dg_du_swapped":
        dg, du = du, dg
    return r64(dg), r64(du), bg, bu


def swiglu_bwd_emul32(g, u, dy):
    g, u, dy = f32(g), f32(u), f32(dy)
    one = np.float32(1)
    with np.errstate(over="ignore"):
        sg = one / (one + np.exp(-g.astype(np.float64)).astype(np.float32))   # another exponential than the kernel's
    return bf16_round(dy * u * (sg * (one + g * (one - sg)))), bf16_round(dy * (g * sg))


def swiglu_data(n, f, seed=0):
    """gate / up / dh [n][f]: random values with the corners in the first columns of every row -- g at the bf16 neighbours of
    -1.2785 (where 1 + g (1 - sg) cancels), |g| > 100, exact zeros."""
    g = operands("random", 11 + seed, (n, f), 2.0)
    u = operands("random", 12 + seed, (n, f), 1.0)
    dy = operands("random", 13 + seed, (n, f), 1.0)
    corners = bf16_round(np.array([-1.2785, -1.2734375, -1.28125, 104.0, -104.0, 0.0, -88.0, 20.0, -20.0, 300.0, -300.0, 1.0],
                                  np.float32))
    k = min(f, len(corners))
    g[:, :k] = corners[:k]
    if f > 13:
        u[:, 13] = 0.0
        dy[:, 12] = 0.0
    return g, u, dy


def interleave_gu(g, u):
    """[n][f] gate and up -> the packed wgu GEMM's [n][2f] layout: 16 gate columns, 16 up columns, ..."""
    n, f = g.shape
    out = np.empty((n, f // 16, 2, 16), np.float32)
    out[:, :, 0], out[:, :, 1] = g.reshape(n, -1, 16), u.reshape(n, -1, 16)
    return out.reshape(n, 2 * f)


def deinterleave_gu(gu):
    n, f2 = gu.shape
    v = gu.reshape(n, f2 // 32, 2, 16)
    return v[:, :, 0].reshape(n, -1), v[:, :, 1].reshape(n, -1)


# ---- RMSNorm backward --------------------------------------------------------------------------------------------------------
def rmsnorm_bwd_ref64(dy, x, w, eps, res=None, lora=None, mutant=None):
    """dy, x, res [rows][d], w [d] bf16 values. lora: dict(dt [rows][32], a_cat [32][d], r, stream, p) or None.
    Returns (out, bound) float64 [rows][d] (out carries the kernel's roundings)."""
    dy, x, w = (np.asarray(v, dtype=np.float64) for v in (dy, x, w))
    rows, d = x.shape
    D = np.zeros_like(dy)
    if lora is not None:
        r, ds = lora["r"], float(drop_scale(lora["p"]))
        idx = np.r_[0:r, 16:16 + r]
        t64, a64 = np.asarray(lora["dt"], dtype=np.float64)[:, idx], np.asarray(lora["a_cat"], dtype=np.float64)[idx]
        l = t64 @ a64
        e = (2 * r + 1) * EPS * (np.abs(t64) @ np.abs(a64))
        k = keep(lora["stream"], rows, d, lora["p"], row0=1 if mutant == "mask_of_next_row" else 0)

        def chain(l_):
            return np.where(k, r64(dy + r64(l_ * ds)), dy)

        dy, lo, hi = chain(l), chain(l - e), chain(l + e)
        D = np.maximum(np.abs(lo - dy), np.abs(hi - dy))
    g = w * dy
    dn = float(2048 * -(-d // 2048)) if mutant == "mean_over_chunks" else float(d)
    rstd = 1.0 / np.sqrt((x * x).sum(-1, keepdims=True) / dn + eps)
    sxg = (x * g).sum(-1, keepdims=True)
    coef = 0.0 * sxg if mutant == "coef_missing" else sxg / dn * rstd ** 3
    dx = rstd * g - x * coef
    e_r = (d / 2 + 5) * EPS
    E = (np.abs(rstd * g) * (e_r + 3 * EPS) + np.abs(x) * rstd ** 3 * (d + 1) * EPS * np.abs(x * g).sum(-1, keepdims=True) / d
         + np.abs(x * coef) * (3 * e_r + 6 * EPS)
         + rstd * np.abs(w) * D + np.abs(x) * rstd ** 3 * (np.abs(x * w) * D).sum(-1, keepdims=True) / d)
    if res is None:
        return r64(dx), ulp(dx) + E + TINY
    res = np.asarray(res, dtype=np.float64)

    def rchain(v):
        return r64(v + res) if mutant == "res_before_rounding" else r64(r64(v) + res)

    out = rchain(dx)
    return out, np.maximum(np.abs(rchain(dx + E) - out), np.abs(rchain(dx - E) - out)) + TINY


def rmsnorm_bwd_emul32(dy, x, w, eps, res=None, lora=None):
    dy, x, w = f32(dy), f32(x), f32(w)
    rows, d = x.shape
    if lora is not None:
        r = lora["r"]
        l = np.zeros((rows, d), np.float32)
        for j in reversed(range(r)):
            l = l + f32(lora["dt"])[:, 16 + j:17 + j] * f32(lora["a_cat"])[16 + j][None] + f32(lora["dt"])[:, j:j + 1] * f32(lora["a_cat"])[j][None]
        k = keep(lora["stream"], rows, d, lora["p"])
        dy = np.where(k, bf16_round(dy + bf16_round(l * drop_scale(lora["p"]))), dy)
    g = dy * w
    s2 = (x * x)[:, ::-1].sum(-1, dtype=np.float32, keepdims=True)
    dot = (x * g)[:, ::-1].sum(-1, dtype=np.float32, keepdims=True)
    rstd = np.float32(1) / np.sqrt(s2 / np.float32(d) + np.float32(eps))
    coef = dot / np.float32(d) * rstd * rstd * rstd
    v = rstd * g - x * coef
    if res is not None:
        v = bf16_round(v) + f32(res)
    return bf16_round(v)


# ---- cross-entropy -----------------------------------------------------------------------------------------------------------
def ce_ref64(logits, targets, gscale, mutant=None):
    """logits [m][V] bf16 values, targets [m] any int. Returns dict: grad, grad_bound [m][V]; out, out_bound [3]; losses [m]."""
    x = np.asarray(logits, dtype=np.float64)
    m, V = x.shape
    tg = np.asarray(targets, dtype=np.int64)
    live = (tg >= 0) & (tg < V)
    mx = x.max(-1, keepdims=True)
    t = x - mx
    ex = np.exp(t)
    se = ex.sum(-1, keepdims=True)
    p = ex / se
    onehot = np.zeros_like(x)
    onehot[np.nonzero(live)[0], tg[live]] = 1.0
    gs = 1.0 if mutant == "gscale_missing" else float(np.float32(gscale))
    pre = (p - (0.0 if mutant == "no_onehot" else onehot)) * gs
    e_j = (np.abs(t) + 2) * 2.0 ** -23
    e_se = (V / 256 + 10) * EPS + (p * e_j).sum(-1, keepdims=True)
    e_p = e_j + e_se + 3 * EPS
    gb = ulp(pre) + abs(gs) * (p * e_p + 2 * EPS * np.abs(p - onehot) + np.where(t < -86.0, p, 0.0)) + TINY
    grad = np.where(live[:, None], r64(pre), 0.0)
    gb = np.where(live[:, None], gb, TINY)
    lse = np.log(se[:, 0])
    picked = x[np.arange(m), np.where(live, tg, 0)]
    loss = np.where(live, lse + mx[:, 0] - picked, 0.0)
    e_loss = np.where(live, e_se[:, 0] + 2.0 ** -22 * np.abs(lse) + EPS + EPS * (np.abs(lse + mx[:, 0]) + np.abs(loss)), 0.0)
    denom = max(int(live.sum()), 1) if mutant == "mean_over_live_rows" else m
    out = np.array([loss.sum() / denom, float(m), float((~live).sum())])
    ob = np.array([(e_loss.sum() + (m + 2) * EPS * np.abs(loss).sum()) / m + TINY, TINY, TINY])
    return dict(grad=grad, grad_bound=gb, out=out, out_bound=ob, losses=loss)


def ce_emul32(logits, targets, gscale):
    x = f32(logits)
    m, V = x.shape
    tg = np.asarray(targets, dtype=np.int64)
    live = (tg >= 0) & (tg < V)
    mx = x.max(-1, keepdims=True)
    ex = np.exp((x - mx).astype(np.float64)).astype(np.float32)
    se = ex[:, ::-1].sum(-1, dtype=np.float32, keepdims=True)
    p = ex * (np.float32(1) / se)
    onehot = np.zeros_like(x)
    onehot[np.nonzero(live)[0], tg[live]] = 1.0
    grad = np.where(live[:, None], bf16_round((p - onehot) * np.float32(gscale)), np.float32(0))
    picked = x[np.arange(m), np.where(live, tg, 0)]
    loss = np.where(live, np.log(se[:, 0]) + mx[:, 0] - picked, np.float32(0)).astype(np.float32)
    tot = np.float32(0)
    for v in loss[::-1]:
        tot = np.float32(tot + v)
    return grad, np.array([tot / np.float32(m), np.float32(m), np.float32((~live).sum())], np.float32)


def ce_data(regime, m, V, seed=0):
    """(logits [m][V] bf16 values, targets [m] int32): every regime mixes live rows with targets 0, V - 1 and the three kinds of
    "no token id" (-100, V, 10^6) once m allows."""
    x = operands("random", 31 + seed, (m, V), 2.0)
    tg = (splitmix64(41 + seed, m) % np.uint64(V)).astype(np.int64)
    special = [0, V - 1, -100, V, 10 ** 6]
    for i, s in enumerate(special):
        if 1 + 2 * i < m:
            tg[1 + 2 * i] = s
    if regime == "spike":
        x[np.arange(m), (tg.clip(0, V - 1) + 1) % V] += np.float32(60.0)
    elif regime == "equal":
        x[:] = np.float32(0.75)
    elif regime == "shifted":
        x = x - np.float32(3e4)
    elif regime == "rare_target":
        x[np.arange(m), tg.clip(0, V - 1)] = np.float32(-80.0) if V > 1 else x[:, 0]
        x[np.arange(m), (tg.clip(0, V - 1) + 1) % V] = np.float32(0.0)
        x = np.minimum(x, np.float32(0.0)) if V > 2 else x
    return bf16_round(x), tg.astype(np.int32)


# ---- rowdot ------------------------------------------------------------------------------------------------------------------
def rowdot_ref64(o, d_o, mutant=None):
    """o, d_o [items][hd]. Returns (out [items], bound)."""
    o, d_o = np.asarray(o, dtype=np.float64), np.asarray(d_o, dtype=np.float64)
    hd = o.shape[1]
    A = (np.abs(o) * np.abs(d_o)).sum(-1)
    if mutant == "second_step_missing":
        o = o[:, :128]
        d_o = d_o[:, :128]
    return (o * d_o).sum(-1), hd * EPS * A + TINY


def rowdot_emul32(o, d_o):
    return (f32(o) * f32(d_o))[:, ::-1].sum(-1, dtype=np.float32)


# ---- AdamW -------------------------------------------------------------------------------------------------------------------
def adamw_ref64(p, g, m, v, step, lr, limit, beta1, beta2, eps, wd, mutant=None):
    """One clip + AdamW step at optimizer step `step` (>= 1) on flat fp32 arrays, hyper-parameters at their fp32 values.
    Returns dict p, m, v, norm and their bounds."""
    from oracle.llama_train_oracle import clip_and_adamw

    lr, limit, b1, b2, eps, wd = (float(np.float32(h)) for h in (lr, limit, beta1, beta2, eps, wd))
    p0, g64, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    n = p0.size
    P, M, V = {"w": p0.copy()}, {"w": m0.copy()}, {"w": v0.copy()}
    norm = clip_and_adamw(P, {"w": g64}, M, V, step - 1 if mutant == "bias_step_minus_one" else step, lr,
                          -1.0 if mutant == "no_clip" else limit, b1, b2, eps, wd)
    pn, mn, vn = P["w"], M["w"], V["w"]
    blocks = min(1024, -(-n // 256))
    e_ss = (n / (256.0 * blocks) + blocks + 32) * EPS
    e_n = e_ss / 2 + EPS
    active = limit > 0 and limit / (norm + 1e-6) < 1.0 + 1e-3
    coef = min(1.0, limit / (norm + 1e-6)) if limit > 0 else 1.0
    e_g = (e_n + 3 * EPS if active else 0.0) + EPS
    gi = g64 * coef
    E_m = EPS * np.abs(b1 * m0) + np.abs((1 - b1) * gi) * (e_g + EPS) + EPS * np.abs(mn)
    E_v = EPS * np.abs(b2 * v0) + (1 - b2) * gi * gi * (2 * e_g + 2 * EPS) + EPS * vn

    def bc(b):
        pw = b ** step
        val = 1.0 - pw
        return val, ((abs(step * np.log2(b)) + 1) * 2.0 ** -22 * pw + EPS * val) / val

    bc1, r1 = bc(b1)
    bc2, r2 = bc(b2)
    den = np.sqrt(vn) / np.sqrt(bc2) + eps
    upd = (lr / bc1) * mn / den
    rel_den = np.where(vn > 0, E_v / (2 * np.maximum(vn, 1e-300)), 0.0) + r2 / 2 + 4 * EPS
    E_upd = np.abs(upd) * (r1 + 4 * EPS + rel_den) + (lr / bc1) * E_m / den
    E_p = 3 * EPS * np.abs(p0) + E_upd + EPS * np.abs(pn) + TINY
    return dict(p=pn, m=mn, v=vn, norm=norm, p_bound=E_p, m_bound=E_m + TINY, v_bound=E_v + TINY,
                norm_bound=e_n * norm + ulp32(norm) + TINY)


def adamw_emul32(p, g, m, v, step, lr, limit, beta1, beta2, eps, wd):
    p, g, m, v = f32(p), f32(g), f32(m), f32(v)
    lr, limit, b1, b2, eps, wd = (np.float32(h) for h in (lr, limit, beta1, beta2, eps, wd))
    one = np.float32(1)
    norm = np.sqrt((g * g)[::-1].sum(dtype=np.float32))
    coef = min(one, limit / (norm + np.float32(1e-6))) if limit > 0 else one
    bc1 = one - np.float32(float(b1) ** step)
    bc2 = one - np.float32(float(b2) ** step)
    gi = g * coef
    pi = p * (one - lr * wd)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    pi = pi - (lr / bc1) * mi / (np.sqrt(vi) / np.sqrt(bc2) + eps)
    return pi.astype(np.float32), mi.astype(np.float32), vi.astype(np.float32), np.float32(norm)


def adamw_data(n, seed=0):
    p = hash_uniform(51 + seed, (n,), 0.05)
    g = hash_uniform(52 + seed, (n,), 0.02)
    m = hash_uniform(53 + seed, (n,), 0.01)
    v = np.abs(hash_uniform(54 + seed, (n,), 1e-4))
    if n > 2:
        g[2], m[2], v[2] = 0.0, 0.0, 0.0    # the update's 0 / (0 + eps) corner
    return p, g, m, v


# ---- forward sweep: adapters' delta, q / k norm, rotation ---------------------------------------------------------------------
def _delta(t, w, r, s):
    t64, w64 = np.asarray(t, dtype=np.float64)[:, :r], np.asarray(w, dtype=np.float64)[:r]
    return r64(r64(t64 @ w64) * float(np.float32(s)))


def _chain_delta(y, t, w, r, s):
    """(x', D): x' = bf16(y + bf16(bf16(l) s)), and how far x' moves when l is off by its fp32 error r eps sum|t||w|."""
    y = np.asarray(y, dtype=np.float64)
    t64, w64 = np.asarray(t, dtype=np.float64)[:, :r], np.asarray(w, dtype=np.float64)[:r]
    l = t64 @ w64
    e = r * EPS * (np.abs(t64) @ np.abs(w64))
    out = r64(_delta_chain(y, l, s))
    return out, np.maximum(np.abs(r64(_delta_chain(y, l + e, s)) - out), np.abs(r64(_delta_chain(y, l - e, s)) - out))


def rope_fwd_ref64(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk=None, bk_t=None, norm=None, mutant=None):
    """qkv [n][(nq + 2 nk) hd] bf16 values, packed heads; t [n][32]; tk [n][16] / bk_t [16][nk hd] or None; norm: dict(wq, wk, eps)
    or None; cos / sin [positions][hd / 2] as the kernel reads them. Returns (out, bound, xsave, xsave_bound): out / bound
    [n][qw] float64 (q | k unrounded after the rotation, as tests/qwen3_ref.py's sweep_ref64 returns them -- this is that
    restatement and its bound behind the delta chain), xsave the pre-norm q | k (None without a norm).
    A move D of x' (see _chain_delta; zero for nearly every element) is carried through the norm as
    |w| (rstd D + |x| rstd^3 sum(|x| D) / hd) and through the rotation as |c| D_a + |s| D_b."""
    from tests import qwen3_ref as QR

    x = np.asarray(qkv, dtype=np.float64)
    n = x.shape[0]
    qc, kc = nq * hd, nk * hd
    q0, k0, v0 = x[:, :qc], x[:, qc:qc + kc], x[:, qc + kc:]
    tq, tv = np.asarray(t)[:, :16], np.asarray(t)[:, 16:32]
    v1, Dv = _chain_delta(v0, tv, bv_t, r, s)
    eps = norm["eps"] if norm else 0.0
    wq, wk = (norm["wq"], norm["wk"]) if norm else (None, None)
    if mutant == "delta_after_rotation":
        rot, _ = QR.sweep_ref64(x[:, :qc + kc], pos, cos, sin, nq, nk, hd, wq, wk, eps, mutant=None if norm else "no_norm")
        rot = r64(rot)
        rot[:, :qc] = r64(rot[:, :qc] + _delta(tq, bq_t, r, s))
        if bk_t is not None:
            rot[:, qc:] = r64(rot[:, qc:] + _delta(tk, bk_t, r, s))
        return np.concatenate([rot, v1], 1), None, None, None
    if mutant == "norm_before_delta":
        xh = x[:, :qc + kc].reshape(n, nq + nk, hd)
        w = QR._weights(nq, nk, hd, wq, wk, None)[None]
        y = r64(w * r64(xh * (1.0 / np.sqrt((xh * xh).mean(-1, keepdims=True) + eps)))).reshape(n, -1)
        y[:, :qc] = r64(y[:, :qc] + _delta(tq, bq_t, r, s))
        if bk_t is not None:
            y[:, qc:] = r64(y[:, qc:] + _delta(tk, bk_t, r, s))
        rot, _ = QR.sweep_ref64(y, pos, cos, sin, nq, nk, hd, None, None, 0.0, mutant="no_norm")
        return np.concatenate([rot, v1], 1), None, None, None
    q1, Dq = _chain_delta(q0, tq, bq_t, r, s)
    k1, Dk = _chain_delta(k0, tk, bk_t, r, s) if bk_t is not None else (k0, np.zeros_like(k0))
    xqk, D = np.concatenate([q1, k1], 1), np.concatenate([Dq, Dk], 1).reshape(n, nq + nk, hd)
    out, bound = QR.sweep_ref64(xqk, pos, cos, sin, nq, nk, hd, wq, wk, eps, mutant=None if norm else "no_norm")
    if norm:
        xh = xqk.reshape(n, nq + nk, hd)
        w = np.abs(QR._weights(nq, nk, hd, wq, wk, None))[None]
        rstd = 1.0 / np.sqrt((xh * xh).mean(-1, keepdims=True) + eps)
        D = w * (rstd * D + np.abs(xh) * rstd ** 3 * (np.abs(xh) * D).sum(-1, keepdims=True) / hd)
    p = np.asarray(pos, dtype=np.int64)
    c, sn = np.abs(np.asarray(cos, dtype=np.float64))[p][:, None, :], np.abs(np.asarray(sin, dtype=np.float64))[p][:, None, :]
    extra = np.empty_like(D)
    extra[..., 0::2], extra[..., 1::2] = c * D[..., 0::2] + sn * D[..., 1::2], c * D[..., 1::2] + sn * D[..., 0::2]
    bound = bound + extra.reshape(n, -1)
    xs = (xqk, np.concatenate([Dq, Dk], 1) + TINY) if norm else (None, None)
    return np.concatenate([out, v1], 1), np.concatenate([bound, Dv + TINY], 1), xs[0], xs[1]


def _delta_emul32(y, t, w, r, s):
    l = np.zeros(np.shape(y), np.float32)
    for j in reversed(range(r)):
        l = l + f32(t)[:, j:j + 1] * f32(w)[j][None, :]
    return bf16_round(f32(y) + bf16_round(bf16_round(l) * np.float32(s)))


def rope_fwd_emul32(qkv, nq, nk, hd, t, bq_t, bv_t, r, s, pos, cos, sin, tk=None, bk_t=None, norm=None):
    x = f32(qkv)
    n = x.shape[0]
    qc, kc = nq * hd, nk * hd
    q = _delta_emul32(x[:, :qc], f32(t)[:, :16], bq_t, r, s)
    k = _delta_emul32(x[:, qc:qc + kc], tk, bk_t, r, s) if bk_t is not None else x[:, qc:qc + kc]
    v = _delta_emul32(x[:, qc + kc:], f32(t)[:, 16:32], bv_t, r, s)
    xh = np.concatenate([q, k], 1).reshape(n, nq + nk, hd)
    xsave = xh.reshape(n, -1).copy()
    if norm:
        from tests import qwen3_ref as QR

        w = QR._weights(nq, nk, hd, norm["wq"], norm["wk"], None)[None].astype(np.float32)
        ss = (xh * xh)[..., ::-1].sum(-1, dtype=np.float32, keepdims=True)
        rstd = np.float32(1) / np.sqrt(ss / np.float32(hd) + np.float32(norm["eps"]))
        xh = bf16_round(w * bf16_round(xh * rstd))
    p = np.asarray(pos, dtype=np.int64)
    c, sn = f32(cos)[p][:, None, :], f32(sin)[p][:, None, :]
    a, b = xh[..., 0::2], xh[..., 1::2]
    out = np.empty_like(xh)
    out[..., 0::2], out[..., 1::2] = a * c - b * sn, b * c + a * sn
    return np.concatenate([bf16_round(out).reshape(n, -1), v], 1), (xsave if norm else None)


# ---- rotation backward -------------------------------------------------------------------------------------------------------
def rope_bwd_ref64(x, heads, hd, pos, cos, sin, mutant=None):
    """x [n][heads hd] bf16 values. The transposed rotation a c + b s, b c - a s: two fp32 products and a sum (3 eps of |a c| +
    |b s|, bounded by 2^-22) and one rounding. Returns (out unrounded, bound)."""
    from tests import stage2_ref as R

    n = x.shape[0]
    xh = np.asarray(x, dtype=np.float64).reshape(n, heads, hd)
    out = R.rope_rotate64(xh, pos, cos, sin, transpose=mutant != "forward_rotation")
    p = np.asarray(pos, dtype=np.int64)
    c, s = np.abs(np.asarray(cos, dtype=np.float64))[p][:, None, :], np.abs(np.asarray(sin, dtype=np.float64))[p][:, None, :]
    a, b = np.abs(xh[..., 0::2]), np.abs(xh[..., 1::2])
    bound = np.empty_like(out)
    bound[..., 0::2], bound[..., 1::2] = 2.0 ** -22 * (a * c + b * s), 2.0 ** -22 * (b * c + a * s)
    return out.reshape(n, -1), (bound + ulp(out)).reshape(n, -1) + TINY


def rope_bwd_emul32(x, heads, hd, pos, cos, sin):
    """The kernel's own operations (nothing to reorder): the kernel must return these bits."""
    n = x.shape[0]
    xh = f32(x).reshape(n, heads, hd)
    p = np.asarray(pos, dtype=np.int64)
    c, s = f32(cos)[p][:, None, :], f32(sin)[p][:, None, :]
    a, b = xh[..., 0::2], xh[..., 1::2]
    out = np.empty_like(xh)
    out[..., 0::2], out[..., 1::2] = a * c + b * s, b * c - a * s
    return bf16_round(out).reshape(n, -1)


# ---- SwiGLU with the gate / up adapters --------------------------------------------------------------------------------------
def swiglu_lora_ref64(g, u, t, w, r, s, mutant=None):
    """g, u [n][f] bf16 values, t [n][32] (16 gate ranks, 16 up ranks), w [32][2f] in the interleaved column order. Returns
    (g', u', Dg, Du): the summed gate / up the kernel writes back and how far each may move (see _chain_delta). h is judged by
    tests/test_gpu_stage2_bounds.py's gated_ratio on (g', u') with those moves as the accumulators' uncertainty."""
    wg, _ = deinterleave_gu(f32(w)[:16])
    _, wu = deinterleave_gu(f32(w)[16:32])
    tg, tu = np.asarray(t)[:, :16], np.asarray(t)[:, 16:32]
    if mutant == "gate_up_ranks_swapped":
        tg, tu = tu, tg
    g1, Dg = _chain_delta(g, tg, wg, r, s)
    u1, Du = _chain_delta(u, tu, wu, r, s)
    return g1, u1, Dg, Du


def swiglu_lora_emul32(g, u, t, w, r, s):
    wg, _ = deinterleave_gu(f32(w)[:16])
    _, wu = deinterleave_gu(f32(w)[16:32])
    g1, u1 = _delta_emul32(g, f32(t)[:, :16], wg, r, s), _delta_emul32(u, f32(t)[:, 16:32], wu, r, s)
    with np.errstate(over="ignore"):
        a = bf16_round((g1.astype(np.float64) / (1.0 + np.exp(-g1.astype(np.float64)))).astype(np.float32))
    return g1, u1, bf16_round(a * u1)


# ---- working copies (bit-exact) ----------------------------------------------------------------------------------------------
def prep_lora_ref(aq, bq, av, bv, r, hd):
    """fp32 masters (A [r][d], B [cols][r]) -> (a_cat [32][d], bq_t [16][qcols], bv_t [16][vcols]) bf16 values."""
    d, qcols, vcols = aq.shape[1], bq.shape[0], bv.shape[0]
    a_cat, bq_t, bv_t = np.zeros((32, d), np.float32), np.zeros((16, qcols), np.float32), np.zeros((16, vcols), np.float32)
    a_cat[:r], a_cat[16:16 + r] = bf16_round(aq), bf16_round(av)
    bq_t[:r] = bf16_round(bq)[_orig_cols(qcols, hd)].T
    bv_t[:r] = bf16_round(bv).T
    return a_cat, bq_t, bv_t


def prep_module_ref(a, b, r, perm, hd, b_t_before):
    """(a_w [16][in], b_t [16][ldb]): b_t starts as b_t_before and only the columns the permutation names are written."""
    out = b.shape[0]
    a_w = np.zeros((16, a.shape[1]), np.float32)
    a_w[:r] = bf16_round(a)
    b_t = np.array(b_t_before, dtype=np.float32)
    c = np.arange(out)
    orig = _orig_cols(out, hd) if perm == 1 else c
    dest = (c >> 4) * 32 + (16 if perm == 3 else 0) + (c & 15) if perm >= 2 else c
    b_t[:, dest] = 0.0
    b_t[:r, dest] = bf16_round(b)[orig].T
    return a_w, b_t


# ---- the cases both test files run: the smallest shapes that reach every arm of every launcher ---------------------------------
STREAM = 0x9E3779B1     # any 32-bit value is a stream


def covered(cases, rotated, against=()):
    """What the case lists below promise, as a list of the promises they break (empty: kept): every value of every rotated
    parameter occurs; with every value of every other rotated parameter; and with every value of each parameter named in
    `against`. rotated: {name: values}. tests/test_lora_kernels_host.py asserts it for every list and every operand kind."""
    cases, missing = list(cases), []
    for name, values in rotated.items():
        others = [(o, v) for o, v in rotated.items() if o != name] + [(o, sorted({c[o] for c in cases}, key=str)) for o in against]
        for val in values:
            mine = [c for c in cases if c[name] == val]
            if not mine:
                missing.append((name, val))
            for o, ovals in others:
                missing += [(name, val, o, ov) for ov in ovals if not any(c[o] == ov for c in mine)]
    return missing


def _drop(kind, on):
    """the rotated dropout probability: 0.3 as the step uses it; 0.5 on exact operands, where ds = 2 keeps x ds exact"""
    return (0.5 if kind == "exact" else 0.3) if on else 0.0


SKINNY_NS = (1, 15, 16, 17, 67)            # one row, a part-full / full / just-over-full 16-row workgroup, several
SKINNY_KS = (64, 192, 256, 320, 1088)      # one step (three idle waves), 3, 4, 5 and 17 steps (uneven wave loads)
SKINNY_ROTATED = dict(nt=(1, 2), ocol=(0, 16), scale=(1.0, 4.0), drop=(False, True))


def skinny_cases():
    """Every (n, K) pair once per operand kind, both kinds with the same arguments. The other arguments rotate on the pair's
    indices a, b (never on the kind), so that each value meets each n, each K, each kind and each value of the others."""
    for a, n in enumerate(SKINNY_NS):
        for b, K in enumerate(SKINNY_KS):
            for kind in ("random", "exact"):
                drop = bool(((a + b) // 2) % 2)
                yield dict(kind=kind, n=n, K=K, nt=1 + (a + b) % 2, ocol=16 * ((a + b // 2) % 2), scale=(1.0, 4.0)[(b + a // 2) % 2],
                           drop=drop, p=_drop(kind, drop), seed=2 * (5 * a + b) + (kind == "exact"))


def skinny_data(c):
    return operands(c["kind"], 100 + c["seed"], (c["n"], c["K"])), operands(c["kind"], 200 + c["seed"], (16 * c["nt"], c["K"]))


TN_CONFIGS = {   # name: (layout, nj, cols, r, hd, which outputs exist)
    "dA": (0, 2, 320, 8, 0, (True, True)),
    "dA1": (0, 1, 64, 16, 0, (True, False)),
    "dBv": (1, 1, 64, 13, 0, (True, False)),
    "dBq64": (2, 1, 192, 4, 64, (True, False)),
    "dBq96": (2, 1, 192, 16, 96, (True, False)),
    "dBq128": (2, 1, 256, 1, 128, (True, False)),
    "gu": (3, 2, 192, 8, 0, (True, True)),
    "gu_gate_frozen": (3, 2, 64, 4, 0, (False, True)),
    "gu_up_frozen": (3, 2, 320, 13, 0, (True, False)),
}
TN_NS = (1, 31, 32, 33, 100, 511, 512, 600, 4136)   # around one 32-token step, the 511 / 512 and the 4095 / 4096 chunk policies


TN_SCALES = {"random": (1.0, 0.25), "exact": (0.5, 2.0)}
TN_ROTATED = dict(si=(0, 1), drop=(False, True), gather=("tcol", "ldx"))


def tn_cases():
    """Every n with every configuration (the 256-token chunk policy of n = 4136 included), once per operand kind. The scale
    (TN_SCALES[kind][si]), the dropout and the way the GPU test selects the gather kernel (a t column offset of 4 or a row stride
    of cols + 4) are the three low bits of a + b, n's index plus the configuration's: nine consecutive values along either, so
    each combination of the three meets each n, each configuration and each kind."""
    for a, n in enumerate(TN_NS):
        for b, name in enumerate(TN_CONFIGS):
            for kind in ("random", "exact"):
                si, drop = (a + b) % 2, bool(((a + b) // 2) % 2)
                yield dict(kind=kind, n=n, config=name, si=si, scale=TN_SCALES[kind][si], drop=drop, p=_drop(kind, drop),
                           gather=("tcol", "ldx")[((a + b) // 4) % 2], seed=2 * (9 * a + b) + (kind == "exact"))


def tn_data(c):
    """(t tiles list of [n][16], x [n][cols], init pair) for a token-reduction case. Columns >= r of t are nonzero on purpose:
    the kernel must not let them reach an output."""
    layout, nj, cols, r, hd, have = TN_CONFIGS[c["config"]]
    n, kind = c["n"], c["kind"]
    t = [operands(kind, 300 + 7 * c["seed"] + a, (n, 16)) for a in range(nj)]
    x = operands(kind, 400 + c["seed"], (n, cols))
    E = r * cols // (2 if layout == 3 else 1)
    init = tuple(operands(kind, 500 + 3 * c["seed"] + a, (E,), 0.5) if have[a] else None for a in range(2))
    return t, x, init


EXPAND_NS = (1, 3, 4, 5, 9)
EXPAND_COLS = (8, 64, 2048, 2056, 4104)
EXPAND_SCALES = {"random": (4.0, 1.4285714), "exact": (4.0, 0.5)}    # 1.4285714 = 1 / (1 - 0.3), the backward's; exact: powers of two
EXPAND_ROTATED = dict(r=(1, 8, 16), tcol=(0, 16), drop=(False, True), si=(0, 1))


def expand_cases():
    """Every (n, cols) pair once per operand kind; r, tcol, the dropout and the scale (EXPAND_SCALES[kind][si]) rotate on the
    pair's indices, never on the kind."""
    for a, n in enumerate(EXPAND_NS):
        for b, cols in enumerate(EXPAND_COLS):
            for kind in ("random", "exact"):
                si, drop = (a + b // 2) % 2, bool(((a + b) // 2) % 2)
                yield dict(kind=kind, n=n, cols=cols, r=(1, 8, 16)[(a + b) % 3], tcol=16 * ((b + a // 2) % 2), drop=drop,
                           p=0.3 if drop else 0.0, si=si, s=EXPAND_SCALES[kind][si], seed=2 * (5 * a + b) + (kind == "exact"))


def expand_data(c):
    kind = c["kind"]
    return (operands(kind, 600 + c["seed"], (c["n"], c["cols"])), operands(kind, 700 + c["seed"], (c["n"], 16)),
            operands(kind, 800 + c["seed"], (16, c["cols"]), 0.25))


NORM_DS = (8, 64, 2048, 2056, 3072, 4096, 4104, 8192)   # 1, 2 and 4 chunks of 2048 columns, full and part-full last chunks
NORM_ROWS = (1, 2, 3, 4, 5, 7)                           # ragged against the 1-, 2- and 4-row workgroups


NORM_ROTATED = dict(r=(4, 8, 16), ldt=(32, 48), p=(0.0, 0.3))    # of the LoRA arm; the other arm ignores them


def rmsnorm_cases():
    """Every (d, rows) pair in four combinations: plain; res + out_rows; LoRA + res; LoRA + out_rows. In the LoRA arm r, ldt and p
    rotate on the indices a of d, b of rows and k of the combination so that one d sees all twelve (r, ldt, p) and every value
    meets every rows count and both combinations."""
    i = 0
    for a, d in enumerate(NORM_DS):
        for b, rows in enumerate(NORM_ROWS):
            for k, (lora, res, gather) in enumerate(((False, False, False), (False, True, True), (True, True, False), (True, False, True))):
                rot = dict(r=(4, 8, 16)[(a + b + k) % 3], ldt=(32, 48)[(b // 3 + a) % 2], p=(0.0, 0.3)[(k + a // 2) % 2]) if lora \
                    else dict(r=8, ldt=32, p=0.0)
                yield dict(d=d, rows=rows, lora=lora, res=res, out_rows=gather, seed=i, **rot)
                i += 1


def rmsnorm_data(c):
    rows, d, s = c["rows"], c["d"], c["seed"]
    x = operands("random", 1000 + s, (rows, d), 1.5)
    dy = bf16_round(hash_uniform(900 + s, (rows, d), 0.5) + np.float32(0.25) * x)   # correlated with x: the mean term counts
    w = bf16_round(1.0 + hash_uniform(1100 + s, (d,), 0.2))
    res = operands("random", 1200 + s, (rows, d), 0.5) if c["res"] else None
    lora = None
    if c["lora"]:
        dt = operands("random", 1300 + s, (rows, 32), 0.5)     # columns >= r of each half nonzero: they must not count
        lora = dict(dt=dt, a_cat=operands("random", 1400 + s, (32, d), 0.2), r=c["r"], stream=STREAM + s, p=c["p"])
    perm = None
    if c["out_rows"]:
        perm = (np.argsort(splitmix64(1500 + s, rows + 3))[:rows]).astype(np.int32)   # distinct rows of a rows + 3 buffer
    return dy, x, w, res, lora, perm


CE_VS = (7, 255, 256, 257, 320, 32064)
CE_MS = (1, 3, 40)
CE_REGIMES = ("flat", "spike", "equal", "shifted", "rare_target")
CE_GSCALE = 0.375


def ce_cases():
    for V in CE_VS:
        for m in CE_MS:
            for regime in CE_REGIMES:
                yield dict(V=V, m=m, regime=regime, seed=V + m)


ROWDOT_HDS = (8, 16, 64, 96, 128, 256)
ROWDOT_ITEMS = (1, 15, 16, 17, 67)


def rowdot_cases():
    for hd in ROWDOT_HDS:
        for items in ROWDOT_ITEMS:
            for kind in ("random", "exact"):
                yield dict(kind=kind, hd=hd, items=items, seed=hd + items)


def rowdot_data(c):
    return operands(c["kind"], 1600 + c["seed"], (c["items"], c["hd"])), operands(c["kind"], 1700 + c["seed"], (c["items"], c["hd"]))


SWIGLU_NS = (1, 4, 5)
SWIGLU_FS = (16, 48, 2064, 11008)

ADAMW_NS = (1, 3, 6, 255, 257, 262147)     # 262 147 > 1024 blocks of 256: the grid-stride loop; 1, 6, 3 mod 4 for the ordered norm
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def adamw_cases():
    i = 0
    for n in ADAMW_NS:
        for step in (1, 2, 1000):
            for clip in ("noop", "active", "off"):
                yield dict(n=n, step=step, clip=clip, wd=(0.0, 0.01)[i % 2], seed=i)
                i += 1


def adamw_limit(c, g):
    norm = float(np.sqrt((np.asarray(g, dtype=np.float64) ** 2).sum()))
    return {"noop": 4.0 * norm + 1.0, "active": 0.25 * norm, "off": 0.0}[c["clip"]]


ROPE_SHAPES = ((4, 2, 64), (2, 2, 96), (16, 8, 128), (4, 1, 256))   # (16, 8, 128): 4096 q columns, two column steps of the sweep
ROPE_NS = (1, 3, 4, 5, 9)                                            # ragged against the sweep's 4-row workgroups
ROPE_T = 512


def rope_positions(n):
    pos = ((np.arange(n, dtype=np.int64) * 2654435761) % ROPE_T).astype(np.int32)
    pos[0] = ROPE_T - 1
    return pos


ROPE_ROTATED = dict(r=(4, 8, 16), s=(4.0, 2.0, 1.4285714), kind=("random", "exact"))


def rope_fwd_cases():
    """Every head shape, n and instantiation (inst = 2 hask + norm). r, the scaling and the adapters' operand kind rotate on the
    indices a of the shape, b of n, and on hask and norm, so that each value meets each instantiation, each head size, each n
    and each value of the others."""
    i = 0
    for a, (nq, nk, hd) in enumerate(ROPE_SHAPES):
        for b, n in enumerate(ROPE_NS):
            for hask in (False, True):
                for norm in (False, True):
                    if norm and hd == 96:
                        continue            # refused: tested on its own
                    yield dict(n=n, nq=nq, nk=nk, hd=hd, hask=hask, norm=norm, inst=2 * hask + norm, r=(4, 8, 16)[(b + hask + norm) % 3],
                               s=(4.0, 2.0, 1.4285714)[(a + b + 2 * hask + norm) % 3], kind=("random", "exact")[(a + b) % 2], seed=i)
                    i += 1


def rope_fwd_data(c):
    n, nq, nk, hd, kind, s = c["n"], c["nq"], c["nk"], c["hd"], c["kind"], c["seed"]
    qkv = operands("random", 2000 + s, (n, (nq + 2 * nk) * hd))
    t = operands(kind, 2100 + s, (n, 32))
    bq_t = operands(kind, 2200 + s, (16, nq * hd), 0.25)
    bv_t = operands(kind, 2300 + s, (16, nk * hd), 0.25)
    tk = operands(kind, 2400 + s, (n, 16)) if c["hask"] else None
    bk_t = operands(kind, 2500 + s, (16, nk * hd), 0.25) if c["hask"] else None
    norm = None
    if c["norm"]:
        norm = dict(wq=bf16_round(1.0 + hash_uniform(2600 + s, (hd,), 0.3)), wk=bf16_round(1.0 + hash_uniform(2700 + s, (hd,), 0.3)),
                    eps=1e-6)
    return qkv, t, bq_t, bv_t, tk, bk_t, norm


def swiglu_lora_data(n, f, r, seed=0):
    g, u, _ = swiglu_data(n, f, seed)
    return g, u, operands("random", 2800 + seed, (n, 32)), operands("random", 2900 + seed, (32, 2 * f), 0.25)
