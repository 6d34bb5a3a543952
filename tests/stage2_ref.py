"""float64 references with per-element error bounds for the stage-2 kernels (attention and its backward, the GEMM epilogues,
the RoPE table), plus mutants of each: the same reference with one plausible bug, to prove that a test built on the bound can fail.

A plain helper module: test_stage2_ref.py pins it on the CPU, test_gpu_stage2_bounds.py and test_gpu_stage2_bwd_bounds.py
compare the HIP kernels with it.

Attention bound (attention_ref64). The kernels (llama_attn.hip variants 1 / 2, llama_attn256.hip variant 3,
llama_attn_hd256.hip variant 4) compute, per query row i with T = i + 1 keys, exact softmax weights p_j = exp(s_j - m),
l = sum_j p_j, ref = sum_j p_j v_j / l, S = sum_j p_j |v_j| / l:
  - scores s_j in fp32 (bf16 x bf16 products are exact in fp32; hd of them summed; times the scale, or folded into the
    exp2 argument with log2 e). Their error moves p_j by a relative eps, row-wise
        eps = 2^-24 * scale * hd * |q_i| * max_{j<=i} |k_j|      (fp32 dot over hd terms, Cauchy-Schwarz)
            + 2^-22 * max_j |s_j| + 2^-21                          (scale / exp-argument rounding, v_exp_f32)
  - P rounded to bf16 before the PV MFMA: relative 2^-9 per weight.
  - l summed in fp32 from the fp32 weights (variants 1 and 3: the `l * alpha + ps` / lsum adds) or from the bf16 weights
    through a ones-MFMA (variants 2 and 4): relative error <= 2^-9 + eps + T 2^-24 either way.
  - the numerator accumulated in fp32: relative T 2^-24 of sum p|v|.
  - O / l rounded to bf16: relative 2^-9.
Collecting first-order terms, with |ref| <= S:
    |got - ref| <= 2^-9 |O|  +  (2^-9 + eps + T 2^-24) S  +  (2^-9 + eps + T 2^-24) |ref|  + O(2^-17) S
                <= 2^-8 |ref| + (2^-8 + T 2^-24 + 2 eps) S          for T <= 2^14,
the l error's 2^-9 |ref| joining the output rounding's in 2^-8 |ref| and its T 2^-24 |ref| + second-order terms fitting in
the spare 2^-9 S of the S coefficient. eps is the one term a bound without score rounding would miss; it stays below 2^-11
on unit-scale data and is computed from the data, not fitted.
lse (natural log of l times e^m, fp32): |got - ref| <= 2^-8 + eps + 2^-20 |ref|  (relative error of l, fp32 log and add).

Attention backward bound (attention_bwd_ref64). llama_attn_bwd.hip computes, from the inputs AS GIVEN (qkv, dO, the
forward's O and lse), P = exp(scale q.k - lse), D = rowsum(dO o O), dP = dO V^T, dS = P o (dP - D), dQ = scale dS K,
dK = scale dS^T Q, dV = P^T dO (dK, dV summed over the query heads of a group). The reference is that function of those
arrays in float64 -- it does not re-derive O or lse, so the forward's own error (already bounded above) stays out of this
bound, and the same reference serves a call fed the rounded float64 forward and one fed the forward kernel's outputs.
Rounding points, T = prompt length, rep = nh / nkv, row i = a query, column j = a key:
  - scores in fp32 (hd exact products summed: absolute 2^-24 hd scale |q_i||k_j|, Cauchy-Schwarz), then the exponent
    fma(s, scale log2 e, -lse log2 e) of the MFMA passes (the rounded constants, the product lse * log2 e and the fma's result:
    < 2^-24 (2 |s| + 2.5 |lse|) in natural-log units) or acc * scale - lse and __expf of the generic kernels (four roundings of
    values <= |s| + |lse|), then v_exp_f32 (1 ulp). Together a relative error of p_ij, row-wise
        eps_i = 2^-24 scale hd |q_i| max_{j<=i} |k_j|  +  2^-22 (max_j |s_ij| + |lse_i|)  +  2^-21
    -- the forward's eps plus the |lse| term, which the forward does not have (it subtracts a running maximum, not lse).
  - dP in fp32 over hd products: absolute ddP_ij = 2^-24 hd |dO_i||v_j|; D in fp32 over hd products (lt_rowdot_kernel):
    absolute dD_i = 2^-24 hd sum_d |dO_id O_id|. Both enter dS multiplied by p_ij, NOT relative to dS: where dP - D cancels
    this is the term that matters.
  - P (for dV) and dS (for dQ, dK) rounded to bf16 before the second MFMA: relative 2^-9. The generic kernels keep both
    in fp32 (plus one rounding of each product): covered with slack.
  - the second product accumulated in fp32 over at most T terms (dQ) or T rep terms (dK, dV), in any order -- the generic
    path adds dK / dV with fp32 atomics: relative N 2^-24 of the sum of the terms' magnitudes.
  - the scale multiply (2^-24) and the bf16 output rounding: relative 2^-9 of the result.
First order, with c_i(N) = 2^-8 + 2 eps_i + N 2^-24 (2^-9 for the bf16 operand; the other 2^-9 and the second eps_i hold
the second-order products, the subtraction's and the products' own fp32 roundings) and
        E_ij(N) = c_i(N) |dS_ij| + 2 p_ij (ddP_ij + dD_i):
    |dQ - ref| <= scale sum_j E_ij(T) |k_j|          + 2^-8 |dQ|
    |dK - ref| <= scale sum_{h,i} E_ij(T rep) |q_i|  + 2^-8 |dK|
    |dV - ref| <= sum_{h,i} c_i(T rep) p_ij |dO_i|   + 2^-8 |dV|
(2^-8, not 2^-9, on the result: the generic path with a rotary table rounds to bf16 twice, see below), plus 2^-100: weights and
products below fp32's normal range may be flushed to zero, and rows whose gradient is exactly zero have a zero bound otherwise.
With rope = (pos, cos, sin) the gradient is taken back through the rotation of q and k: a' = a c + b s, b' = b c - a s on
each packed pair (a, b), c / s the bf16 table entries, exact in both computations. The MFMA passes rotate the fp32
accumulators in their epilogues (three fp32 roundings, then bf16); the generic path rounds to bf16, lt_rope_bwd_kernel
rotates in fp32 and rounds again. Either way, with B_a, B_b the bounds above (which already hold the first rounding):
        B_a' = |c| B_a + |s| B_b + 2^-22 (|a c| + |b s|) + 2^-8 |a'|          (and the same for b').
Every term is computed from the data; none is fitted to a kernel's result.

Epilogue references follow include/llamarec_mi355x.h (lr_gemm_bf16_nt_epi) and llama_kernels.h at the documented rounding
points, with the rotation stated in the kernel's operation order and no contraction (the library builds with
-ffp-contract=off). RoPE works in HF's rotate-half layout and maps through the pair interleave of lr_llama_pack_qkv
(packed row 2i = HF row i, 2i + 1 = HF row i + hd/2), so an indexing slip in the kernel does not cancel out.
"""
from __future__ import annotations

import numpy as np

from llamarec_amd.synth import bf16_round

ATTN_MUTANTS = ("diag", "late_block", "first_block", "gqa_mod", "half_scale")
BWD_MUTANTS = ("diag", "tail", "gqa_mod", "no_D", "half_scale", "d_other_head", "rotate_forward")
ROPE_MUTANTS = ("pos_plus1", "freq_plus1", "hf_layout")
CHUNK = 512


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _split_qkv(qkv, nh, nkv, hd):
    n = qkv.shape[0]
    q = qkv[:, : nh * hd].reshape(n, nh, hd)
    k = qkv[:, nh * hd: (nh + nkv) * hd].reshape(n, nkv, hd)
    v = qkv[:, (nh + nkv) * hd:].reshape(n, nkv, hd)
    return q, k, v


def _mutant_mask(mutant, rows, T):
    """Extra key mask [rows, T] (True = key kept) of a mutant, rows = positions inside the prompt."""
    keys = np.arange(T)[None, :]
    r = rows[:, None]
    keep = keys <= r
    if mutant == "diag":                       # the diagonal key is left out
        keep &= keys != r
    elif mutant == "late_block":               # rows from 128 on lose key block 1 (keys 64..127)
        keep &= ~((r >= 128) & (keys >= 64) & (keys < 128))
    elif mutant == "first_block":              # rows from 64 on lose key block 0
        keep &= ~((r >= 64) & (keys < 64))
    return keep


def attention_ref64(qkv, cu, nh, nkv, hd, mutant=None):
    """Exact float64 causal softmax attention on the bf16 inputs qkv [n][(nh + 2 nkv) hd] (float32 holding bf16 values),
    segments cu [B + 1]. Returns out [n][nh hd], lse [n][nh], bound [n][nh hd], lse_bound [n][nh] (module docstring).
    mutant: one of ATTN_MUTANTS -- the same computation with that bug (rows left without a key get 0 / -inf)."""
    qkv = np.asarray(qkv, dtype=np.float64)
    cu = np.asarray(cu, dtype=np.int64)
    n = qkv.shape[0]
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    rep = nh // nkv
    scale = 1.0 / np.sqrt(hd / 2 if mutant == "half_scale" else hd)
    out = np.zeros((n, nh * hd))
    bound = np.zeros((n, nh * hd))
    lse = np.full((n, nh), -np.inf)
    lse_bound = np.zeros((n, nh))
    for b in range(len(cu) - 1):
        s0, e0 = int(cu[b]), int(cu[b + 1])
        T = e0 - s0
        assert 0 < T <= 1 << 14, T
        for h in range(nh):
            g = h % nkv if mutant == "gqa_mod" else h // rep
            qh, kh, vh = q[s0:e0, h], k[s0:e0, g], v[s0:e0, g]
            qn = np.linalg.norm(qh, axis=1)
            kmax = np.maximum.accumulate(np.linalg.norm(kh, axis=1))
            for c0 in range(0, T, CHUNK):
                c1 = min(T, c0 + CHUNK)
                rows = np.arange(c0, c1)
                sc = (qh[c0:c1] @ kh[:c1].T) * scale
                keep = _mutant_mask(mutant, rows, c1)
                sc = np.where(keep, sc, -np.inf)
                m = sc.max(axis=1, keepdims=True)
                live = np.isfinite(m[:, 0])
                p = np.exp(sc - np.where(np.isfinite(m), m, 0.0))
                l = p.sum(axis=1, keepdims=True)
                lsafe = np.where(l > 0, l, 1.0)
                o = (p @ vh[:c1]) / lsafe
                S = (p @ np.abs(vh[:c1])) / lsafe
                smax = np.where(keep, np.abs(sc), 0.0).max(axis=1)
                eps = 2.0 ** -24 * scale * hd * qn[c0:c1] * kmax[c0:c1] + 2.0 ** -22 * smax + 2.0 ** -21
                cols = slice(h * hd, (h + 1) * hd)
                out[s0 + c0: s0 + c1, cols] = o
                bound[s0 + c0: s0 + c1, cols] = (2.0 ** -8 * np.abs(o)
                                                 + (2.0 ** -8 + (rows + 1)[:, None] * 2.0 ** -24 + 2 * eps[:, None]) * S)
                lrow = np.where(live, m[:, 0] + np.log(lsafe[:, 0]), -np.inf)
                lse[s0 + c0: s0 + c1, h] = lrow
                lse_bound[s0 + c0: s0 + c1, h] = 2.0 ** -8 + eps + 2.0 ** -20 * np.abs(np.where(live, lrow, 0.0))
    return out, lse, bound, lse_bound


def attention_emul32(qkv, cu, nh, nkv, hd, l_from_bf16_p=False):
    """numpy emulation of the kernels' arithmetic: fp32 scores and weights, P rounded to bf16 for the PV product, fp32
    sums, the row sum l from the fp32 weights (variants 1, 3) or the bf16 ones (l_from_bf16_p: variants 2, 4), bf16 output.
    Returns out [n][nh hd] (bf16 values) and lse [n][nh] fp32."""
    qkv = _f32(qkv)
    n = qkv.shape[0]
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    rep = nh // nkv
    scale = np.float32(1.0 / np.sqrt(np.float32(hd)))
    out = np.zeros((n, nh * hd), np.float32)
    lse = np.zeros((n, nh), np.float32)
    for b in range(len(cu) - 1):
        s0, e0 = int(cu[b]), int(cu[b + 1])
        T = e0 - s0
        for h in range(nh):
            qh, kh, vh = q[s0:e0, h], k[s0:e0, h // rep], v[s0:e0, h // rep]
            for c0 in range(0, T, CHUNK):
                c1 = min(T, c0 + CHUNK)
                sc = (qh[c0:c1] @ kh[:c1].T).astype(np.float32) * scale
                sc = np.where(np.arange(c1)[None, :] <= np.arange(c0, c1)[:, None], sc, np.float32(-np.inf))
                m = sc.max(axis=1, keepdims=True)
                p = np.exp(sc - m).astype(np.float32)
                pb = bf16_round(p)
                l = (pb if l_from_bf16_p else p).sum(axis=1, keepdims=True, dtype=np.float32)
                out[s0 + c0: s0 + c1, h * hd:(h + 1) * hd] = bf16_round((pb @ vh[:c1]).astype(np.float32) / l)
                lse[s0 + c0: s0 + c1, h] = m[:, 0] + np.log(l[:, 0])
    return out, lse


# ---------------------------------------------------------------------------------------------------------------------
# attention backward
# ---------------------------------------------------------------------------------------------------------------------
def rope_rotate64(x, pos, cos, sin, transpose=False):
    """The rotation of epi_rope in float64 without its rounding, on packed heads x [n][heads][hd] (pair (a, b) = columns
    (2i, 2i + 1)): a c - b s, b c + a s with c / s = cos / sin[pos][i]; transpose: its adjoint a c + b s, b c - a s."""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(cos, dtype=np.float64)[np.asarray(pos, dtype=np.int64)][:, None, :]
    s = np.asarray(sin, dtype=np.float64)[np.asarray(pos, dtype=np.int64)][:, None, :]
    if transpose:
        s = -s
    a, b = x[..., 0::2], x[..., 1::2]
    y = np.empty_like(x)
    y[..., 0::2], y[..., 1::2] = a * c - b * s, b * c + a * s
    return y


def _rope_bound(x, bound, rot, pos, cos, sin):
    """Bound of the rotated gradient `rot` of x (module docstring): |c| B_a + |s| B_b + 2^-22 (|a c| + |b s|) + 2^-8 |a'|."""
    c = np.abs(np.asarray(cos, dtype=np.float64))[np.asarray(pos, dtype=np.int64)][:, None, :]
    s = np.abs(np.asarray(sin, dtype=np.float64))[np.asarray(pos, dtype=np.int64)][:, None, :]
    a, b = np.abs(x[..., 0::2]), np.abs(x[..., 1::2])
    Ba, Bb = bound[..., 0::2], bound[..., 1::2]
    out = np.empty_like(bound)
    out[..., 0::2] = c * Ba + s * Bb + 2.0 ** -22 * (a * c + b * s)
    out[..., 1::2] = c * Bb + s * Ba + 2.0 ** -22 * (b * c + a * s)
    return out + 2.0 ** -8 * np.abs(rot)


def attention_bwd_ref64(qkv, d_out, out, lse, cu, nh, nkv, hd, mutant=None, rope=None):
    """Exact float64 backward of the causal attention as a function of the kernel's inputs as given: qkv
    [n][(nh + 2 nkv) hd] and d_out, out [n][nh hd] (bf16 values), lse [n][nh] (fp32 values), segments cu. rope = (pos, cos,
    sin), pos [n] = each row's position inside its prompt, cos / sin [positions][hd/2]: the gradient w.r.t. the unrotated
    q and k. Returns (dqkv, bound), both [n][(nh + 2 nkv) hd] float64 (module docstring). mutant: one of BWD_MUTANTS."""
    qkv = np.asarray(qkv, dtype=np.float64)
    cu = np.asarray(cu, dtype=np.int64)
    n = qkv.shape[0]
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    do = np.asarray(d_out, dtype=np.float64).reshape(n, nh, hd)
    o = np.asarray(out, dtype=np.float64).reshape(n, nh, hd)
    lse = np.asarray(lse, dtype=np.float64)
    rep = nh // nkv
    scale = 1.0 / np.sqrt(hd / 2 if mutant == "half_scale" else hd)
    D = (do * o).sum(-1)
    dD = 2.0 ** -24 * hd * np.abs(do * o).sum(-1)
    if mutant == "no_D":
        D = np.zeros_like(D)
    elif mutant == "d_other_head":
        D = np.roll(D, -1, axis=1)
    dq, dk, dv = np.zeros((n, nh, hd)), np.zeros((n, nkv, hd)), np.zeros((n, nkv, hd))
    bq, bk, bv = np.zeros((n, nh, hd)), np.zeros((n, nkv, hd)), np.zeros((n, nkv, hd))
    for b in range(len(cu) - 1):
        s0, e0 = int(cu[b]), int(cu[b + 1])
        T = e0 - s0
        assert 0 < T <= 1 << 12, T
        rows = np.arange(T)
        keep = rows[None, :] <= rows[:, None]
        if mutant == "diag":
            keep &= rows[None, :] != rows[:, None]
        in_kv = np.ones(T)                              # queries that reach dK / dV
        if mutant == "tail" and T % 64:
            in_kv[T // 64 * 64:] = 0.0
        for h in range(nh):
            g = h % nkv if mutant == "gqa_mod" else h // rep
            qh, kh, vh, doh = q[s0:e0, h], k[s0:e0, g], v[s0:e0, g], do[s0:e0, h]
            s = (qh @ kh.T) * scale
            with np.errstate(over="ignore"):
                p = np.where(keep, np.exp(s - lse[s0:e0, h, None]), 0.0)
            ds = p * (doh @ vh.T - D[s0:e0, h, None])
            smax = np.where(keep, np.abs(s), 0.0).max(axis=1)
            kmax = np.maximum.accumulate(np.linalg.norm(kh, axis=1))
            eps = (2.0 ** -24 * scale * hd * np.linalg.norm(qh, axis=1) * kmax
                   + 2.0 ** -22 * (smax + np.abs(lse[s0:e0, h])) + 2.0 ** -21)
            ddp = 2.0 ** -24 * hd * np.outer(np.linalg.norm(doh, axis=1), np.linalg.norm(vh, axis=1))
            absolute = 2.0 * p * (ddp + dD[s0:e0, h, None])
            c_q = (2.0 ** -8 + 2 * eps + T * 2.0 ** -24)[:, None]
            c_kv = (2.0 ** -8 + 2 * eps + T * rep * 2.0 ** -24)[:, None]
            dq[s0:e0, h] = scale * (ds @ kh)
            bq[s0:e0, h] = scale * ((c_q * np.abs(ds) + absolute) @ np.abs(kh))
            dk[s0:e0, g] += scale * ((ds * in_kv[:, None]).T @ qh)
            bk[s0:e0, g] += scale * ((c_kv * np.abs(ds) + absolute).T @ np.abs(qh))
            dv[s0:e0, g] += (p * in_kv[:, None]).T @ doh
            bv[s0:e0, g] += (c_kv * p).T @ np.abs(doh)
    bq += 2.0 ** -8 * np.abs(dq)
    bk += 2.0 ** -8 * np.abs(dk)
    bv += 2.0 ** -8 * np.abs(dv)
    if rope is not None:
        pos, cos, sin = rope
        for x, bx in ((dq, bq), (dk, bk)):
            rot = rope_rotate64(x, pos, cos, sin, transpose=(mutant != "rotate_forward"))
            bx[...] = _rope_bound(x, bx, rot, pos, cos, sin)
            x[...] = rot
    dqkv = np.concatenate([dq.reshape(n, -1), dk.reshape(n, -1), dv.reshape(n, -1)], axis=1)
    bound = np.concatenate([bq.reshape(n, -1), bk.reshape(n, -1), bv.reshape(n, -1)], axis=1) + 2.0 ** -100
    return dqkv, bound


def attention_bwd_emul32(qkv, d_out, out, lse, cu, nh, nkv, hd, bf16_operands=True, rope=None, round_before_rope=False):
    """numpy emulation of the backward kernels' arithmetic: fp32 scores, P (through exp2 of the folded argument), dP and D,
    P and dS rounded to bf16 for the second product (bf16_operands: the MFMA passes; off: the generic kernels), fp32 sums, bf16
    outputs; rope as in attention_bwd_ref64, rotated in fp32 from the fp32 sums or (round_before_rope: the generic path) from
    their bf16 rounding. Returns dqkv [n][(nh + 2 nkv) hd] (bf16 values)."""
    qkv = _f32(qkv)
    n = qkv.shape[0]
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    do = _f32(d_out).reshape(n, nh, hd)
    o = _f32(out).reshape(n, nh, hd)
    lse = _f32(lse)
    rep = nh // nkv
    log2e = np.float32(1.4426950408889634)
    scale = np.float32(1.0) / np.sqrt(np.float32(hd))
    sl2 = np.float32(scale * log2e)
    D = (do * o).sum(-1, dtype=np.float32)
    rnd = bf16_round if bf16_operands else (lambda x: x)
    dq, dk, dv = (np.zeros((n, nh, hd), np.float32), np.zeros((n, nkv, hd), np.float32), np.zeros((n, nkv, hd), np.float32))
    for b in range(len(cu) - 1):
        s0, e0 = int(cu[b]), int(cu[b + 1])
        T = e0 - s0
        keep = np.arange(T)[None, :] <= np.arange(T)[:, None]
        for h in range(nh):
            g = h // rep
            qh, kh, vh, doh = q[s0:e0, h], k[s0:e0, g], v[s0:e0, g], do[s0:e0, h]
            x = _f32(_f32(_f32(qh @ kh.T) * sl2) - _f32(lse[s0:e0, h, None] * log2e))
            p = np.where(keep, np.exp2(x).astype(np.float32), np.float32(0.0))
            ds = _f32(p * _f32(_f32(doh @ vh.T) - D[s0:e0, h, None]))
            pb, dsb = rnd(p), rnd(ds)
            dq[s0:e0, h] = _f32(dsb @ kh)
            dk[s0:e0, g] += _f32(dsb.T @ qh)
            dv[s0:e0, g] += _f32(pb.T @ doh)
    dq, dk = _f32(dq * scale), _f32(dk * scale)
    if rope is not None:
        pos, cos, sin = rope
        c = _f32(cos)[np.asarray(pos, dtype=np.int64)][:, None, :]
        s = _f32(sin)[np.asarray(pos, dtype=np.int64)][:, None, :]
        for x in (dq, dk):
            y = bf16_round(x) if round_before_rope else x
            a, bb = y[..., 0::2].copy(), y[..., 1::2].copy()
            x[..., 0::2] = _f32(_f32(a * c) + _f32(bb * s))
            x[..., 1::2] = _f32(_f32(bb * c) - _f32(a * s))
    return bf16_round(np.concatenate([dq.reshape(n, -1), dk.reshape(n, -1), dv.reshape(n, -1)], axis=1))


def bwd_ratios(got, ref, bound, nh, nkv, hd):
    """ratio() of the dq, dk and dv column blocks of a packed gradient, separately: {"dq": .., "dk": .., "dv": ..}."""
    edges = (0, nh * hd, (nh + nkv) * hd, (nh + 2 * nkv) * hd)
    got = np.asarray(got)
    return {name: ratio(got[:, a:b], ref[:, a:b], bound[:, a:b]) for name, a, b in zip(("dq", "dk", "dv"), edges, edges[1:])}


def bwd_mutant_applies(mutant, nh, nkv, rope):
    """False where a mutant of BWD_MUTANTS coincides with the correct computation: gqa_mod when h % nkv == h // (nh / nkv)
    for every head, rotate_forward without a rotation."""
    if mutant == "gqa_mod":
        return nkv not in (1, nh)
    if mutant == "rotate_forward":
        return rope is not None
    return True


def ratio(got, ref, bound):
    """max |got - ref| / bound (inf where got is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# attention test data: the regimes of the bound tests
# ---------------------------------------------------------------------------------------------------------------------
def attention_data(regime, cu, nh, nkv, hd, seed=0):
    """bf16-valued qkv for a regime: flat (unit-variance hash_uniform, score std 1), peaked (q and k times 2: score
    std ~4), large_v (|v| up to 2^8), last_block (every 5th row finds its score maximum at its own diagonal key, so the
    maximum arrives only in the row's last key block)."""
    from llamarec_amd.synth import hash_uniform

    n = int(cu[-1])
    qkv = hash_uniform(seed * 1000 + nh * 100 + nkv * 10 + hd, (n, (nh + 2 * nkv) * hd), 1.0)
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    if regime == "peaked":
        q *= 2.0
        k *= 2.0
    elif regime == "large_v":
        v *= 2.0 ** 8 / np.sqrt(3.0)
    elif regime == "last_block":
        rep = nh // nkv
        for b in range(len(cu) - 1):
            rows = np.arange(int(cu[b]), int(cu[b + 1]))[::5]
            for g in range(nkv):
                k[rows, g] = 3.0 * q[rows, g * rep]
    elif regime != "flat":
        raise ValueError(regime)
    return bf16_round(qkv)


ZERO_DOUT_ROWS = 70


def zero_dout_rows(cu):
    """The rows attention_bwd_data sets to zero: the last ZERO_DOUT_ROWS rows of the first prompt of at least 129 rows, as a slice
    (None when no prompt is that long). 70 rows end in a partial 64-row block and start two blocks earlier."""
    lens = np.diff(np.asarray(cu, dtype=np.int64))
    long = np.nonzero(lens >= 129)[0]
    if not len(long):
        return None
    e0 = int(cu[long[0] + 1])
    return slice(e0 - ZERO_DOUT_ROWS, e0)


def attention_bwd_data(cu, nh, hd, seed=0):
    """bf16-valued d_out [n][nh hd]: unit-scale hash_uniform, the rows of zero_dout_rows(cu) exactly zero -- those rows' dq, and
    their dk / dv as keys (every query at or after them has a zero d_out too), must then be exactly zero."""
    from llamarec_amd.synth import hash_uniform

    n = int(cu[-1])
    d_out = bf16_round(hash_uniform(77000 + seed * 1000 + nh * 10 + hd, (n, nh * hd), 1.0))
    z = zero_dout_rows(cu)
    if z is not None:
        d_out[z] = 0.0
    return d_out


# ---------------------------------------------------------------------------------------------------------------------
# GEMM epilogues (acc: the exact product as float64 or float32 [M][N])
# ---------------------------------------------------------------------------------------------------------------------
def epi_store(acc):
    return bf16_round(_f32(acc))


def epi_residual(acc, R):
    return bf16_round(bf16_round(_f32(acc)) + _f32(R))


def _gate_up(acc, swap=False):
    M, N = acc.shape
    a = np.asarray(acc).reshape(M, N // 32, 2, 16)
    gate, up = a[:, :, 0].reshape(M, N // 2), a[:, :, 1].reshape(M, N // 2)
    if swap:
        gate, up = up, gate
    return bf16_round(_f32(gate)).astype(np.float64), bf16_round(_f32(up))


def gated_parts(acc, act, swap=False):
    """(a, u): the activation of bf16(gate) rounded to bf16 (act "silu": g sigmoid(g); "gelu": the tanh-approximate GELU
    0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3)))), float64, and bf16(up)."""
    g, u = _gate_up(acc, swap)
    if act == "silu":
        with np.errstate(over="ignore"):
            a = g / (1.0 + np.exp(-g))
    else:
        a = 0.5 * g * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (g + 0.044715 * g ** 3)))
    return bf16_round(_f32(a)), u


def epi_swiglu(acc, swap=False):
    """bf16(bf16(g sigmoid(g)) u) over gate/up column groups of 16 (lr_llama_pack_gate_up); activation in float64."""
    a, u = gated_parts(acc, "silu", swap)
    return bf16_round(a * u)


def epi_geglu(acc, swap=False):
    """As epi_swiglu with the tanh-approximate GELU."""
    a, u = gated_parts(acc, "gelu", swap)
    return bf16_round(a * u)


def epi_rope(acc, pos, cos, sin, hd, rot_cols, mutant=None):
    """Rotary epilogue on pair-interleaved q/k columns [0, rot_cols): x = bf16(acc); per head, HF's rotate-half on the
    un-interleaved head (HF row i = packed 2i, HF row i + hd/2 = packed 2i + 1), out1 = x1 c - x2 s, out2 = x2 c + x1 s
    in fp32 without contraction, rounded to bf16. cos / sin: [positions][hd/2] bf16 values (the table the kernel reads)."""
    x = bf16_round(_f32(acc))
    M, N = x.shape
    out = x.copy()
    half = hd // 2
    p = np.minimum(np.asarray(pos, dtype=np.int64) + (1 if mutant == "pos_plus1" else 0), len(cos) - 1)
    fi = np.arange(half) + (1 if mutant == "freq_plus1" else 0)
    fi = np.minimum(fi, half - 1)
    c = _f32(cos)[p][:, fi][:, None, :]                      # [M][1][half]
    s = _f32(sin)[p][:, fi][:, None, :]
    heads = x[:, :rot_cols].reshape(M, rot_cols // hd, hd)
    if mutant == "hf_layout":                                # rotate-half on the packed layout as if it were HF's
        x1, x2 = heads[..., :half], heads[..., half:]
    else:
        x1, x2 = heads[..., 0::2], heads[..., 1::2]
    o1 = _f32(_f32(x1 * c) - _f32(x2 * s))
    o2 = _f32(_f32(x2 * c) + _f32(x1 * s))
    rot = np.empty_like(heads)
    if mutant == "hf_layout":
        rot[..., :half], rot[..., half:] = o1, o2
    else:
        rot[..., 0::2], rot[..., 1::2] = o1, o2
    out[:, :rot_cols] = bf16_round(rot.reshape(M, rot_cols))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# RoPE table
# ---------------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    x = np.abs(_f32(x))
    return (np.spacing(x)).astype(np.float64)


def rope_table_hf(T, hd, theta):
    """HF LlamaRotaryEmbedding in fp32: inv_freq = 1 / theta^(arange(0, hd, 2) / hd), angle = pos * inv_freq, cos / sin
    rounded to bf16. Returns cos, sin [T][hd/2] float32 and the fp32 inv_freq [hd/2] and angles [T][hd/2]."""
    inv = (np.float32(1.0) / (np.float32(theta) ** (np.arange(0, hd, 2, dtype=np.float32) / np.float32(hd)))).astype(np.float32)
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return bf16_round(np.cos(ang).astype(np.float32)), bf16_round(np.sin(ang).astype(np.float32)), inv, ang


def rope_band(T, hd, theta):
    """Acceptance band of a device RoPE table: for every (pos, i), the bf16 values cos / sin take over the angle interval
    theta_hf +- (4 ulp_f32(theta_hf) + pos * 2 ulp_f32(inv_freq_hf)), the fp32 cos / sin themselves within 2 ulp -- bf16
    rounding is monotone, so that set is every bf16 value between the rounded minimum and maximum over the interval (both
    ends and any interior extremum, float64).
    Returns (cos_lo, cos_hi, sin_lo, sin_hi), float64 [T][hd/2]."""
    _, _, inv, ang = rope_table_hf(T, hd, theta)
    a = ang.astype(np.float64)
    w = 4 * _ulp32(ang) + np.arange(T, dtype=np.float64)[:, None] * 2 * _ulp32(inv)[None, :]
    lo, hi = a - w, a + w
    res = []
    for f, shift in ((np.cos, 0.0), (np.sin, np.pi / 2)):
        fa, fb = f(lo), f(hi)
        fmin, fmax = np.minimum(fa, fb), np.maximum(fa, fb)
        # extrema of cos at k pi, of sin at pi/2 + k pi: k = ceil((lo - shift) / pi) .. if <= hi
        kk = np.ceil((lo - shift) / np.pi)
        inside = kk * np.pi + shift <= hi
        val = np.where(np.mod(kk, 2) == 0, 1.0, -1.0)
        fmax = np.where(inside & (val > 0), 1.0, fmax)
        fmin = np.where(inside & (val < 0), -1.0, fmin)
        # (two extrema inside the interval would need w > pi / 2: not at these sizes.) The device rounds cosf / sinf,
        # each within 2 fp32 ulp of the true value, to bf16: the band is bf16(fmin - 2 ulp) .. bf16(fmax + 2 ulp).
        lo32, hi32 = _f32(fmin), _f32(fmax)
        res += [bf16_round(lo32 - 2 * np.spacing(np.abs(lo32))).astype(np.float64),
                bf16_round(hi32 + 2 * np.spacing(np.abs(hi32))).astype(np.float64)]
    return tuple(res)
