"""float64 references with per-element error bounds for the stage-2 kernels (attention, the GEMM epilogues, the RoPE
table), plus mutants of each: the same reference with one plausible bug, to prove that a test built on the bound can fail.

A plain helper module: test_stage2_ref.py pins it on the CPU, test_gpu_stage2_bounds.py compares the HIP kernels with it.

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

Epilogue references follow include/llamarec_mi355x.h (lr_gemm_bf16_nt_epi) and llama_kernels.h at the documented rounding
points, with the rotation stated in the kernel's operation order and no contraction (the library builds with
-ffp-contract=off). RoPE works in HF's rotate-half layout and maps through the pair interleave of lr_llama_pack_qkv
(packed row 2i = HF row i, 2i + 1 = HF row i + hd/2), so an indexing slip in the kernel does not cancel out.
"""
from __future__ import annotations

import numpy as np

from llamarec_amd.synth import bf16_round

ATTN_MUTANTS = ("diag", "late_block", "first_block", "gqa_mod", "half_scale")
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
