"""References for the Qwen3 ranker's one non-Llama step, the per-head RMSNorm of q and k between projection and rotation.
Test infrastructure only: tests/test_qwen3_host.py pins it on the CPU, tests/test_gpu_qwen3*.py compare the HIP kernels with it.

1. sweep_ref64 / sweep_bound: float64 numpy restatement of lr_qk_norm_rope_bf16 (llama_elem.hip, qk_norm_rope_kernel) on packed
   heads, with its error bound in the style of tests/stage2_ref.py. Per (row, head), x = the bf16 values of the head:
     rstd = 1 / sqrt(mean(x^2) + eps)      fp32 in the kernel: hd fused multiply-adds, an hd / 8-lane butterfly, a division, an
                                           add, a square root and a reciprocal -- relative error <= hd 2^-24 (hd >= 16)
     t    = bf16(x rstd)                   first rounding.  The kernel's product differs from the exact one by the relative
                                           (hd + 1) 2^-24, far below a bf16 step, so its t is the reference's or its neighbour:
                                           |t' - t| <= ulp(x rstd), one bf16 ulp
     y    = bf16(w t)                      second rounding. |y' - y| <= |w| |t' - t| + ulp(w t): the first error carried through
                                           the weight, and one bf16 ulp of its own
     out  = bf16(rotation of y)            epi_rope's operation order: a c - b s, b c + a s on the packed pair (a, b) with the
                                           bf16 table entries c, s. With E_a, E_b the bounds of y: |c| E_a + |s| E_b, the three
                                           fp32 roundings 2^-22 (|a c| + |b s|), and one bf16 ulp of the result (the pair bound
                                           tests/test_gpu_qwen2.py holds the rope epilogue to)
   Every term is computed from the data; none is fitted to the kernel's result. ulp(v) is taken at 1.01 |v| so that a value just
   below a power of two is given the step above it, which the other side of the comparison may have rounded to.
   Mutants (SWEEP_MUTANTS), the same restatement with one plausible bug each: no_norm (rotation only), norm_after_rope,
   k_norm_for_q, unpermuted_weight (HF's weight order on packed columns).
2. norm_bwd_ref64: the backward lr_qk_norm_bwd_bf16 computes, dx = rstd (g - xh mean(xh g)) with g = w dy, xh = x rstd, in
   float64, and its bound: the kernel forms rstd (g - x m), m = rstd^2 sum(x g) / hd, in fp32 and rounds once. g = fp32(w dy)
   carries 2^-24 |g|; sum(x g) over hd terms hd 2^-24 sum|x g|; rstd and rstd^2 (hd + 2) 2^-24 relative; the subtraction and the
   products 2^-23 of the larger operand; the result one bf16 ulp:
       |dx' - dx| <= ulp(dx) + rstd [ (hd + 8) 2^-24 (|g| + |x| |m|) + |x| rstd^2 (hd 2^-24 sum|x g| + 2^-24 sum|x g|) / hd ]
3. forward_packed64: the float64 forward WITHOUT roundings on packed heads as a torch function (for autograd).
4. last_logits: float32 / bf16 torch restatement of HF Qwen3ForCausalLM's forward for one unpadded prompt at a time (full-width
   shapes, any device), like tests/qwen2_ref.py. QWEN3_MUTANTS: ones_norm (both norm weights replaced by ones).
"""
from __future__ import annotations

import numpy as np
import torch

from llamarec_amd.synth import bf16_round
from tests.llama3_ref import _rmsnorm, _rope, _rotate_half, _tensors, llama3_inv_freq

SWEEP_MUTANTS = ("no_norm", "norm_after_rope", "k_norm_for_q", "unpermuted_weight")
QWEN3_MUTANTS = ("ones_norm",)


def pack_head(w):
    """HF order [.., hd] -> packed order (2i = HF i, 2i + 1 = HF i + hd/2): _interleave_rope_rows on a head's last axis."""
    w = np.asarray(w)
    h = w.shape[-1] // 2
    out = np.empty_like(w)
    out[..., 0::2], out[..., 1::2] = w[..., :h], w[..., h:]
    return out


def unpack_head(w):
    w = np.asarray(w)
    return np.concatenate([w[..., 0::2], w[..., 1::2]], -1)


def _ulp(v):
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)) * 1.01, 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _r64(v):
    return bf16_round(np.asarray(v, dtype=np.float64).astype(np.float32)).astype(np.float64)


def _weights(nq, nk, hd, wq, wk, mutant):
    """[nq + nk][hd] packed weights per head"""
    wq = np.ones(hd) if wq is None else np.asarray(wq, dtype=np.float64)
    wk = np.ones(hd) if wk is None else np.asarray(wk, dtype=np.float64)
    if mutant == "k_norm_for_q":
        wq = wk
    if mutant == "unpermuted_weight":
        wq, wk = unpack_head(wq), unpack_head(wk)
    return np.concatenate([np.broadcast_to(wq, (nq, hd)), np.broadcast_to(wk, (nk, hd))], 0)


def _rotate(y, c, s):
    a, b = y[..., 0::2], y[..., 1::2]
    out = np.empty_like(y)
    out[..., 0::2], out[..., 1::2] = a * c - b * s, b * c + a * s
    return out


def sweep_ref64(x, pos, cos, sin, nq, nk, hd, wq, wk, eps, mutant=None):
    """x [M][(nq + nk) hd]: bf16 values, packed heads. wq / wk: packed [hd] bf16 values (None with an empty group). cos / sin
    [positions][hd/2]: the bf16 table the kernel reads. Returns (out, bound) float64 [M][(nq + nk) hd]; out carries the two
    roundings of the norm and none after the rotation."""
    M = x.shape[0]
    xh = np.asarray(x, dtype=np.float64).reshape(M, nq + nk, hd)
    w = _weights(nq, nk, hd, wq, wk, mutant)[None]
    p = np.asarray(pos, dtype=np.int64)
    c = np.asarray(cos, dtype=np.float64)[p][:, None, :]
    s = np.asarray(sin, dtype=np.float64)[p][:, None, :]
    rstd = 1.0 / np.sqrt((xh * xh).mean(-1, keepdims=True) + eps)

    def norm(v, r):
        t = v * r
        tb = _r64(t)
        y = _r64(w * tb)
        e = np.abs(w) * (_ulp(t) + hd * 2.0 ** -24 * np.abs(t)) + _ulp(w * tb)
        return y, e

    if mutant == "no_norm":
        y, e = xh, np.zeros_like(xh)
    elif mutant == "norm_after_rope":
        rot = _r64(_rotate(xh, c, s))
        y, e = norm(rot, 1.0 / np.sqrt((rot * rot).mean(-1, keepdims=True) + eps))
        return y.reshape(M, -1), e.reshape(M, -1) + _ulp(y).reshape(M, -1)
    else:
        y, e = norm(xh, rstd)
    out = _rotate(y, c, s)
    a, b, ea, eb = np.abs(y[..., 0::2]), np.abs(y[..., 1::2]), e[..., 0::2], e[..., 1::2]
    ca, sa = np.abs(c), np.abs(s)
    bound = np.empty_like(out)
    bound[..., 0::2] = ca * ea + sa * eb + 2.0 ** -22 * (a * ca + b * sa)
    bound[..., 1::2] = ca * eb + sa * ea + 2.0 ** -22 * (b * ca + a * sa)
    bound += _ulp(out)
    return out.reshape(M, -1), bound.reshape(M, -1)


def norm_bwd_ref64(dy, x, nq, nk, hd, wq, wk, eps):
    """dy, x [M][(nq + nk) hd] bf16 values, packed heads; wq / wk packed [hd]. Returns (dx, bound) float64."""
    M = x.shape[0]
    xh = np.asarray(x, dtype=np.float64).reshape(M, nq + nk, hd)
    d = np.asarray(dy, dtype=np.float64).reshape(M, nq + nk, hd)
    w = _weights(nq, nk, hd, wq, wk, None)[None]
    rstd = 1.0 / np.sqrt((xh * xh).mean(-1, keepdims=True) + eps)
    g = w * d
    xn = xh * rstd
    dx = rstd * (g - xn * (xn * g).mean(-1, keepdims=True))
    sxg = np.abs(xh * g).sum(-1, keepdims=True)
    m = np.abs(rstd * rstd * (xh * g).sum(-1, keepdims=True) / hd)
    bound = _ulp(dx) + rstd * ((hd + 8) * 2.0 ** -24 * (np.abs(g) + np.abs(xh) * m)
                               + np.abs(xh) * rstd * rstd * (hd + 1) * 2.0 ** -24 * sxg / hd) + 2.0 ** -100
    return dx.reshape(M, -1), bound.reshape(M, -1)


def forward_packed64(x, pos, cos, sin, nq, nk, hd, wq, wk, eps):
    """The sweep without roundings, float64 torch (differentiable in x): per-head RMSNorm, then the packed-pair rotation."""
    M = x.shape[0]
    xh = x.reshape(M, nq + nk, hd)
    w = torch.from_numpy(np.ascontiguousarray(_weights(nq, nk, hd, wq, wk, None)))[None]
    y = w * xh * torch.rsqrt((xh * xh).mean(-1, keepdim=True) + eps)
    p = torch.as_tensor(np.asarray(pos, dtype=np.int64))
    c = torch.as_tensor(np.asarray(cos, dtype=np.float64))[p][:, None, :]
    s = torch.as_tensor(np.asarray(sin, dtype=np.float64))[p][:, None, :]
    a, b = y[..., 0::2], y[..., 1::2]
    return torch.stack([a * c - b * s, b * c + a * s], -1).reshape(M, -1)


def normed_packed64(x, nq, nk, hd, wq, wk, eps):
    """The norm alone (no rotation), float64 torch: what lr_qk_norm_bwd_bf16 differentiates."""
    M = x.shape[0]
    xh = x.reshape(M, nq + nk, hd)
    w = torch.from_numpy(np.ascontiguousarray(_weights(nq, nk, hd, wq, wk, None)))[None]
    return (w * xh * torch.rsqrt((xh * xh).mean(-1, keepdim=True) + eps)).reshape(M, -1)


# ---- the whole forward ------------------------------------------------------------------------------------------------------
def _head_norm(x, w, eps):
    """HF Qwen3RMSNorm over the last axis (head_dim): w * (x.float() * rsqrt(mean + eps)).to(dtype)"""
    return _rmsnorm(x, w, eps)


@torch.no_grad()
def last_hidden(W, cfg, ids, dtype=torch.float32, device="cpu", mutant=None):
    d, nh, nkv, hd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    eps = cfg["rms_norm_eps"]
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=device)
    T = ids.numel()
    x = W["model.embed_tokens.weight"][ids]
    cos, sin = _rope(T, llama3_inv_freq(hd, cfg["rope_theta"], None, device), dtype)
    mask = torch.full((T, T), float("-inf"), device=device).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}.self_attn."
        wq, wk = W[p + "q_norm.weight"], W[p + "k_norm.weight"]
        if mutant == "ones_norm":
            wq, wk = torch.ones_like(wq), torch.ones_like(wk)
        h = _rmsnorm(x, W[f"model.layers.{i}.input_layernorm.weight"], eps)
        q = _head_norm((h @ W[p + "q_proj.weight"].T).view(T, nh, hd), wq, eps).transpose(0, 1)
        k = _head_norm((h @ W[p + "k_proj.weight"].T).view(T, nkv, hd), wk, eps).transpose(0, 1)
        v = (h @ W[p + "v_proj.weight"].T).view(T, nkv, hd).transpose(0, 1)
        q = q * cos + _rotate_half(q) * sin
        k = k * cos + _rotate_half(k) * sin
        k = k.repeat_interleave(nh // nkv, 0)
        v = v.repeat_interleave(nh // nkv, 0)
        s = (q @ k.transpose(1, 2)) * (hd ** -0.5) + mask.to(dtype)
        a = torch.softmax(s.float(), -1).to(dtype)
        o = (a @ v).transpose(0, 1).reshape(T, nh * hd)
        x = x + o @ W[p + "o_proj.weight"].T
        p = f"model.layers.{i}."
        h = _rmsnorm(x, W[p + "post_attention_layernorm.weight"], eps)
        g = h @ W[p + "mlp.gate_proj.weight"].T
        u = h @ W[p + "mlp.up_proj.weight"].T
        x = x + (torch.nn.functional.silu(g) * u) @ W[p + "mlp.down_proj.weight"].T
    return x[-1]


@torch.no_grad()
def last_logits(sd, cfg, seqs, dtype=torch.float32, device="cpu", mutant=None):
    """fp32 [B][vocab] logits of each prompt's last token."""
    W = _tensors(sd, dtype, device)
    head = W.get("lm_head.weight", W["model.embed_tokens.weight"])
    out = []
    for s in seqs:
        x = _rmsnorm(last_hidden(W, cfg, s, dtype, device, mutant), W["model.norm.weight"], cfg["rms_norm_eps"])
        out.append((x @ head.T).float())
    return torch.stack(out).cpu().numpy()


def random_qwen3_state(cfg, seed, std=0.02, norm_jitter=0.1, qk_norm_spread=0.5, device="cpu"):
    """Random bf16-valued weights (float32 tensors) for full-width shapes, generated with torch on `device`."""
    from llamarec_amd.synth import qwen3_param_shapes

    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in qwen3_param_shapes(cfg):
        if len(shape) == 1:
            j = qk_norm_spread if name.endswith(("q_norm.weight", "k_norm.weight")) else norm_jitter
            w = 1.0 + (torch.rand(*shape, generator=g, device=device) * 2 - 1) * j
        else:
            w = torch.randn(*shape, generator=g, device=device) * std
        sd[name] = w.to(torch.bfloat16).float()
    return sd
