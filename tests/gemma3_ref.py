"""Float32 / bf16 torch restatement of the Gemma-3 text forward -- HF Gemma3ForCausalLM / Gemma3TextModel, model_type
"gemma3_text" -- for one unpadded prompt at a time, independent of the HIP library and of transformers, like
tests/gemma2_ref.py and tests/qwen3_ref.py (whose RoPE, norm and weight helpers it restates rather than imports, so the file
reads alone). Plus float64 references with element-wise error bounds for the two kernels the family adds -- sliding-window
attention and the q/k norm sweep in Gemma's rounding -- and named mutants of all three: the same computation with one plausible
bug, to prove that a test built on them can fail.

What Gemma-3 computes, all restated in last_hidden:
  embedding   bf16(bf16(e) * bf16(sqrt(hidden))); tied lm_head
  norms       every norm is bf16(x_f32 * rsqrt(mean(x_f32^2) + eps) * (1 + w_f32))
  sandwich    x = x + post_attention_layernorm(attn(input_layernorm(x)))
              x = x + post_feedforward_layernorm(mlp(pre_feedforward_layernorm(x))),  GeGLU (gelu_pytorch_tanh)
  attention   q, k, v without bias; q = q_norm(q), k = k_norm(k) (one norm over head_dim per head, weights [head_dim] shared by
              the layer's heads); rotate-half RoPE with the LAYER's table; scores q.k * query_pre_attn_scalar^-0.5, no soft cap;
              fp32 softmax; o_proj
  layer kinds layer i is sliding when layer_types[i] == "sliding_attention"; without layer_types when
              (i + 1) % sliding_window_pattern != 0
  mask        a sliding layer's query i sees keys j with i - W < j <= i (W = sliding_window keys, itself included); a global
              layer the plain causal range
  RoPE        sliding layers: rope_local_base_freq, unscaled; global layers: rope_theta with rope_scaling null or linear
              (inv_freq / factor); transformers 5 spells the four numbers as rope_parameters[layer kind]
  head        final norm, tied lm_head, no cap

Windowed attention bound (attention_window_ref64). The kernels (llama_attn_hd256_window.hip, and the generic kernel of
llama_attn.hip with a window) compute, per query row i over its n_i = min(i + 1, W) visible keys j in (i - W, i], the softmax
weights p_j = exp(s_j - m), l = sum_j p_j, ref = sum_j p_j v_j / l, S = sum_j p_j |v_j| / l. Keys outside the window take no part
in any step (masked scores are -inf, their weight is exactly 0), so the rounding points are those of the causal kernels over
the in-window keys only:
  - scores s_j in fp32 (bf16 x bf16 products are exact in fp32; hd of them summed; the scale folded into the exp2 argument with
    log2 e). Their error moves p_j by a relative eps, row-wise
        eps = 2^-24 * scale * hd * |q_i| * max_{i-W<j<=i} |k_j|     (fp32 dot over hd terms, Cauchy-Schwarz)
            + 2^-22 * max_j |s_j| + 2^-21                            (scale / exp-argument rounding, v_exp_f32)
  - P rounded to bf16 before the PV MFMA: relative 2^-9 per weight (at any reference value of the deferred maximum: bf16's
    relative step does not depend on the weight's scale).
  - l summed in fp32 from the fp32 weights (generic) or from the bf16 weights through a ones-MFMA (head_dim 256): relative
    error <= 2^-9 + eps + n_i 2^-24 either way.
  - the numerator accumulated in fp32: relative n_i 2^-24 of sum p|v|.
  - O / l rounded to bf16: relative 2^-9.
First order, with |ref| <= S, exactly as for the causal kernels with n_i in the place of T:
    |got - ref| <= 2^-8 |ref| + (2^-8 + n_i 2^-24 + 2 eps) S          for n_i <= 2^14.
Every term is computed from the data; none is fitted to a kernel's result.

q/k norm sweep bound (qk_norm_rope_ref64, norm_style 1). Per (row, head) over the packed pair-interleaved columns; u = 2^-8 is
bf16's unit roundoff (8 significant bits: half a spacing of 2^-7 at 1):
  - ss = sum x^2 in fp32 (hd positive terms, any order: relative hd 2^-24), ss / hd + eps, sqrt and reciprocal: rstd within
    a relative (hd / 2 + 4) 2^-24; 1 + w rounded to fp32 (2^-24) and the two multiplies (2^-24 each): the normed value before
    rounding within a relative (hd / 2 + 8) 2^-24 <= (hd + 32) 2^-24 / 2; rounded to bf16: u. da = (u + (hd + 32) 2^-24) |a|.
  - the rotation a0 c - a1 s, a1 c + a0 s in fp32 on the bf16 a and the bf16-valued table: two products and an add,
    2^-22 (|a0 c| + |a1 s|) with slack; the inputs' errors enter as |c| da0 + |s| da1. E = that sum.
  - the result rounded to bf16: u (|ref| + E).
    |got - ref| <= E + u (|ref| + E) + 2^-100.
"""
from __future__ import annotations

import numpy as np
import torch

MODEL_MUTANTS = ("window_plus_one", "window_minus_one", "no_window", "local_theta_everywhere", "llama_qk_norm")
WINDOW_MUTANTS = ("window_plus_one", "window_minus_one", "no_window")
CHUNK = 512


# ---------------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------------
def _rmsnorm(x, w, eps, llama_weight=False):
    xf = x.float()
    out = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (out * (w.float() if llama_weight else 1.0 + w.float())).to(x.dtype)


def _rope(T, hd, theta, factor, dtype, device):
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64, device=device).float() / hd))
    if factor is not None:
        inv = inv / factor
    f = torch.outer(torch.arange(T, device=device).float(), inv)
    emb = torch.cat([f, f], -1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def _tensors(sd, dtype, device):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(device=device, dtype=dtype)
            for k, v in sd.items()}


def layer_is_sliding(cfg):
    """[bool per layer]: layer_types when the config has them, else (i + 1) % sliding_window_pattern != 0."""
    lt = cfg.get("layer_types")
    if lt is not None:
        return [t == "sliding_attention" for t in lt]
    return [(i + 1) % cfg["sliding_window_pattern"] != 0 for i in range(cfg["num_hidden_layers"])]


def rope_numbers(cfg):
    """(theta_global, linear factor or None, theta_local) from either spelling of the config."""
    rp = cfg.get("rope_parameters")
    if isinstance(rp, dict) and "full_attention" in rp:
        g, loc = rp["full_attention"], rp["sliding_attention"]
        factor = g.get("factor") if g.get("rope_type") == "linear" else None
        return float(g["rope_theta"]), factor, float(loc["rope_theta"])
    rs = cfg.get("rope_scaling")
    factor = rs["factor"] if rs is not None and (rs.get("rope_type") or rs.get("type")) == "linear" else None
    return float(cfg["rope_theta"]), factor, float(cfg["rope_local_base_freq"])


def window_mask(T, W, device="cpu"):
    """Additive [T][T] mask: 0 where i - W < j <= i, -inf elsewhere. W = None: the plain causal mask."""
    i = torch.arange(T, device=device)[:, None]
    j = torch.arange(T, device=device)[None, :]
    keep = j <= i
    if W is not None:
        keep = keep & (j > i - W)
    return torch.zeros((T, T), device=device).masked_fill(~keep, float("-inf"))


@torch.no_grad()
def last_hidden(W, cfg, ids, dtype=torch.float32, device="cpu", mutant=None):
    """Final-norm input of the last token of one prompt (1-D ids) -> [hidden] in `dtype`. mutant: one of MODEL_MUTANTS."""
    assert mutant is None or mutant in MODEL_MUTANTS, mutant
    d, nh, nkv, hd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    eps = cfg["rms_norm_eps"]
    scaling = cfg["query_pre_attn_scalar"] ** -0.5
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=device)
    T = ids.numel()
    x = W["model.embed_tokens.weight"][ids]
    x = x * torch.tensor(d ** 0.5, dtype=dtype, device=device)
    theta_g, factor, theta_l = rope_numbers(cfg)
    win = cfg["sliding_window"] + {"window_plus_one": 1, "window_minus_one": -1}.get(mutant, 0)
    tables = {False: _rope(T, hd, theta_g, factor, dtype, device), True: _rope(T, hd, theta_l, None, dtype, device)}
    if mutant == "local_theta_everywhere":
        tables[False] = tables[True]
    masks = {False: window_mask(T, None, device), True: window_mask(T, None if mutant == "no_window" else win, device)}
    sliding = layer_is_sliding(cfg)
    llama_w = mutant == "llama_qk_norm"
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        cos, sin = tables[sliding[i]]
        h = _rmsnorm(x, W[p + "input_layernorm.weight"], eps)
        q = (h @ W[p + "self_attn.q_proj.weight"].T).view(T, nh, hd).transpose(0, 1)
        k = (h @ W[p + "self_attn.k_proj.weight"].T).view(T, nkv, hd).transpose(0, 1)
        v = (h @ W[p + "self_attn.v_proj.weight"].T).view(T, nkv, hd).transpose(0, 1)
        q = _rmsnorm(q, W[p + "self_attn.q_norm.weight"], eps, llama_w)
        k = _rmsnorm(k, W[p + "self_attn.k_norm.weight"], eps, llama_w)
        q = q * cos + _rotate_half(q) * sin
        k = k * cos + _rotate_half(k) * sin
        k = k.repeat_interleave(nh // nkv, 0)
        v = v.repeat_interleave(nh // nkv, 0)
        s = (q @ k.transpose(1, 2)) * scaling + masks[sliding[i]].to(dtype)
        a = torch.softmax(s.float(), -1).to(dtype)
        o = (a @ v).transpose(0, 1).reshape(T, nh * hd)
        x = x + _rmsnorm(o @ W[p + "self_attn.o_proj.weight"].T, W[p + "post_attention_layernorm.weight"], eps)
        h = _rmsnorm(x, W[p + "pre_feedforward_layernorm.weight"], eps)
        g = h @ W[p + "mlp.gate_proj.weight"].T
        u = h @ W[p + "mlp.up_proj.weight"].T
        m = (torch.nn.functional.gelu(g, approximate="tanh") * u) @ W[p + "mlp.down_proj.weight"].T
        x = x + _rmsnorm(m, W[p + "post_feedforward_layernorm.weight"], eps)
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


# ---------------------------------------------------------------------------------------------------------------------
# sliding-window attention in float64, with its bound
# ---------------------------------------------------------------------------------------------------------------------
def _split_qkv(qkv, nh, nkv, hd):
    n = qkv.shape[0]
    q = qkv[:, : nh * hd].reshape(n, nh, hd)
    k = qkv[:, nh * hd: (nh + nkv) * hd].reshape(n, nkv, hd)
    v = qkv[:, (nh + nkv) * hd:].reshape(n, nkv, hd)
    return q, k, v


def attention_window_ref64(qkv, cu, nh, nkv, hd, window, mutant=None):
    """Exact float64 sliding-window softmax attention on the bf16 inputs qkv [n][(nh + 2 nkv) hd] (float32 holding bf16
    values), segments cu [B + 1]: query i of a segment sees keys i - window < j <= i. Returns out [n][nh hd] and bound
    [n][nh hd] (module docstring). mutant: one of WINDOW_MUTANTS -- window + 1 keys, window - 1 keys (a row always keeps its
    own key), or no window at all."""
    assert mutant is None or mutant in WINDOW_MUTANTS, mutant
    assert window >= 1
    W = {"window_plus_one": window + 1, "window_minus_one": max(window - 1, 1), "no_window": 1 << 30}.get(mutant, window)
    qkv = np.asarray(qkv, dtype=np.float64)
    cu = np.asarray(cu, dtype=np.int64)
    n = qkv.shape[0]
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    rep = nh // nkv
    scale = 1.0 / np.sqrt(hd)
    out = np.zeros((n, nh * hd))
    bound = np.zeros((n, nh * hd))
    for b in range(len(cu) - 1):
        s0, e0 = int(cu[b]), int(cu[b + 1])
        T = e0 - s0
        assert 0 < T <= 1 << 14, T
        for h in range(nh):
            qh, kh, vh = q[s0:e0, h], k[s0:e0, h // rep], v[s0:e0, h // rep]
            qn = np.linalg.norm(qh, axis=1)
            kn = np.linalg.norm(kh, axis=1)
            for c0 in range(0, T, CHUNK):
                c1 = min(T, c0 + CHUNK)
                rows = np.arange(c0, c1)
                keys = np.arange(c1)[None, :]
                keep = (keys <= rows[:, None]) & (keys > rows[:, None] - W)
                sc = np.where(keep, (qh[c0:c1] @ kh[:c1].T) * scale, -np.inf)
                m = sc.max(axis=1, keepdims=True)
                p = np.exp(sc - m)
                l = p.sum(axis=1, keepdims=True)
                o = (p @ vh[:c1]) / l
                S = (p @ np.abs(vh[:c1])) / l
                smax = np.where(keep, np.abs(sc), 0.0).max(axis=1)
                kmax = np.where(keep, kn[None, :c1], 0.0).max(axis=1)
                n_keys = keep.sum(axis=1)
                eps = 2.0 ** -24 * scale * hd * qn[c0:c1] * kmax + 2.0 ** -22 * smax + 2.0 ** -21
                cols = slice(h * hd, (h + 1) * hd)
                out[s0 + c0: s0 + c1, cols] = o
                bound[s0 + c0: s0 + c1, cols] = (2.0 ** -8 * np.abs(o)
                                                 + (2.0 ** -8 + n_keys[:, None] * 2.0 ** -24 + 2 * eps[:, None]) * S)
    return out, bound


def attention_dense_window(qkv, cu, nh, nkv, hd, window):
    """The same attention as a dense masked softmax over the whole [T][T] score matrix, one (segment, head) at a time, written
    without the chunking and bookkeeping of attention_window_ref64 (the host test compares the two at tiny sizes)."""
    qkv = np.asarray(qkv, dtype=np.float64)
    q, k, v = _split_qkv(qkv, nh, nkv, hd)
    out = np.zeros((qkv.shape[0], nh * hd))
    for b in range(len(cu) - 1):
        s0, e0 = int(cu[b]), int(cu[b + 1])
        T = e0 - s0
        for h in range(nh):
            g = h // (nh // nkv)
            s = np.full((T, T), -np.inf)
            for i in range(T):
                for j in range(T):
                    if i - window < j <= i:
                        s[i, j] = q[s0 + i, h] @ k[s0 + j, g] / np.sqrt(hd)
            e = np.exp(s - s.max(axis=1, keepdims=True))
            out[s0:e0, h * hd:(h + 1) * hd] = (e / e.sum(axis=1, keepdims=True)) @ v[s0:e0, g]
    return out


def ratio(got, ref, bound):
    """max |got - ref| / bound (inf where got is not finite)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


def window_data(regime, cu, nh, nkv, hd, seed=0):
    """bf16-valued qkv for a regime: flat (unit-variance hash_uniform, score std 1) or peaked (q and k times 2: score std ~4, a
    few keys carry a row's weight, so one key more or less at the window's edge is visible)."""
    from llamarec_amd.synth import bf16_round, hash_uniform

    n = int(cu[-1])
    qkv = hash_uniform(seed * 1000 + nh * 100 + nkv * 10 + hd, (n, (nh + 2 * nkv) * hd), 1.0)
    q, k, _ = _split_qkv(qkv, nh, nkv, hd)
    if regime == "peaked":
        q *= 2.0
        k *= 2.0
    elif regime != "flat":
        raise ValueError(regime)
    return bf16_round(qkv)


# ---- the walk of the head_dim-256 windowed kernel, restated from its description ("Gemma-3"), for the case census --
QROWS, KBLOCK, WAVE_ROWS = 128, 64, 16


def window_cases(lens, W):
    """Which of the listed hazards a batch of segment lengths meets at window W, from the block arithmetic alone: a tile of 128
    query rows starting at q0 visits key blocks max(0, q0 - W + 1) // 64 .. min(q0 + 127, T - 1) // 64; a wave is 16 of its rows."""
    c = dict(t_le_w=False, t_eq_w_plus_1=False, odd_first_block=False, skips_two_blocks=False, wave_two_start_blocks=False,
             row_first_block_masked=False)
    for T in lens:
        c["t_le_w"] |= T <= W
        c["t_eq_w_plus_1"] |= T == W + 1
        for q0 in range(0, T, QROWS):
            first = max(0, q0 - W + 1) // KBLOCK
            c["odd_first_block"] |= first % 2 == 1
            c["skips_two_blocks"] |= first >= 2
            for w0 in range(q0, min(q0 + QROWS, T), WAVE_ROWS):
                rows = range(w0, min(w0 + WAVE_ROWS, T))
                starts = {max(0, r - W + 1) // KBLOCK for r in rows}
                c["wave_two_start_blocks"] |= len(starts) > 1
                # a row whose window starts behind the tile's first visited block: that block is wholly masked for it
                c["row_first_block_masked"] |= any(max(0, r - W + 1) // KBLOCK > first for r in rows)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the q/k norm + rotation sweep in float64, with its bound
# ---------------------------------------------------------------------------------------------------------------------
def qk_norm_rope_ref64(x, w, eps, pos, cos, sin, mutant=None):
    """x [rows][heads][hd] (bf16 values) in the packed pair-interleaved order, w [hd] in the same order, cos / sin [T][hd / 2]
    (bf16 values), pos [rows]. Gemma's norm (1 + w) in float64, then the rotation a c - b s, b c + a s on each packed pair
    (a, b) = columns (2i, 2i + 1). Returns (out, bound) [rows][heads][hd]. mutant "llama_qk_norm": w in place of 1 + w."""
    assert mutant in (None, "llama_qk_norm"), mutant
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    hd = x.shape[-1]
    rstd = 1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps)
    a = x * rstd * (w if mutant else 1.0 + w)
    da = (2.0 ** -8 + (hd + 32) * 2.0 ** -24) * np.abs(a)
    c = np.asarray(cos, dtype=np.float64)[pos][:, None, :]
    s = np.asarray(sin, dtype=np.float64)[pos][:, None, :]
    a0, a1, d0, d1 = a[..., 0::2], a[..., 1::2], da[..., 0::2], da[..., 1::2]
    out = np.empty_like(a)
    out[..., 0::2] = a0 * c - a1 * s
    out[..., 1::2] = a1 * c + a0 * s
    E = np.empty_like(a)
    E[..., 0::2] = np.abs(c) * d0 + np.abs(s) * d1 + 2.0 ** -22 * (np.abs(a0 * c) + np.abs(a1 * s))
    E[..., 1::2] = np.abs(c) * d1 + np.abs(s) * d0 + 2.0 ** -22 * (np.abs(a1 * c) + np.abs(a0 * s))
    return out, E + 2.0 ** -8 * (np.abs(out) + E) + 2.0 ** -100
