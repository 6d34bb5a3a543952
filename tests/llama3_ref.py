"""Float32 / bf16 torch restatement of the Llama forward the reference scores with -- HF LlamaForCausalLM under
model/llm.py:35-145 -- with the `llama3` RoPE frequency scaling of Llama-3.1 / 3.2 (HF's _compute_llama3_parameters), for
one unpadded prompt at a time. Independent of the HIP library and of transformers, so the GPU tests can compare against it
at full width (where the eager HF model would be slow) and on any device.

  RMSNorm    out = w * (x * rsqrt(mean(x^2) + eps)).to(dtype), statistics in fp32
  MLP        down(silu(gate(x)) * up(x))
  RoPE       inv_freq from rope_scaling / rope_parameters (llamarec_amd.llm.rope_parameters), or plain with scaled=False
  lm_head    the embedding when the state has no lm_head.weight (tie_word_embeddings)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from llamarec_amd.llm import rope_parameters


def llama3_inv_freq(hd, theta, scaling, device="cpu"):
    """fp32 inverse frequencies [hd / 2]; scaling = None (plain) or the dict of the four llama3 numbers."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64, device=device).float() / hd))
    if scaling is None:
        return inv
    factor, low, high = scaling["factor"], scaling["low_freq_factor"], scaling["high_freq_factor"]
    orig = scaling["original_max_position_embeddings"]
    low_wavelen, high_wavelen = orig / low, orig / high
    wavelen = 2 * math.pi / inv
    inv_l = torch.where(wavelen > low_wavelen, inv / factor, inv)
    smooth = (orig / wavelen - low) / (high - low)
    smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
    medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
    return torch.where(medium, smoothed, inv_l)


def _rmsnorm(x, w, eps):
    xf = x.float()
    out = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return w * out.to(x.dtype)


def _rope(T, inv, dtype):
    pos = torch.arange(T, device=inv.device).float()
    f = torch.outer(pos, inv)
    emb = torch.cat([f, f], -1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def _tensors(sd, dtype, device):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(device=device, dtype=dtype)
            for k, v in sd.items()}


@torch.no_grad()
def last_hidden(W, cfg, ids, dtype=torch.float32, device="cpu", scaled=True):
    """Final-norm input of the last token of one prompt (1-D ids) -> [hidden] in `dtype`."""
    d, nh, nkv = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or d // nh
    eps = cfg["rms_norm_eps"]
    theta, scaling = rope_parameters(cfg)
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=device)
    T = ids.numel()
    x = W["model.embed_tokens.weight"][ids]
    cos, sin = _rope(T, llama3_inv_freq(hd, theta, scaling if scaled else None, device), dtype)
    mask = torch.full((T, T), float("-inf"), device=device).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        h = _rmsnorm(x, W[p + "input_layernorm.weight"], eps)
        q = (h @ W[p + "self_attn.q_proj.weight"].T).view(T, nh, hd).transpose(0, 1)
        k = (h @ W[p + "self_attn.k_proj.weight"].T).view(T, nkv, hd).transpose(0, 1)
        v = (h @ W[p + "self_attn.v_proj.weight"].T).view(T, nkv, hd).transpose(0, 1)
        q = q * cos + _rotate_half(q) * sin
        k = k * cos + _rotate_half(k) * sin
        k = k.repeat_interleave(nh // nkv, 0)
        v = v.repeat_interleave(nh // nkv, 0)
        s = (q @ k.transpose(1, 2)) * (hd ** -0.5) + mask.to(dtype)
        a = torch.softmax(s.float(), -1).to(dtype)
        o = (a @ v).transpose(0, 1).reshape(T, nh * hd)
        x = x + o @ W[p + "self_attn.o_proj.weight"].T
        h = _rmsnorm(x, W[p + "post_attention_layernorm.weight"], eps)
        g = h @ W[p + "mlp.gate_proj.weight"].T
        u = h @ W[p + "mlp.up_proj.weight"].T
        x = x + (torch.nn.functional.silu(g) * u) @ W[p + "mlp.down_proj.weight"].T
    return x[-1]


@torch.no_grad()
def last_logits(sd, cfg, seqs, dtype=torch.float32, device="cpu", scaled=True):
    """fp32 [B][vocab] logits of each prompt's last token (the patched forward's logits[:, -1].float())."""
    W = _tensors(sd, dtype, device)
    head = W.get("lm_head.weight", W["model.embed_tokens.weight"])
    out = []
    for s in seqs:
        x = _rmsnorm(last_hidden(W, cfg, s, dtype, device, scaled), W["model.norm.weight"], cfg["rms_norm_eps"])
        out.append((x @ head.T).float())
    return torch.stack(out).cpu().numpy()


def llama_param_shapes(cfg):
    """HF LlamaForCausalLM names and shapes with an explicit head_dim; no lm_head.weight when the embeddings are tied."""
    d, f, v = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or d // nh
    out = [("model.embed_tokens.weight", (v, d))]
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        out += [(p + "self_attn.q_proj.weight", (nh * hd, d)), (p + "self_attn.k_proj.weight", (nkv * hd, d)),
                (p + "self_attn.v_proj.weight", (nkv * hd, d)), (p + "self_attn.o_proj.weight", (d, nh * hd)),
                (p + "mlp.gate_proj.weight", (f, d)), (p + "mlp.up_proj.weight", (f, d)), (p + "mlp.down_proj.weight", (d, f)),
                (p + "input_layernorm.weight", (d,)), (p + "post_attention_layernorm.weight", (d,))]
    out.append(("model.norm.weight", (d,)))
    if not cfg.get("tie_word_embeddings"):
        out.append(("lm_head.weight", (v, d)))
    return out


def random_llama_state(cfg, seed, device="cpu", std=0.02, norm_jitter=0.1):
    """Random bf16-valued weights (float32 tensors) for full-width shapes, generated with torch on `device`; norm weights
    1 + N(0, norm_jitter)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in llama_param_shapes(cfg):
        w = torch.randn(*shape, generator=g, device=device)
        w = 1.0 + w * norm_jitter if len(shape) == 1 else w * std
        sd[name] = w.to(torch.bfloat16).float()
    return sd
