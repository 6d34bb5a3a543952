"""Float32 / bf16 torch restatement of the Phi-3 forward the reference scores with -- HF Phi3ForCausalLM under
model/llm.py:148-248 -- for one unpadded prompt at a time. Independent of the HIP library and of transformers, so the GPU
tests can compare against it at full width (where the eager HF model would be slow) and on any device.

Phi-3's arithmetic is Llama's behind two fused Linears:
  qkv       qkv_proj(x) cut into q | k | v at nh hd, nkv hd, nkv hd columns
  MLP       gate, up = gate_up_proj(x).chunk(2); down(up * silu(gate))
  RMSNorm   out = w * (x * rsqrt(mean(x^2) + eps)).to(dtype), statistics in fp32
  RoPE      plain, rotate-half over the whole head (no longrope here)
  lm_head   untied
Mutants (for the goldens' own check that they are Phi-3's): swap_gate_up reads the halves of gate_up_proj the other way
round; interleaved_qkv reads qkv_proj as if its rows were stored per KV group, [q of the group | k | v] group after group.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.llama3_ref import _rmsnorm, _rope, _rotate_half, _tensors, llama3_inv_freq


def split_qkv_rows(w, nh, nkv, hd, interleaved=False):
    """q, k, v row blocks of a qkv_proj weight [(nh + 2 nkv) hd][d]"""
    if not interleaved:
        return torch.split(w, [nh * hd, nkv * hd, nkv * hd], 0)
    g = nh // nkv
    w = w.view(nkv, (g + 2) * hd, w.shape[1])
    return (w[:, : g * hd].reshape(nh * hd, -1), w[:, g * hd: (g + 1) * hd].reshape(nkv * hd, -1),
            w[:, (g + 1) * hd:].reshape(nkv * hd, -1))


@torch.no_grad()
def last_hidden(W, cfg, ids, dtype=torch.float32, device="cpu", mutant=None):
    """Final-norm input of the last token of one prompt (1-D ids) -> [hidden] in `dtype`."""
    d, nh, nkv = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = d // nh
    eps = cfg["rms_norm_eps"]
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=device)
    T = ids.numel()
    x = W["model.embed_tokens.weight"][ids]
    cos, sin = _rope(T, llama3_inv_freq(hd, cfg["rope_theta"], None, device), dtype)
    mask = torch.full((T, T), float("-inf"), device=device).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        h = _rmsnorm(x, W[p + "input_layernorm.weight"], eps)
        wq, wk, wv = split_qkv_rows(W[p + "self_attn.qkv_proj.weight"], nh, nkv, hd, mutant == "interleaved_qkv")
        q = (h @ wq.T).view(T, nh, hd).transpose(0, 1)
        k = (h @ wk.T).view(T, nkv, hd).transpose(0, 1)
        v = (h @ wv.T).view(T, nkv, hd).transpose(0, 1)
        q = q * cos + _rotate_half(q) * sin
        k = k * cos + _rotate_half(k) * sin
        k = k.repeat_interleave(nh // nkv, 0)
        v = v.repeat_interleave(nh // nkv, 0)
        s = (q @ k.transpose(1, 2)) * (hd ** -0.5) + mask.to(dtype)
        a = torch.softmax(s.float(), -1).to(dtype)
        o = (a @ v).transpose(0, 1).reshape(T, nh * hd)
        x = x + o @ W[p + "self_attn.o_proj.weight"].T
        h = _rmsnorm(x, W[p + "post_attention_layernorm.weight"], eps)
        g, u = (h @ W[p + "mlp.gate_up_proj.weight"].T).chunk(2, -1)
        if mutant == "swap_gate_up":
            g, u = u, g
        x = x + (u * torch.nn.functional.silu(g)) @ W[p + "mlp.down_proj.weight"].T
    return x[-1]


@torch.no_grad()
def last_logits(sd, cfg, seqs, dtype=torch.float32, device="cpu", mutant=None):
    """fp32 [B][vocab] logits of each prompt's last token (the patched forward's logits[:, -1].float())."""
    W = _tensors(sd, dtype, device)
    out = []
    for s in seqs:
        x = _rmsnorm(last_hidden(W, cfg, s, dtype, device, mutant), W["model.norm.weight"], cfg["rms_norm_eps"])
        out.append((x @ W["lm_head.weight"].T).float())
    return torch.stack(out).cpu().numpy()


def random_phi3_state(cfg, seed, device="cpu", std=0.02, norm_jitter=0.1):
    """Random bf16-valued weights (float32 tensors) under Phi-3's fused names for full-width shapes, generated with torch on
    `device`; norm weights 1 + N(0, norm_jitter)."""
    from llamarec_amd.synth import phi3_param_shapes

    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in phi3_param_shapes(cfg):
        w = torch.randn(*shape, generator=g, device=device)
        w = 1.0 + w * norm_jitter if len(shape) == 1 else w * std
        sd[name] = w.to(torch.bfloat16).float()
    return sd
