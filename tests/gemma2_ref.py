"""Float32 / bf16 torch restatement of the Gemma-2 forward the reference scores with -- HF Gemma2ForCausalLM under
model/llm.py:457-567 -- for one unpadded prompt at a time. Independent of the HIP library and of transformers, like
tests/gemma_ref.py (whose RoPE, norm and weight helpers it restates rather than imports, so either file reads alone).

Gemma-2's differences from Gemma v1, all restated here:
  attention  scores * query_pre_attn_scalar ** -0.5, then cap * tanh(scores / cap) (attn_logit_softcapping, each of the
             three steps in the working dtype as HF's eager attention runs them), then the causal mask and an fp32 softmax.
             Even layers carry a sliding window; a prompt within it sees the plain causal mask, and a longer one is refused.
  sandwich   x = x + post_attention_layernorm(attn(input_layernorm(x)))
             x = x + post_feedforward_layernorm(mlp(pre_feedforward_layernorm(x)))
  head       cap * tanh(logits / cap) (final_logit_softcapping) in the working dtype, then .float()
"""
from __future__ import annotations

import numpy as np
import torch


def _rmsnorm(x, w, eps):
    xf = x.float()
    out = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (out * (1.0 + w.float())).to(x.dtype)


def _rope(T, hd, theta, dtype, device):
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64, device=device).float() / hd))
    f = torch.outer(torch.arange(T, device=device).float(), inv)
    emb = torch.cat([f, f], -1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], -1)


def _tensors(sd, dtype, device):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).to(device=device, dtype=dtype)
            for k, v in sd.items()}


def _softcap(x, cap):
    if cap is None:
        return x
    return torch.tanh(x / cap) * cap


@torch.no_grad()
def last_hidden(W, cfg, ids, dtype=torch.float32, device="cpu"):
    """Final-norm input of the last token of one prompt (1-D ids) -> [hidden] in `dtype`."""
    d, nh, nkv, hd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    eps = cfg["rms_norm_eps"]
    scaling = cfg["query_pre_attn_scalar"] ** -0.5
    ids = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=device)
    T = ids.numel()
    if T > cfg["sliding_window"]:
        raise NotImplementedError(f"{T} tokens exceed the sliding window {cfg['sliding_window']}")
    x = W["model.embed_tokens.weight"][ids]
    x = x * torch.tensor(d ** 0.5, dtype=dtype, device=device)
    theta = cfg.get("rope_theta") or (cfg.get("rope_parameters") or {}).get("rope_theta", 10000.0)
    cos, sin = _rope(T, hd, theta, dtype, device)
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
        s = _softcap((q @ k.transpose(1, 2)) * scaling, cfg["attn_logit_softcapping"]) + mask.to(dtype)
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
def last_logits(sd, cfg, seqs, dtype=torch.float32, device="cpu"):
    """fp32 [B][vocab] logits of each prompt's last token (the patched forward's logits[:, -1], soft-capped, .float())."""
    W = _tensors(sd, dtype, device)
    head = W.get("lm_head.weight", W["model.embed_tokens.weight"])
    out = []
    for s in seqs:
        x = _rmsnorm(last_hidden(W, cfg, s, dtype, device), W["model.norm.weight"], cfg["rms_norm_eps"])
        out.append(_softcap(x @ head.T, cfg["final_logit_softcapping"]).float())
    return torch.stack(out).cpu().numpy()


def random_gemma2_state(cfg, seed, std=0.02, norm_std=0.3, device="cpu"):
    """Random bf16-valued weights (float32 tensors) for full-width shapes, generated with torch on `device`."""
    from llamarec_amd.synth import gemma2_param_shapes

    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in gemma2_param_shapes(cfg):
        s = norm_std if len(shape) == 1 else std
        sd[name] = (torch.randn(*shape, generator=g, device=device) * s).to(torch.bfloat16).float()
    return sd
