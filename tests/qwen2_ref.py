"""Float32 / bf16 torch restatement of the Qwen2 forward the reference scores with -- HF Qwen2ForCausalLM under
model/llm.py:570-672 -- for one unpadded prompt at a time. Independent of the HIP library and of transformers, so the GPU
tests can compare against it on any device.

Qwen2's arithmetic is Llama's with a bias on three Linears:
  q, k, v   q_proj(x) + b_q, k_proj(x) + b_k, v_proj(x) + b_v; o_proj and the MLP have none
  RMSNorm   out = w * (x * rsqrt(mean(x^2) + eps)).to(dtype), statistics in fp32
  MLP       down(silu(gate(x)) * up(x))
  RoPE      plain, rotate-half over the whole head
  lm_head   the embedding when the state has no lm_head.weight (tie_word_embeddings)
  window    none here: use_sliding_window is false in the goldens, and within the window it is the plain causal mask
Mutants (for the goldens' own check that they are Qwen2's): no_bias drops the three biases; hf_order_bias applies the q and k
biases as a loader would that pair-interleaves the weight rows of every head (row 2i = dim i, row 2i + 1 = dim i + hd/2) for
the rotary epilogue but leaves the biases in HF's order: output dim j then receives the bias of interleaved position j.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.llama3_ref import _rmsnorm, _rope, _rotate_half, _tensors, llama3_inv_freq

QWEN2_MUTANTS = ("no_bias", "hf_order_bias")


def _misplaced(b, hd):
    """What an un-interleaved bias adds in HF's order: packed column c of a head gets b[c]; packed column 2i is HF dim i and
    2i + 1 is HF dim i + hd/2, so HF dim i receives b[2i] and HF dim i + hd/2 receives b[2i + 1]."""
    h = b.view(-1, hd)
    return torch.cat([h[:, 0::2], h[:, 1::2]], -1).reshape(-1)


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
        p = f"model.layers.{i}.self_attn."
        bq, bk, bv = (W[p + f"{n}_proj.bias"] for n in "qkv")
        if mutant == "no_bias":
            bq, bk, bv = torch.zeros_like(bq), torch.zeros_like(bk), torch.zeros_like(bv)
        elif mutant == "hf_order_bias":
            bq, bk = _misplaced(bq, hd), _misplaced(bk, hd)
        h = _rmsnorm(x, W[f"model.layers.{i}.input_layernorm.weight"], eps)
        q = (h @ W[p + "q_proj.weight"].T + bq).view(T, nh, hd).transpose(0, 1)
        k = (h @ W[p + "k_proj.weight"].T + bk).view(T, nkv, hd).transpose(0, 1)
        v = (h @ W[p + "v_proj.weight"].T + bv).view(T, nkv, hd).transpose(0, 1)
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
    """fp32 [B][vocab] logits of each prompt's last token (the patched forward's logits[:, -1].float())."""
    W = _tensors(sd, dtype, device)
    head = W.get("lm_head.weight", W["model.embed_tokens.weight"])
    out = []
    for s in seqs:
        x = _rmsnorm(last_hidden(W, cfg, s, dtype, device, mutant), W["model.norm.weight"], cfg["rms_norm_eps"])
        out.append((x @ head.T).float())
    return torch.stack(out).cpu().numpy()
