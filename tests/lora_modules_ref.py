"""Restatement of the ranker's LoRA training forward with adapters on ANY Linear of a decoder layer, for the tests of
`--lora_target_modules` (tests/test_lora_modules_host.py, tests/test_gpu_lora_modules.py). Test infrastructure only.

torch autograd over one unpadded prompt at a time, float64 by default -- oracle/llama_train_oracle.py's arithmetic
(transformers 4.42.3 modeling_llama.py under the patched forward of model/llm.py:89-127) with peft 0.11.1's lora.Linear
around every selected module:  y = W x + (alpha / r) B A dropout(x).

Dropout masks are explicit, one per (layer, adapter INPUT tensor), the HIP step's convention:
    masks["xn"][l]   input of q_proj, k_proj, v_proj     [tokens, hidden]
    masks["att"][l]  input of o_proj                      [tokens, heads * head_dim]
    masks["xn2"][l]  input of gate_proj, up_proj          [tokens, hidden]
    masks["hmid"][l] input of down_proj                   [tokens, intermediate]
each holding 0 or 1 / (1 - p), rows in packed order. `hip_drop_masks` builds the very masks the kernels use.

mode="bf16" is the restatement's own bf16 arithmetic: every Linear (base and adapter) takes bf16 operands and returns a bf16
tensor, as under torch.autocast; norms, rotary, softmax and the loss run in fp32 like HF's modules. Its distance to the
float64 result is the yardstick for what bf16 arithmetic alone does to each gradient on a given input.
"""
from __future__ import annotations

import numpy as np
import torch

MODULES = ("q_proj", "v_proj", "k_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
INPUT_OF = {"q_proj": "xn", "k_proj": "xn", "v_proj": "xn", "o_proj": "att", "gate_proj": "xn2", "up_proj": "xn2",
            "down_proj": "hmid"}
STREAM_OF = {"xn": 0, "att": 1, "xn2": 2, "hmid": 3}   # j of lr_lora_drop_stream(seed, pass, layer + j * num_layers)


def shapes(cfg, r, modules):
    d, f, nh, nkv = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = d // nh
    io = {"q_proj": (d, nh * hd), "k_proj": (d, nkv * hd), "v_proj": (d, nkv * hd), "o_proj": (nh * hd, d),
          "gate_proj": (d, f), "up_proj": (d, f), "down_proj": (f, d)}
    return {(m, ab): ((r, io[m][0]) if ab == "A" else (io[m][1], r)) for m in MODULES if m in modules for ab in "AB"}


def random_adapters(cfg, r, modules, seed, b_std=0.02):
    """{"layers.{l}.{module}.lora_{A,B}": fp32 array}: A as peft initialises it, B != 0 so that A has a gradient."""
    rng = np.random.default_rng(seed)
    out = {}
    for l in range(cfg["num_hidden_layers"]):
        for (m, ab), shp in shapes(cfg, r, modules).items():
            if ab == "A":
                out[f"layers.{l}.{m}.lora_A"] = rng.uniform(-1, 1, shp).astype(np.float32) / np.sqrt(shp[1])
            else:
                out[f"layers.{l}.{m}.lora_B"] = (rng.standard_normal(shp) * b_std).astype(np.float32)
    return out


def hip_drop_masks(cfg, seed, pass_no, n_rows, p):
    """The four mask families of one loss_grad call (pass_no counts the handle's loss_grad calls from 1)."""
    from oracle.llama_train_oracle import drop_mask

    L, d, f = cfg["num_hidden_layers"], cfg["hidden_size"], cfg["intermediate_size"]
    width = {"xn": d, "att": d, "xn2": d, "hmid": f}   # heads * head_dim == hidden for the configs used here
    return {k: [drop_mask(seed, pass_no, l + j * L, n_rows, width[k], p) for l in range(L)] for k, j in STREAM_OF.items()}


def _rms(x, w, eps, low):
    xf = x.float() if low else x
    y = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return (w.float() * y).to(x.dtype) if low else w * y


def _rope(x, cos, sin):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def loss_and_grads(sd, cfg, lora, seqs, labels, r, alpha, masks=None, mode="float64", device="cpu"):
    """sd: HF-named arrays of the frozen base; lora: {"layers.{l}.{module}.lora_{A,B}": array} for any subset of MODULES.
    Returns (loss, {name: float64 grad array}, last-position logits per prompt [B, vocab] float64)."""
    low = mode == "bf16"
    master = torch.float32 if low else torch.float64
    act = torch.bfloat16 if low else torch.float64
    d, nh, nkv = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd, eps, theta, L = d // nh, cfg["rms_norm_eps"], cfg["rope_theta"], cfg["num_hidden_layers"]
    def tensor(v, dtype):
        v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, np.float64))
        return v.detach().to(device=device, dtype=dtype)

    W = {k: tensor(v, act) for k, v in sd.items()}
    P = {k: tensor(v, master).clone().requires_grad_(True) for k, v in lora.items()}
    scaling = alpha / r

    def linear(x, wname, l, mod, row0):
        y = x @ W[wname].T
        ka = f"layers.{l}.{mod}.lora_A"
        if ka not in P:
            return y
        xd = x
        if masks is not None:
            mk = np.asarray(masks[INPUT_OF[mod]][l][row0:row0 + x.shape[0]], np.float64)
            xd = x * torch.from_numpy(mk).to(device=device, dtype=act)
        return y + ((xd @ P[ka].to(act).T) @ P[f"layers.{l}.{mod}.lora_B"].to(act).T) * scaling

    total, count, row0, last = torch.zeros((), dtype=master, device=device), 0, 0, []
    for ids, lab in zip(seqs, labels):
        T = len(ids)
        inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
        ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
        cdt = torch.float32 if low else torch.float64
        cos, sin = torch.cos(ang).to(device=device, dtype=cdt), torch.sin(ang).to(device=device, dtype=cdt)
        x = W["model.embed_tokens.weight"][torch.as_tensor(np.asarray(ids), device=device).long()]
        causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=device))
        for i in range(L):
            p = f"model.layers.{i}."
            xn = _rms(x, W[p + "input_layernorm.weight"], eps, low)
            q = linear(xn, p + "self_attn.q_proj.weight", i, "q_proj", row0).reshape(T, nh, hd)
            k = linear(xn, p + "self_attn.k_proj.weight", i, "k_proj", row0).reshape(T, nkv, hd)
            v = linear(xn, p + "self_attn.v_proj.weight", i, "v_proj", row0).reshape(T, nkv, hd)
            q, k = _rope(q.to(cdt), cos, sin).to(act), _rope(k.to(cdt), cos, sin).to(act)
            rep = nh // nkv
            k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
            s = torch.einsum("qhd,khd->hqk", q, k) / np.sqrt(hd)
            s = s.masked_fill(~causal[None], float("-inf"))
            pr = torch.softmax(s.to(cdt), dim=-1).to(act)
            att = torch.einsum("hqk,khd->qhd", pr, v).reshape(T, nh * hd)
            x = x + linear(att, p + "self_attn.o_proj.weight", i, "o_proj", row0)
            xn2 = _rms(x, W[p + "post_attention_layernorm.weight"], eps, low)
            g = linear(xn2, p + "mlp.gate_proj.weight", i, "gate_proj", row0)
            u = linear(xn2, p + "mlp.up_proj.weight", i, "up_proj", row0)
            hmid = torch.nn.functional.silu(g) * u
            x = x + linear(hmid, p + "mlp.down_proj.weight", i, "down_proj", row0)
        logits = (_rms(x, W["model.norm.weight"], eps, low) @ W["lm_head.weight"].T).to(master)
        last.append(logits[-1].detach().double().cpu().numpy())
        tgt = torch.as_tensor(np.asarray(lab[1:]), dtype=torch.long, device=device)   # row p predicts token p + 1
        keep = tgt != -100
        if keep.any():
            lp = torch.log_softmax(logits[:-1][keep], dim=-1)
            total = total - lp[torch.arange(int(keep.sum()), device=device), tgt[keep]].sum()
            count += int(keep.sum())
        row0 += T
    loss = total / max(count, 1)
    if count:
        loss.backward()
    grads = {k: (v.grad.double().cpu().numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items()}
    return float(loss.detach()), grads, np.stack(last)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (np.linalg.norm(b) + 1e-30))


def lora_init(cfg, seed, modules, r=8):
    """Deterministic, bf16-representable adapters of the goldens (tests/gen_goldens_rank_train_modules.py regenerates them
    instead of storing them); B is not zero, so that A has a gradient."""
    from llamarec_amd.synth import bf16_round, hash_uniform

    out = {}
    for l in range(cfg["num_hidden_layers"]):
        for j, ((m, ab), shp) in enumerate(shapes(cfg, r, modules).items()):
            out[f"layers.{l}.{m}.lora_{ab}"] = bf16_round(hash_uniform(seed * 131 + l * 16 + j, shp, 0.05))
    return out
