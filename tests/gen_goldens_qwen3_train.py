"""Generate tests/golden/qwen3_lora_train_*.npz by RUNNING HF Qwen3ForCausalLM's training forward on the CPU, in the manner of
tests/gen_goldens_rank_train.py (whose restated peft layer `LoraLinear`, batches and use of the reference's collate are reused):
shifted cross-entropy over the positions whose label is not -100 (what the reference's patched forwards compute,
model/llm.py:116-127, and HF's own `labels=` path), fp32, LoRA r = 8, alpha = 32, torch autograd gradients of every LoRA matrix,
clipping and two torch.optim.AdamW steps; then the first step again under bf16 autocast with bf16 base weights, of which the
DISTANCE of every gradient tensor to the fp32 one is kept: the yardstick of the GPU test's bars.

On tests/gen_goldens_qwen3.py's hd128_gqa config, once with adapters on q_proj | v_proj ("qv") and once on q, k, v and o
("qkvo"), so that a delta passes through k_norm. For "qkvo" the first step is also run on a model WITHOUT k_norm (the module
replaced by the identity): the gradient of every k_proj.lora_B there must be more than 10 % (relative L2) from the true one --
asserted here, and stored so that the GPU test can hold the HIP step to the same margin.

One file per case: batches, losses (with the bf16 run's for both batches), the fp32 gradients of step 0, the bf16 distances, and the two steps' parameter UPDATES
(param - init) as float16 (updates are ~lr = 2e-4, which float16 resolves to 1e-7). The initial adapters are not stored:
lora_init below regenerates them from the seed. Fixed zip timestamps: a rerun with one thread reproduces the files byte for byte.

Only data leaves this script. Run from the repo root:
    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 PYTHONDONTWRITEBYTECODE=1 python -m tests.gen_goldens_qwen3_train <reference dir> [out dir]
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

from llamarec_amd.synth import bf16_round, hash_uniform, synth_qwen3_state
from tests.gen_goldens_gemma import save_npz_fixed

R, ALPHA = 8, 32
CONFIG = "hd128_gqa"
SETS = {"qv": ("q_proj", "v_proj"), "qkvo": ("q_proj", "v_proj", "k_proj", "o_proj")}
STEPS = (([37, 9, 64, 21], 1.0), ([12, 50, 5], 0.05))
# Width of the q / k norm weights (1 + U(.)) of the train goldens. The GPU test holds a bf16 step to fixed bars (loss 4e-3, 3 %
# per gradient tensor, 1.5 % overall); they can only be asked where bf16 arithmetic itself meets them, so the width is the
# widest of 0.75, 0.5, 0.3 at which the reference's OWN bf16-autocast run does, on both module sets -- asserted in run():
#   0.75 (the scoring goldens' width)  loss gap 5.9e-3 / 1.8e-3, gradients 2.6 % / 2.1 % overall, up to 3.6 % per tensor   misses
#   0.5                                 loss gap 4.3e-3 / 0.6e-3, gradients 1.6 % / 1.6 % overall, up to 3.1 % per tensor   misses
#   0.3                                 loss gap 3.9e-3 / 0.1e-3, gradients 1.42 % / 1.48 % overall, up to 2.7 % per tensor meets
# (q_proj | v_proj / q, k, v, o). The sharper the normed scores, the more a bf16 rounding of q or k moves the softmax.
QK_NORM_SPREAD = 0.3


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (np.linalg.norm(b) + 1e-30))


def lora_shapes(cfg, modules, r=R):
    d, nh, nkv, hd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    io = {"q_proj": (d, nh * hd), "k_proj": (d, nkv * hd), "v_proj": (d, nkv * hd), "o_proj": (nh * hd, d)}
    return {(m, ab): ((r, io[m][0]) if ab == "A" else (io[m][1], r)) for m in modules for ab in "AB"}


def lora_init(cfg, seed, modules, r=R):
    """Deterministic, bf16-representable adapters {"layers.{l}.{module}.lora_{A,B}": fp32 array}; B is not zero, so that A has
    a gradient."""
    out = {}
    for l in range(cfg["num_hidden_layers"]):
        for j, ((m, ab), shp) in enumerate(lora_shapes(cfg, modules, r).items()):
            out[f"layers.{l}.{m}.lora_{ab}"] = bf16_round(hash_uniform(seed * 137 + l * 16 + j, shp, 0.05))
    return out


def build(cd, sd, lora, dtype, modules, drop_k_norm=False):
    from tests.gen_goldens_qwen3 import hf_model
    from tests.gen_goldens_rank_train import LoraLinear

    model = hf_model(cd, sd).to(dtype)
    for p in model.parameters():
        p.requires_grad_(False)
    params = {}
    for l, layer in enumerate(model.model.layers):
        if drop_k_norm:
            layer.self_attn.k_norm = torch.nn.Identity()
        for pn in modules:
            a = torch.from_numpy(lora[f"layers.{l}.{pn}.lora_A"]).float().clone()   # fp32 masters, like peft
            b = torch.from_numpy(lora[f"layers.{l}.{pn}.lora_B"]).float().clone()
            mod = LoraLinear(getattr(layer.self_attn, pn), a, b)
            setattr(layer.self_attn, pn, mod)
            params[f"layers.{l}.{pn}.lora_A"], params[f"layers.{l}.{pn}.lora_B"] = mod.lora_A, mod.lora_B
    return model.train(), params


def forward_loss(model, batch):
    mask = batch["attention_mask"]
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    return model(input_ids=batch["input_ids"], attention_mask=mask, position_ids=pos, labels=batch["labels"]).loss


def run(REF, OUT, tag, ci):
    from tests import gen_goldens_rank_train as G
    from tests.gen_goldens import functions_from
    from tests.gen_goldens_qwen3 import QWEN3_CONFIGS, qwen3_cfg_dict

    modules, seed = SETS[tag], 800 + ci
    cd = qwen3_cfg_dict(CONFIG)
    std, spread = QWEN3_CONFIGS[CONFIG][-2], QK_NORM_SPREAD
    sd = synth_qwen3_state(cd, seed, std=std, qk_norm_spread=spread)
    if not cd["tie_word_embeddings"]:
        raise SystemExit("the train goldens assume the tied head of hd128_gqa")
    lora = lora_init(cd, seed, modules)
    fns = functions_from(os.path.join(REF, "trainer", "llm.py"), ["llama_collate_fn_w_truncation"], {"torch": torch})
    collate = fns["llama_collate_fn_w_truncation"](1536, eval=False)
    model, params = build(cd, sd, lora, torch.float32, modules)
    names = sorted(params)
    out = {"config": np.array(json.dumps(cd, sort_keys=True)), "weight_seed": np.array(seed), "weight_std": np.array(std),
           "qk_norm_spread": np.array(spread), "lora_r": np.array(R), "lora_alpha": np.array(ALPHA), "modules": np.array(modules),
           "param_names": np.array(names)}
    opt = torch.optim.AdamW([params[n] for n in names], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    for step, (lens, limit) in enumerate(STEPS):
        samples, batch = G.make_batch(cd, seed * 10 + step, lens, False, collate)
        out[f"step{step}/lens"] = np.array(lens)
        out[f"step{step}/packed_ids"] = np.concatenate([np.array(s["input_ids"]) for s in samples]).astype(np.int32)
        out[f"step{step}/packed_labels"] = np.concatenate([np.array(s["labels"]) for s in samples]).astype(np.int32)
        opt.zero_grad()
        loss = forward_loss(model, batch)
        loss.backward()
        out[f"step{step}/loss"] = np.float32(loss.item())
        if step == 0:
            for n in names:
                out["step0/grad/" + n] = params[n].grad.detach().numpy().copy()
        norm = torch.nn.utils.clip_grad_norm_([params[n] for n in names], limit)
        out[f"step{step}/grad_norm"] = np.float32(float(norm))
        out[f"step{step}/clip_limit"] = np.float32(limit)
        opt.step()
        if step == 0:
            after0 = {n: params[n].detach().clone() for n in names}
        for n in names:
            out[f"step{step}/update/" + n] = (params[n].detach().numpy().astype(np.float64) - lora[n]).astype(np.float16)
    # the first step under bf16 autocast with bf16 base weights: what bf16 arithmetic alone does to each gradient
    model, params = build(cd, sd, lora, torch.bfloat16, modules)
    samples, batch = G.make_batch(cd, seed * 10, STEPS[0][0], False, collate)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        loss = forward_loss(model, batch)
    loss.backward()
    out["bf16/loss"] = np.float32(loss.item())
    gbf = {n: params[n].grad.detach().float().numpy().astype(np.float64) for n in names}
    out["bf16/grad_rel"] = np.array([rel(gbf[n], out["step0/grad/" + n].astype(np.float64)) for n in names])
    cat = lambda g: np.concatenate([np.asarray(g[n], np.float64).ravel() for n in names])  # noqa: E731
    out["bf16/grad_rel_all"] = np.float64(rel(cat(gbf), cat({n: out["step0/grad/" + n] for n in names})))
    # ... and the second batch's loss under bf16 autocast AT the fp32 run's parameters after its first step: what bf16 arithmetic
    # alone does to that loss (the yardstick of the GPU test's step-1 loss bar, as in tests/gen_goldens_rank_train_modules.py)
    with torch.no_grad():
        for n in names:
            params[n].copy_(after0[n])
    _, batch1 = G.make_batch(cd, seed * 10 + 1, STEPS[1][0], False, collate)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        out["bf16/step1_loss"] = np.float32(forward_loss(model, batch1).item())
    assert abs(float(out["bf16/loss"]) - float(out["step0/loss"])) < 4e-3 and float(out["bf16/grad_rel"].max()) < 3e-2 and \
        float(out["bf16/grad_rel_all"]) < 1.5e-2, "the reference's own bf16 run misses the GPU test's bars: see QK_NORM_SPREAD"
    margins = []
    if "k_proj" in modules:   # the same step on a model without k_norm: k_proj.lora_B's gradient must be clearly another one
        model, params = build(cd, sd, lora, torch.float32, modules, drop_k_norm=True)
        forward_loss(model, batch).backward()
        for n in names:
            if n.endswith("k_proj.lora_B"):
                g = params[n].grad.detach().numpy().copy()
                out["no_k_norm/grad/" + n] = g
                margins.append(rel(g, out["step0/grad/" + n].astype(np.float64)))
                assert np.linalg.norm(out["step0/grad/" + n]) > 0 and margins[-1] > 0.1, (n, margins[-1])
    path = os.path.join(OUT, f"qwen3_lora_train_{CONFIG}_{tag}.npz")
    save_npz_fixed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; loss", out["step0/loss"], out["step1/loss"], "bf16 loss", out["bf16/loss"], out["bf16/step1_loss"],
          "grad norm", out["step0/grad_norm"], "bf16 vs fp32 grad rel", float(out["bf16/grad_rel_all"]), "per tensor",
          float(out["bf16/grad_rel"].min()), "..", float(out["bf16/grad_rel"].max()), "k_proj.lora_B without k_norm", margins)


def main(REF, OUT):
    warnings.filterwarnings("ignore")
    torch.manual_seed(0)
    for ci, tag in enumerate(SETS):
        run(REF, OUT, tag, ci)


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LLAMAREC_REFERENCE", "")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("usage: python -m tests.gen_goldens_qwen3_train <reference tree> [out dir]")
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    main(ref, out_dir)
