"""Generate tests/golden/llama_lora_modules_*.npz by RUNNING the reference's ranker training forward on CPU with LoRA on
the Linears `--lora_target_modules` may name (config.py:260, train_ranker.py:71-79), not only its default q_proj / v_proj.

Same method as tests/gen_goldens_rank_train.py (whose restated peft layer `LoraLinear`, batches and collate are reused):
the reference's patched `LlamaForCausalLM.forward` in training mode, fp32, torch autograd gradients of every LoRA matrix,
clipping and two torch.optim.AdamW steps; then the first step again under bf16 autocast with bf16 base weights (the
reference's own arithmetic), of which only the DISTANCE of every gradient tensor to the fp32 one is kept: it is the yardstick
of the GPU test's bars; likewise the second batch's loss under autocast at the fp32 run's parameters after its first step. Two module sets -- all seven Linears, and {k, o, down} (none of the default's) -- on tiny_hd128 and
tiny_gqa (k / v narrower than q). Dropout is 0 (torch's masks cannot be reproduced elsewhere).

Per case two files, each below the size of the existing llama_lora_train_*.npz: `<case>.npz` (batches, losses, fp32
gradients of step 0, bf16 distances) and `<case>_adamw.npz` (the two steps' parameter UPDATES, param - init, as float16:
updates are ~lr = 2e-4, so float16 resolves them to 1e-7, 1 % of the tightest bar that reads them). The initial adapters
are not stored: tests/lora_modules_ref.lora_init regenerates them from the seed.

Only data leaves this script. Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 python tests/gen_goldens_rank_train_modules.py
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

from tests import gen_goldens_rank_train as G  # noqa: E402
from tests import lora_modules_ref as R  # noqa: E402
from tests.gen_goldens import functions_from  # noqa: E402

SETS = {"all7": R.MODULES, "kod": ("k_proj", "o_proj", "down_proj")}
CASES = [("tiny_hd128", 1), ("tiny_gqa", 2)]


def build(name, seed, dtype, modules):
    """G.build's model with LoraLinear around `modules` instead of q_proj / v_proj."""
    from llamarec_amd.llm import LORA_MODULE_BLOCK

    model, cd, _, _ = G.build(name, seed, dtype)
    for layer in model.model.layers:     # undo G.build's q/v wrapping
        for pn in ("q_proj", "v_proj"):
            setattr(layer.self_attn, pn, getattr(layer.self_attn, pn).base)
    lora = R.lora_init(cd, seed, modules, G.R)
    params = {}
    for l, layer in enumerate(model.model.layers):
        for pn in modules:
            block = getattr(layer, LORA_MODULE_BLOCK[pn])
            a = torch.from_numpy(lora[f"layers.{l}.{pn}.lora_A"]).float().clone()
            b = torch.from_numpy(lora[f"layers.{l}.{pn}.lora_B"]).float().clone()
            mod = G.LoraLinear(getattr(block, pn), a, b)
            setattr(block, pn, mod)
            params[f"layers.{l}.{pn}.lora_A"], params[f"layers.{l}.{pn}.lora_B"] = mod.lora_A, mod.lora_B
    return model.train(), cd, lora, params


def run(name, ci, tag):
    seed, modules = 400 + ci, SETS[tag]
    fns = functions_from(os.path.join(G.REF, "trainer", "llm.py"), ["llama_collate_fn_w_truncation"], {"torch": torch})
    collate = fns["llama_collate_fn_w_truncation"](1536, eval=False)
    model, cd, lora, params = build(name, seed, torch.float32, modules)
    names = sorted(params)
    out = {"config": json.dumps(cd), "weight_seed": seed, "lora_r": G.R, "lora_alpha": G.ALPHA,
           "modules": np.array(modules), "param_names": np.array(names)}
    steps = {}
    opt = torch.optim.AdamW([params[n] for n in names], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    for step, (lens, limit) in enumerate((([37, 9, 64, 21], 1.0), ([12, 50, 5], 0.05))):
        samples, batch = G.make_batch(cd, seed * 10 + step, lens, False, collate)
        out[f"step{step}/lens"] = np.array(lens)
        out[f"step{step}/packed_ids"] = np.concatenate([np.array(s["input_ids"]) for s in samples]).astype(np.int32)
        out[f"step{step}/packed_labels"] = np.concatenate([np.array(s["labels"]) for s in samples]).astype(np.int32)
        opt.zero_grad()
        o = model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
        o.loss.backward()
        out[f"step{step}/loss"] = np.float32(o.loss.item())
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
            steps[f"step{step}/update/" + n] = (params[n].detach().numpy().astype(np.float64) - lora[n]).astype(np.float16)
    model, cd, lora, params = build(name, seed, torch.bfloat16, modules)
    samples, batch = G.make_batch(cd, seed * 10, [37, 9, 64, 21], False, collate)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        o = model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
    o.loss.backward()
    out["bf16/loss"] = np.float32(o.loss.item())
    gbf = {n: params[n].grad.detach().float().numpy().astype(np.float64) for n in names}
    out["bf16/grad_rel"] = np.array([R.rel(gbf[n], out["step0/grad/" + n].astype(np.float64)) for n in names])
    cat = lambda g: np.concatenate([np.asarray(g[n], np.float64).ravel() for n in names])
    out["bf16/grad_rel_all"] = np.float64(R.rel(cat(gbf), cat({n: out["step0/grad/" + n] for n in names})))
    # ... and the second batch's loss under bf16 autocast AT the fp32 run's parameters after its first step: what bf16
    # arithmetic alone does to that loss (the yardstick of the GPU test's step-1 loss bar)
    with torch.no_grad():
        for n in names:
            params[n].copy_(after0[n])
    samples, batch = G.make_batch(cd, seed * 10 + 1, [12, 50, 5], False, collate)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        o = model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
    out["bf16/step1_loss"] = np.float32(o.loss.item())
    path = os.path.join(G.OUT, f"llama_lora_modules_{name}_{tag}.npz")
    np.savez_compressed(path, **out)
    np.savez_compressed(path[:-4] + "_adamw.npz", **steps)
    print("wrote", path, os.path.getsize(path), os.path.getsize(path[:-4] + "_adamw.npz"), "bytes; loss", out["step0/loss"],
          out["step1/loss"], "bf16 loss", out["bf16/loss"], out["bf16/step1_loss"], "bf16 vs fp32 grad rel", float(out["bf16/grad_rel_all"]),
          "per tensor", float(out["bf16/grad_rel"].min()), "..", float(out["bf16/grad_rel"].max()))


if __name__ == "__main__":
    for name, ci in CASES:
        for tag in SETS:
            run(name, ci, tag)
