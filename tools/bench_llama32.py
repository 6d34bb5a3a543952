"""Llama-3.2 ranker timings on one MI355X (prints a table and one JSON line). One process, HIP events around every timed
call, median of --reps (30) after warm-up launches of the same shape; the device name and its current clock are printed
beside the numbers.
  1. attention at head_dim 64, (nh, nkv) = (32, 8) (Llama-3.2-1B) and (24, 8), over 16 prompts of 5, 64, 129, 600 and 1 125
     tokens: variant 5 (head_dim-64 MFMA) against the generic kernel -- the parent's behaviour at these shapes -- and, at equal
     nh * hd, against variant 2 at head_dim 128 ((16, 4) and (12, 4) heads). TF/s of the causal work as lr_launch_attention
     counts it (4 nh hd T (T + 1) / 2 per prompt).
     --ab-lib NAME=PATH (repeatable): variant 5 of another BUILD of the library, timed in the same process right after the
     product's for every shape (the 32-vs-64-rows-per-wave arm of DESIGN section 10 is the same source built with
     -DFA5_QT=4 -DFA5_MIN_WG=2).
  2. a random-weight Llama-3.2-1B prefill + verbalizer over a Beauty-sized token budget (prompts of 460 .. 1 125 tokens,
     packing.TOKEN_BUDGET rows): ms per step with attention auto (variant 5) and forced generic, and the kernel split from the
     library's LrProfScope records.
Usage: python tools/bench_llama32.py [--reps 30] [--steps 5] [--layers 16] [--ab-lib qt4=path/to/lib.so]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llamarec_amd import _lib  # noqa: E402
from llamarec_amd._lib import check, lib, stream_ptr  # noqa: E402

KINDS = {0: "gemm 256-tile", 1: "gemm generic", 2: "attention MFMA", 3: "attention generic"}
LENGTHS = (5, 64, 129, 600, 1125)
PROMPTS = 16


def other_build(path):
    """lr_attention_varlen of another build of the library, loaded beside the product's."""
    l = C.CDLL(os.path.abspath(path))
    l.lr_attention_varlen.restype, l.lr_attention_varlen.argtypes = _lib.PROTOTYPES["lr_attention_varlen"]
    return l


def time_attention(L, nh, nkv, hd, T, B, variant, reps):
    n = B * T
    g = torch.Generator(device="cuda").manual_seed(T + nh)
    qkv = torch.randn(n, (nh + 2 * nkv) * hd, generator=g, device="cuda").to(torch.bfloat16)
    out = torch.empty(n, nh * hd, dtype=torch.bfloat16, device="cuda")
    cu = np.arange(0, n + 1, T, dtype=np.int32)
    cud = torch.from_numpy(cu).cuda()

    def run():
        rc = L.lr_attention_varlen(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, variant,
                                   stream_ptr())
        if rc:
            raise RuntimeError(f"lr_attention_varlen: {rc}")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    work = 4.0 * nh * hd * B * T * (T + 1) / 2
    return ms, work / ms / 1e9, out


def attention_table(reps, arms):
    rows = []
    for nh, nkv in ((32, 8), (24, 8)):
        for T in LENGTHS:
            ms5, tf5, o5 = time_attention(lib(), nh, nkv, 64, T, PROMPTS, 5, reps)
            o5 = o5.clone()
            row = dict(nh=nh, nkv=nkv, T=T, B=PROMPTS, v5_ms=ms5, v5_tflops=tf5)
            line = ""
            for name, L in arms.items():
                msa, tfa, oa = time_attention(L, nh, nkv, 64, T, PROMPTS, 5, reps)
                row[f"{name}_ms"], row[f"{name}_tflops"], row[f"{name}_same_bits"] = msa, tfa, bool(torch.equal(oa, o5))
                line += f" | {name} {msa:7.3f} ms {tfa:6.1f} TF/s"
            ms1, tf1, o1 = time_attention(lib(), nh, nkv, 64, T, PROMPTS, 1, reps)
            row["max_abs_v5_minus_generic"] = float((o1.float() - o5.float()).abs().max())
            ms2, tf2, _ = time_attention(lib(), nh // 2, nkv // 2, 128, T, PROMPTS, 2, reps)
            row.update(generic_ms=ms1, generic_tflops=tf1, v2_hd128_ms=ms2, v2_hd128_tflops=tf2, v5_over_generic=ms1 / ms5,
                       v5_over_v2=tf5 / tf2)
            rows.append(row)
            print(f"attention nh={nh:2d} nkv={nkv} {PROMPTS} x {T:4d}: v5 hd64 {ms5:7.3f} ms {tf5:6.1f} TF/s{line} | generic hd64 "
                  f"{ms1:8.3f} ms {tf1:6.2f} TF/s | v2 hd128 {ms2:7.3f} ms {tf2:6.1f} TF/s | v5/generic {ms1 / ms5:5.1f}x "
                  f"v5/v2 {tf5 / tf2:4.2f} | max |v5 - generic| {row['max_abs_v5_minus_generic']:.4f}", flush=True)
    return rows


def llama32_step(steps, layers, attention_variant):
    from llamarec_amd.llm import LLAMA32_1B, LlamaRanker, pack_prompts
    from llamarec_amd.packing import TOKEN_BUDGET

    cfg = dict(LLAMA32_1B, num_hidden_layers=layers)
    model = LlamaRanker.random_init(cfg, seed=1).set_variants(0, attention_variant)
    rng = np.random.default_rng(0)
    seqs, total = [], 0
    while True:
        t = int(rng.integers(460, 1126))
        if total + t > TOKEN_BUDGET:
            break
        seqs.append(np.concatenate([[1], rng.integers(3, cfg["vocab_size"], size=t - 1)]).astype(np.int32))
        total += t
    ids, cu = pack_prompts(seqs)
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    lab = torch.arange(100, 120, dtype=torch.int32, device="cuda")
    out = torch.empty(len(seqs), 20, dtype=torch.float32, device="cuda")
    for _ in range(2):
        model.prefill_verbalize_packed(ids_d, cu_d, cu, lab, out=out)
    torch.cuda.synchronize()
    L = lib()
    check(L.lr_profile_start(steps * (layers * 10 + 32)), "lr_profile_start")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        model.prefill_verbalize_packed(ids_d, cu_d, cu, lab, out=out)
    e1.record()
    torch.cuda.synchronize()
    check(L.lr_profile_stop(), "lr_profile_stop")
    step_ms = e0.elapsed_time(e1) / steps
    split = {}
    for kind, name in KINDS.items():
        ms, work, n = C.c_double(), C.c_double(), C.c_int64()
        L.lr_profile_collect(kind, C.byref(ms), C.byref(work), C.byref(n))
        if n.value:
            split[name] = dict(ms_per_step=ms.value / steps, tflops=work.value / max(ms.value, 1e-9) / 1e9,
                               launches_per_step=n.value / steps)
    assert torch.isfinite(out).all()
    what = "auto (variant 5)" if attention_variant == 0 else f"variant {attention_variant}"
    print(f"llama-3.2-1b ({layers} layers, random weights) prefill + verbalizer, attention {what}: {len(seqs)} prompts, "
          f"{total} tokens: {step_ms:.2f} ms per step", flush=True)
    for name, v in split.items():
        print(f"  {name:18s} {v['ms_per_step']:8.2f} ms/step {v['tflops']:7.1f} TF/s {v['launches_per_step']:6.1f} launches",
              flush=True)
    attn = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("attention"))
    return dict(prompts=len(seqs), tokens=total, layers=layers, attention_variant=attention_variant, step_ms=step_ms,
                kernels=split, attention_share=attn / step_ms), out.clone()


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(0))
    except Exception:   # no SMI binding in this Python: say so instead of guessing
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--ab-lib", action="append", default=[], metavar="NAME=PATH")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    _lib.lib()
    p = torch.cuda.get_device_properties(0)
    box = dict(device=p.name, compute_units=p.multi_processor_count, clock_mhz=clock_mhz(),
               method=f"HIP events, one process, median of {args.reps}")
    print(f"box: {box['device']}, {box['compute_units']} CUs, clock {box['clock_mhz'] or 'not readable here'} MHz at start; {box['method']}", flush=True)
    arms = {}
    for spec in args.ab_lib:
        name, path = spec.split("=", 1)
        arms[name] = other_build(path)
    res = dict(box=box, attention=attention_table(args.reps, arms))
    res["llama32_1b"], auto = llama32_step(args.steps, args.layers, 0)
    res["llama32_1b_generic_attention"], gen = llama32_step(args.steps, args.layers, 1)
    res["max_abs_scores_auto_minus_generic"] = float((auto - gen).abs().max())
    box["clock_mhz_end"] = clock_mhz()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
