"""Phi-3 ranker timings on one MI355X (prints a table and one JSON line). One process, HIP events around every timed call, the
arms of a shape ALTERNATING inside every repeat, median and min .. max of --reps (20) after warm-up launches of the same
shape; the device name and its clock are printed beside the numbers.
  1. attention over 16 prompts of 64, 129, 600 and 1 125 tokens at (32, 32) x 96 (Phi-3-mini): variant 7 (head_dim-96 MFMA)
     against the generic kernel -- the parent's behaviour at this head size; it takes every fourth repeat, being some hundred
     times slower -- and at equal width nh * hd = 3072 against variant 5 at (48, 48) x 64 and variant 2 at (24, 24) x 128.
     TF/s of the causal work as lr_launch_attention counts it (4 nh hd T (T + 1) / 2 per prompt).
  2. a random-weight Phi-3-mini prefill + verbalizer (--layers 32) over a Beauty-sized token budget (prompts of 460 .. 1 125
     tokens sharing the 36-token template prefix, packing.TOKEN_BUDGET rows), split into GEMMs / attention / rest from the
     library's own LrProfScope records, with the prefix shared and with prefix_len = 0 (tools/prefix_ab.py's step A/B).
  3. --prefix-ab (instead of 1): the shared-prefix and last-row launches at head_dim 96 against variant 7 on the same whole
     prompts and against full attention + gather (tools/prefix_ab.py's attention arms), then 2.
Usage: python tools/bench_phi3.py [--reps 20] [--layers 32] [--prefix-ab] [--no-step]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llamarec_amd import _lib  # noqa: E402
from llamarec_amd._lib import lib, stream_ptr  # noqa: E402

LENGTHS = (64, 129, 600, 1125)
PROMPTS = 16
# arm -> (nh, nkv, hd, variant, take every n-th repeat)
ARMS = {"v7_hd96": (32, 32, 96, 7, 1), "generic_hd96": (32, 32, 96, 1, 4), "v5_hd64": (48, 48, 64, 5, 1),
        "v2_hd128": (24, 24, 128, 2, 1)}


def attention_table(reps):
    L = lib()
    rows = []
    for T in LENGTHS:
        n = PROMPTS * T
        cu = np.arange(0, n + 1, T, dtype=np.int32)
        cud = torch.from_numpy(cu).cuda()
        g = torch.Generator(device="cuda").manual_seed(T)
        runs, outs = {}, {}
        qkv96 = torch.randn(n, 3 * 3072, generator=g, device="cuda").to(torch.bfloat16)   # every arm: nh = nkv, width 3 x 3072
        for name, (nh, nkv, hd, variant, _) in ARMS.items():
            out = torch.empty(n, nh * hd, dtype=torch.bfloat16, device="cuda")
            outs[name] = out

            def run(out=out, nh=nh, nkv=nkv, hd=hd, variant=variant):
                rc = L.lr_attention_varlen(qkv96.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, PROMPTS, nh, nkv, hd,
                                           variant, stream_ptr())
                if rc:
                    raise RuntimeError(f"lr_attention_varlen: {rc} {L.lr_last_error()}")

            runs[name] = run
        for name, r in runs.items():
            for _ in range(1 if name.startswith("generic") else 3):
                r()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for rep in range(reps):
            for name, r in runs.items():
                if rep % ARMS[name][4]:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        work = 4.0 * 3072 * PROMPTS * T * (T + 1) / 2
        row = dict(T=T, B=PROMPTS, work_flops=work)
        line = f"attention {PROMPTS} x {T:4d}, nh hd = 3072:"
        for name, t in times.items():
            med = float(np.median(t))
            row[name] = dict(ms_median=med, ms_min=min(t), ms_max=max(t), reps=len(t), tflops=work / med / 1e9)
            line += f" | {name} {med:8.3f} ms ({min(t):.3f} .. {max(t):.3f}, n={len(t)}) {work / med / 1e9:7.2f} TF/s"
        row["v7_over_generic"] = row["generic_hd96"]["ms_median"] / row["v7_hd96"]["ms_median"]
        row["max_abs_v7_minus_generic"] = float((outs["v7_hd96"].float() - outs["generic_hd96"].float()).abs().max())
        rows.append(row)
        print(line + f" | v7 / generic {row['v7_over_generic']:.1f}x, max |v7 - generic| {row['max_abs_v7_minus_generic']:.4f}",
              flush=True)
    return rows


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(0))
    except Exception:   # no SMI binding in this Python: say so instead of guessing
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prefix-ab", action="store_true", help="the shared-prefix / last-row attention arms instead of table 1")
    ap.add_argument("--no-step", action="store_true", help="skip the Phi-3-mini step")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    _lib.lib()
    from llamarec_amd.llm import PHI3_MINI
    from tools import prefix_ab

    p = torch.cuda.get_device_properties(0)
    box = dict(device=p.name, compute_units=p.multi_processor_count, clock_mhz=clock_mhz(),
               method=f"HIP events, one process, arms alternating, median of {args.reps}")
    print(f"box: {box['device']}, {box['compute_units']} CUs, clock {box['clock_mhz'] or 'not readable here'} MHz at start; "
          f"{box['method']}", flush=True)
    res = dict(box=box)
    if args.prefix_ab:
        res["attention_prefix"] = prefix_ab.attention_prefix_table(96, 7, ((32, 32),), args.reps)
    else:
        res["attention"] = attention_table(args.reps)
    if not args.no_step:
        step = prefix_ab.step_ab(dict(PHI3_MINI, num_hidden_layers=args.layers), 1, args.reps, {}, "phi-3-mini")
        for arm in step["arms"].values():
            arm["attention_share"] = arm["attention_ms"] / arm["ms_median"]
        res["phi3_mini_step"] = step
        print("phi-3-mini step: attention share " +
              ", ".join(f"{k} {100 * a['attention_share']:.1f} %" for k, a in step["arms"].items()), flush=True)
    box["clock_mhz_end"] = clock_mhz()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
