"""LRURec user states against whole-history encoding at the Synth-1M shape (parity: tests/test_gpu_lru_state.py).

Arms, alternating inside every repeat of one process, timed with device events, K = 50, history exclusion on:
  (a) retrieve_topk on whole histories                      (b) retrieve_topk_from_states, one new id per user
  (c) advance alone, one new id per user                    (d) encode_last on the same histories
  (e) bootstrap: advance with the whole history on reset states
  (f) encode_states: (d) whose encoder pass also writes the states     (g) retrieve_topk(..., states=): (a) likewise
Prints median and min..max per arm and the ratios (b)/(a), (c)/(d), (f)/(d), (f)/(e) and (g)/(a) per B; the conditions are
(c) < (d) and (f) < (e) at B = 4096.

The times are CALL times between device events: where a call's kernels are shorter than its host-side enqueue (the small
batches, and (c) at any B) they are bounded by the host; kernel times come from a kernel trace of `--arms cd`.

  python tools/bench_lru_state.py [--B 1 32 4096] [--repeats 30] [--arms abcdefg] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llamarec_amd.lru import LRURec, init_lru_state_dict  # noqa: E402
from llamarec_amd.synth import WORKLOADS, synth_users  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, nargs="+", default=[1, 32, 4096])
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--workload", default="synth-1m")
ap.add_argument("--arms", default="abcdefg", help="subset of the arms, e.g. cd (for a kernel trace of the two encoders alone)")
ap.add_argument("--json", default=None)
args = ap.parse_args()
assert args.repeats >= 20, "at least 20 repeats per arm"

K = 50
w = WORKLOADS[args.workload]
model = LRURec.from_state_dict(init_lru_state_dict(w["V"], seed=42))
hist_all, _, n_all, _ = synth_users(args.workload, max(args.B))
rng = np.random.default_rng(0)
results = []
for B in args.B:
    hist = torch.from_numpy(hist_all[:B]).cuda()
    new = torch.from_numpy(rng.integers(1, w["V"] + 1, size=(B, 1))).cuda()
    st = model.new_user_states(B)
    boot = model.new_user_states(B)
    seeded = model.new_user_states(B)   # written by (f) and (g): every call overwrites the rows, no reset between
    model.advance(st, hist)   # bootstrapped states for (b) and (c)

    def arm_e():
        model.reset_user_states(boot)
        return model.advance(boot, hist)

    arms = {
        "a_retrieve_whole": lambda: model.retrieve_topk(hist, K, True),
        "b_retrieve_states": lambda: model.retrieve_topk_from_states(st, K, new_ids=new, exclude=hist),
        "c_advance_one": lambda: model.advance(st, new),
        "d_encode_whole": lambda: model.encode_last(hist),
        "e_bootstrap": arm_e,
        "f_encode_states": lambda: model.encode_states(seeded, hist),
        "g_retrieve_seed": lambda: model.retrieve_topk(hist, K, True, states=seeded),
    }
    arms = {k: f for k, f in arms.items() if k[0] in args.arms}
    for _ in range(args.warmup):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ts.items()}

    def ratio(x, y):
        kx, ky = (next((k for k in med if k[0] == c), None) for c in (x, y))
        return med[kx] / med[ky] if kx and ky else None

    row = {"workload": args.workload, "B": B, "K": K, "V": w["V"], "L": w["L"], "mean_hist": float(n_all[:B].mean()),
           "repeats": args.repeats,
           "ms": {k: {"median": med[k], "min": float(min(v)), "max": float(max(v))} for k, v in ts.items()},
           "b_over_a": ratio("b", "a"), "c_over_d": ratio("c", "d"), "f_over_d": ratio("f", "d"), "f_over_e": ratio("f", "e"),
           "g_over_a": ratio("g", "a")}
    results.append(row)
    print(f"B={B:5d} V={w['V']} L={w['L']} mean_hist={row['mean_hist']:.1f} repeats={args.repeats}")
    for k, v in row["ms"].items():
        print(f"    {k:18s} {v['median']:9.4f} ms   ({v['min']:.4f} .. {v['max']:.4f})")
    print("    " + "    ".join(f"{n} = {row[k]:.4f}" for n, k in (("(b)/(a)", "b_over_a"), ("(c)/(d)", "c_over_d"),
                                                                  ("(f)/(d)", "f_over_d"), ("(f)/(e)", "f_over_e"),
                                                                  ("(g)/(a)", "g_over_a")) if row[k] is not None), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
big = [r for r in results if r["B"] == 4096]
if big and big[0]["c_over_d"] is not None and not big[0]["c_over_d"] < 1.0:
    sys.exit("advance (c) is not faster than encode_last (d) at B = 4096")
if big and big[0]["f_over_e"] is not None and not big[0]["f_over_e"] < 1.0:
    sys.exit("encode_states (f) is not faster than the advance bootstrap (e) at B = 4096")
