"""Ranker sessions against whole-prompt prefill at the online shape: B = 1, a Llama-2-7b prompt of --tokens
(460) tokens of which the last --new (160: one more history item and the candidate pool) are not in the user's slot.

  (a) prefill_verbalize of the whole prompt, default GEMM mode
  (b) the same in latency mode (gemm variant 5, split-K)
  (c) extend_verbalize of the whole prompt into an empty slot: the price of the new path when nothing is reused
  (d) extend_verbalize of the last --new tokens behind --tokens - --new cached ones

All arms run in one process on device-resident inputs, alternating inside every repeat; a repeat times --inner back-to-back
calls of an arm between two HIP events. Reported per arm: median and min..max of the repeats' per-call times; per ratio:
median and min..max of the per-repeat ratios. (c) and (d) must give the scores of (a) bit for bit, which is checked first.
Then (d)'s kernel time by kind, from the library's own event profiler in a run of its own.
usage: bench_rank_session.py [--tokens 460] [--new 160] [--layers 32] [--reps 15] [--inner 5]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llamarec_amd import _lib  # noqa: E402
from llamarec_amd.llm import LLAMA2_7B, LlamaRanker  # noqa: E402

KINDS = {0: "GEMM 256-tile", 1: "GEMM generic", 2: "attention MFMA", 3: "attention generic", 6: "element-wise"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=460)
    ap.add_argument("--new", type=int, default=160)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_session.py measures on a GPU; none is visible")
    if not 0 < a.new <= a.tokens:
        raise SystemExit("--new must be in 1 .. --tokens")
    T, c = a.tokens, a.tokens - a.new
    lib = _lib.lib()
    model = LlamaRanker.random_init(dict(LLAMA2_7B, num_hidden_layers=a.layers), seed=42)
    dev = model.device
    rng = np.random.default_rng(0)
    ids = np.concatenate([[1], rng.integers(3, 32000, size=T - 1)]).astype(np.int32)
    labels = torch.arange(319, 339, dtype=torch.int32, device=dev)
    ids_d = torch.from_numpy(ids).to(dev)
    cu_h = np.array([0, T], np.int32)
    cu_d = torch.from_numpy(cu_h).to(dev)
    max_tokens = T
    cache = model.new_prompt_cache(2, max_tokens)   # slot 0: arm (c), always from empty; slot 1: arm (d), c tokens cached
    ws_bytes = lib.lr_llama_extend_workspace_bytes(model._h, T, 1, max_tokens)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = {k: torch.empty((1, 20), dtype=torch.float32, device=dev) for k in "abcd"}

    def extend_args(slot, cached, lo, hi, keep):
        host = [np.array(v, np.int32) for v in ([slot], [cached], [0, hi - lo], [keep])]
        devs = [torch.from_numpy(h).to(dev) for h in host[:3]]
        return host, devs, ids_d[lo:hi]

    def extend(args, dst):
        (sl_h, cl_h, cun_h, keep_h), (sl_d, cl_d, cun_d), new_d = args
        _lib.check(lib.lr_llama_extend_verbalize(
            model._h, cache.table.data_ptr(), 2, max_tokens, sl_d.data_ptr(), sl_h.ctypes.data, cl_d.data_ptr(), cl_h.ctypes.data,
            new_d.data_ptr(), cun_d.data_ptr(), cun_h.ctypes.data, keep_h.ctypes.data, 1, labels.data_ptr(), 20, dst.data_ptr(),
            ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "lr_llama_extend_verbalize")

    args_c = extend_args(0, 0, 0, T, 0)
    args_d = extend_args(1, c, c, T, 0)   # keep 0: the slot holds the first c tokens before and after every call
    if c:
        extend(extend_args(1, 0, 0, c, c), out["d"])

    def arm(name):
        if name == "a":
            model.set_variants(0, 0)
            model.prefill_verbalize_packed(ids_d, cu_d, cu_h, labels, out=out["a"])
        elif name == "b":
            model.set_variants(5, 0)
            model.prefill_verbalize_packed(ids_d, cu_d, cu_h, labels, out=out["b"])
            model.set_variants(0, 0)
        elif name == "c":
            extend(args_c, out["c"])
        else:
            extend(args_d, out["d"])

    for _ in range(3):
        for name in "abcd":
            arm(name)
    torch.cuda.synchronize()
    for name in "cd":
        if not torch.equal(out[name], out["a"]):
            raise SystemExit(f"arm ({name}) does not give the whole-prompt scores: max diff "
                             f"{float((out[name] - out['a']).abs().max()):.3e}")
    print(f"scores of (c) and (d) equal (a) bit for bit; (b) differs by at most {float((out['b'] - out['a']).abs().max()):.3e}")

    ms = {k: [] for k in "abcd"}
    for _ in range(a.reps):
        for name in "abcd":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                arm(name)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.inner)
    what = {"a": "prefill_verbalize, default mode", "b": "prefill_verbalize, latency mode",
            "c": f"extend_verbalize, empty slot ({T} new)", "d": f"extend_verbalize, {c} cached + {a.new} new"}
    print(f"B = 1, {T} prompt tokens, {a.layers} layers, {a.reps} repeats x {a.inner} calls, arms alternating")
    for k in "abcd":
        v = np.array(ms[k])
        print(f"  ({k}) {what[k]:<44s} median {np.median(v):7.3f} ms  (min {v.min():.3f} .. max {v.max():.3f})")
    for num, den in (("d", "a"), ("d", "b"), ("c", "a"), ("c", "b")):
        r = np.array(ms[num]) / np.array(ms[den])
        print(f"  ({num}) / ({den}): median {np.median(r):.3f}  (min {r.min():.3f} .. max {r.max():.3f})")
    rdb = np.array(ms["d"]) / np.array(ms["b"])
    print("  (d) beats (b) outside the spread" if rdb.max() < 1.0 else
          "  (d) does NOT beat (b) outside the spread" if rdb.min() <= 1.0 else "  (d) is slower than (b) in every repeat")

    # (d)'s kernel time by kind: the library's event profiler, in a run of its own (its events serialise the launches)
    n_prof = 5
    _lib.check(lib.lr_profile_start(n_prof * (a.layers * 16 + 32)), "lr_profile_start")
    for _ in range(n_prof):
        arm("d")
    torch.cuda.synchronize()
    lib.lr_profile_stop()
    total = 0.0
    rows = []
    for kind, label in KINDS.items():
        t, w, n = C.c_double(), C.c_double(), C.c_int64()
        lib.lr_profile_collect(kind, C.byref(t), C.byref(w), C.byref(n))
        if n.value:
            rows.append((label, t.value / n_prof, n.value // n_prof))
            total += t.value / n_prof
    print(f"(d) kernel time by kind, per call ({total:.3f} ms in kernels):")
    for label, t, n in rows:
        print(f"  {label:<18s} {t:7.3f} ms  {100 * t / total:5.1f} %  ({n} launches)")


if __name__ == "__main__":
    main()
