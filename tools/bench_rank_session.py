"""Ranker sessions against whole-prompt prefill at the online shape: B = 1, a Llama-2-7b prompt of --tokens
(460) tokens of which the last --new (160: one more history item and the candidate pool; 32: one item and a short pool) are
not in the user's slot.

  (a) prefill_verbalize of the whole prompt, default GEMM mode
  (b) the same in latency mode (gemm variant 5, split-K)
  (c) extend_verbalize of the whole prompt into an empty slot: the price of the new path when nothing is reused
  (d) extend_verbalize of the last --new tokens behind --tokens - --new cached ones
  (e) prefill_verbalize of the whole prompt in the row-invariant latency mode (gemm variant 7)
  (f) (d) under gemm variant 7: the split-K products on the new rows only, K | V written by the QKV product's reduce pass
  (g) (f) with LR_EXTEND_SEPARATE_CACHE_WRITE=1: the reduce pass writes ws.qkv and kv_cache_write_kernel copies

All arms run in one process on device-resident inputs, alternating inside every repeat; a repeat times --inner back-to-back
calls of an arm between two HIP events. Reported per arm: median and min..max of the repeats' per-call times; per ratio:
median and min..max of the per-repeat ratios. (c) and (d) must give the scores of (a) bit for bit, (f) and (g) those of (e),
which is checked first. Then (d)'s and (f)'s kernel time by kind, from the library's own event profiler in runs of their own.
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
ARMS = "abcdefg"
SEPARATE = "LR_EXTEND_SEPARATE_CACHE_WRITE"


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
    os.environ.pop(SEPARATE, None)
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
    # slot 0: arm (c), always from empty; slots 1, 2, 3: arms (d), (f), (g), c tokens cached -- (f)'s and (g)'s in variant 7's bits
    n_slots = 4
    cache = model.new_prompt_cache(n_slots, max_tokens)
    ws_bytes = lib.lr_llama_extend_workspace_bytes(model._h, T, 1, max_tokens)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = {k: torch.empty((1, 20), dtype=torch.float32, device=dev) for k in ARMS}

    def extend_args(slot, cached, lo, hi, keep):
        host = [np.array(v, np.int32) for v in ([slot], [cached], [0, hi - lo], [keep])]
        devs = [torch.from_numpy(h).to(dev) for h in host[:3]]
        return host, devs, ids_d[lo:hi]

    def extend(args, dst):
        (sl_h, cl_h, cun_h, keep_h), (sl_d, cl_d, cun_d), new_d = args
        _lib.check(lib.lr_llama_extend_verbalize(
            model._h, cache.table.data_ptr(), n_slots, max_tokens, sl_d.data_ptr(), sl_h.ctypes.data, cl_d.data_ptr(),
            cl_h.ctypes.data, new_d.data_ptr(), cun_d.data_ptr(), cun_h.ctypes.data, keep_h.ctypes.data, 1, labels.data_ptr(), 20,
            dst.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "lr_llama_extend_verbalize")

    args_c = extend_args(0, 0, 0, T, 0)
    # keep 0: a slot holds the first c tokens before and after every call
    args = {"d": extend_args(1, c, c, T, 0), "f": extend_args(2, c, c, T, 0), "g": extend_args(3, c, c, T, 0)}
    if c:
        extend(extend_args(1, 0, 0, c, c), out["d"])
        model.set_variants(7, 0)
        extend(extend_args(2, 0, 0, c, c), out["f"])
        extend(extend_args(3, 0, 0, c, c), out["g"])
        model.set_variants(0, 0)

    def arm(name):
        if name == "a":
            model.set_variants(0, 0)
            model.prefill_verbalize_packed(ids_d, cu_d, cu_h, labels, out=out["a"])
        elif name in "be":
            model.set_variants(5 if name == "b" else 7, 0)
            model.prefill_verbalize_packed(ids_d, cu_d, cu_h, labels, out=out[name])
            model.set_variants(0, 0)
        elif name == "c":
            extend(args_c, out["c"])
        elif name == "d":
            extend(args["d"], out["d"])
        else:
            model.set_variants(7, 0)
            if name == "g":
                os.environ[SEPARATE] = "1"   # read by the library per call
            extend(args[name], out[name])
            os.environ.pop(SEPARATE, None)
            model.set_variants(0, 0)

    for _ in range(3):
        for name in ARMS:
            arm(name)
    torch.cuda.synchronize()
    for name, ref in (("c", "a"), ("d", "a"), ("f", "e"), ("g", "e")):
        if not torch.equal(out[name], out[ref]):
            raise SystemExit(f"arm ({name}) does not give the scores of ({ref}): max diff "
                             f"{float((out[name] - out[ref]).abs().max()):.3e}")
    print(f"scores of (c) and (d) equal (a) bit for bit, those of (f) and (g) equal (e) bit for bit; (b) differs from (a) by at "
          f"most {float((out['b'] - out['a']).abs().max()):.3e}, (e) by {float((out['e'] - out['a']).abs().max()):.3e}")

    ms = {k: [] for k in ARMS}
    for _ in range(a.reps):
        for name in ARMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                arm(name)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.inner)
    what = {"a": "prefill_verbalize, default mode", "b": "prefill_verbalize, latency mode (variant 5)",
            "c": f"extend_verbalize, empty slot ({T} new)", "d": f"extend_verbalize, {c} cached + {a.new} new",
            "e": "prefill_verbalize, variant 7", "f": f"extend_verbalize, variant 7, {c} cached + {a.new} new",
            "g": "(f) with the separate cache write"}
    print(f"B = 1, {T} prompt tokens, {a.layers} layers, {a.reps} repeats x {a.inner} calls, arms alternating")
    for k in ARMS:
        v = np.array(ms[k])
        print(f"  ({k}) {what[k]:<48s} median {np.median(v):7.3f} ms  (min {v.min():.3f} .. max {v.max():.3f})")
    for num, den in (("d", "a"), ("d", "b"), ("c", "a"), ("c", "b"), ("f", "b"), ("f", "d"), ("e", "b"), ("f", "g"), ("f", "e")):
        r = np.array(ms[num]) / np.array(ms[den])
        print(f"  ({num}) / ({den}): median {np.median(r):.3f}  (min {r.min():.3f} .. max {r.max():.3f})")
    for num in "df":
        r = np.array(ms[num]) / np.array(ms["b"])
        print(f"  ({num}) beats (b) in every repeat" if r.max() < 1.0 else
              f"  ({num}) does NOT beat (b) outside the spread" if r.min() <= 1.0 else f"  ({num}) is slower than (b) in every repeat")
    print("  ranges of (f) and (b): " + ("disjoint" if max(ms["f"]) < min(ms["b"]) or max(ms["b"]) < min(ms["f"]) else "overlapping"))
    rfg = np.array(ms["f"]) / np.array(ms["g"])
    print("  (f) / (g): " + ("the fused cache write is faster in every repeat" if rfg.max() < 1.0 else
                             "the fused cache write is slower in every repeat" if rfg.min() > 1.0 else "inside the repeats' spread"))

    # kernel time by kind: the library's event profiler, in runs of their own (its events serialise the launches)
    n_prof = 5
    for name in "df":
        _lib.check(lib.lr_profile_start(n_prof * (a.layers * 16 + 32)), "lr_profile_start")
        for _ in range(n_prof):
            arm(name)
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
        print(f"({name}) kernel time by kind, per call ({total:.3f} ms in kernels; a product's launches count as one):")
        for label, t, n in rows:
            print(f"  {label:<18s} {t:7.3f} ms  {100 * t / total:5.1f} %  ({n} scopes)")


if __name__ == "__main__":
    main()
