"""Gemma-3 ranker timings on one MI355X (prints a table and one JSON line), modelled on tools/bench_gemma.py:
  1. attention: the windowed head_dim-256 MFMA kernel (lr_attention_varlen_window, variant 4) at W = 512 and W = 1 024 against
     variant 4 unwindowed on the same Beauty-length prompts (471 .. 1 125 tokens) at (nh, nkv) = (4, 1), one process, arms
     alternating inside every repeat, median and min .. max of --reps; TF/s counted on the IN-WINDOW work
     (4 nh hd sum_i min(i + 1, W) per prompt) and the time ratio against variant 4.
  2. the q/k norm + rotation sweep alone (norm_style 1) on the step's rows: us and GB/s.
  3. a random-weight step at Gemma-3-1B's shape (vocab 262 144, hidden 1 152, intermediate 6 912, --layers 26, 4 x 256 heads
     on 1 KV head, W = 512, pattern 6) over the Beauty token budget, prompts sharing a 36-token prefix: ms per step with its
     kernel split from the library's profile records (kind 6, element-wise, holds the sandwich-norm kernel AND the q/k sweep),
     then three arms alternating: the prompts whole (the handle drops the shared prefix: a prompt exceeds W), the same prompts
     clipped to W tokens with the prefix shared (the variant-4 prefix route), and clipped without sharing it.
Usage: python tools/bench_gemma3.py [--reps 20] [--steps 5] [--layers 26] [--no-step]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llamarec_amd._lib import check, lib, stream_ptr  # noqa: E402

KINDS = {0: "gemm 256-tile", 1: "gemm generic", 2: "attention MFMA", 3: "attention generic", 6: "element-wise (TB/s)"}
PREFIX = 36


def _event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(times):
    return dict(ms=float(np.median(times)), min_ms=float(np.min(times)), max_ms=float(np.max(times)))


def beauty_lengths(budget, rng):
    lens, total = [], 0
    while True:
        t = int(rng.integers(471, 1126))
        if total + t > budget:
            return lens
        lens.append(t)
        total += t


def window_attention_table(reps, nh=4, nkv=1, hd=256):
    from llamarec_amd.packing import TOKEN_BUDGET

    lens = beauty_lengths(TOKEN_BUDGET, np.random.default_rng(0))
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n, B = int(cu[-1]), len(lens)
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(n, (nh + 2 * nkv) * hd, generator=g, device="cuda").to(torch.bfloat16)
    out = torch.empty(n, nh * hd, dtype=torch.bfloat16, device="cuda")
    cud = torch.from_numpy(cu).cuda()

    def arm(W):
        return lambda: check(lib().lr_attention_varlen_window(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, 0,
                                                              nh, nkv, hd, W, 4, stream_ptr()), "attention")

    arms = {"v4": arm(0), "w512": arm(512), "w1024": arm(1024)}
    work = {k: 4.0 * nh * hd * sum(float(np.minimum(np.arange(1, t + 1), W or t).sum()) for t in lens)
            for k, W in (("v4", 0), ("w512", 512), ("w1024", 1024))}
    for run in arms.values():
        run()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, run in arms.items():
            times[k].append(_event_ms(run))
    st = {k: dict(_stats(v), tflops_in_window=work[k] / float(np.median(v)) / 1e9) for k, v in times.items()}
    for k in ("w512", "w1024"):
        st[k]["ratio_to_v4"] = st[k]["ms"] / st["v4"]["ms"]
        st[k]["ratio_range"] = [st[k]["min_ms"] / st["v4"]["max_ms"], st[k]["max_ms"] / st["v4"]["min_ms"]]
    print(f"window attention ({nh}, {nkv}) x {hd}, {B} prompts of 471 .. 1125 tokens ({n} rows):")
    for k, v in st.items():
        print(f"  {k:6s} {v['ms']:7.3f} ms ({v['min_ms']:.3f} .. {v['max_ms']:.3f}) {v['tflops_in_window']:6.1f} TF/s in-window"
              + (f"  ratio to v4 {v['ratio_to_v4']:.3f}" if "ratio_to_v4" in v else ""), flush=True)
    return dict(prompts=B, rows=n, **st)


def sweep_row(reps, rows, nh=4, nkv=1, hd=256):
    ld = (nh + 2 * nkv) * hd
    buf = torch.randn(rows, ld, device="cuda").to(torch.bfloat16)
    w = torch.zeros(hd, dtype=torch.bfloat16, device="cuda")
    pos = (torch.arange(rows, device="cuda") % 1000).to(torch.int32)
    cs = torch.empty(lib().lr_rope_table_bytes(1125, hd), dtype=torch.uint8, device="cuda")
    check(lib().lr_rope_table(cs.data_ptr(), 1125, hd, 10000.0, stream_ptr()), "lr_rope_table")

    def run():
        check(lib().lr_qk_norm_rope_ex_bf16(buf.data_ptr(), rows, ld, 0, nh, nkv, hd, w.data_ptr(), w.data_ptr(), 1e-6,
                                            pos.data_ptr(), cs.data_ptr(), stream_ptr(), 1), "sweep")

    for _ in range(3):
        run()
    st = _stats([_event_ms(run) for _ in range(reps)])
    st["gbytes_per_s"] = 2.0 * rows * (nh + nkv) * hd * 2 / st["ms"] / 1e6
    print(f"q/k norm sweep (norm_style 1) {rows} rows x {nh + nkv} heads of {hd}: {st['ms'] * 1e3:.1f} us "
          f"({st['min_ms'] * 1e3:.1f} .. {st['max_ms'] * 1e3:.1f}) {st['gbytes_per_s']:.0f} GB/s", flush=True)
    return st


def gemma3_step(steps, layers, reps):
    from llamarec_amd.llm import GEMMA3_1B, LlamaRanker, pack_prompts
    from llamarec_amd.packing import TOKEN_BUDGET

    cfg = dict(GEMMA3_1B, num_hidden_layers=layers)
    model = LlamaRanker.random_init(cfg, seed=1)
    W = cfg["sliding_window"]
    rng = np.random.default_rng(0)
    head = np.concatenate([[2], rng.integers(3, cfg["vocab_size"], size=PREFIX - 1)])
    whole = [np.concatenate([head, [3 + b], rng.integers(3 + 64, cfg["vocab_size"], size=t - PREFIX - 1)]).astype(np.int32)
             for b, t in enumerate(beauty_lengths(TOKEN_BUDGET, rng))]
    lab = torch.arange(100, 120, dtype=torch.int32, device="cuda")

    def packed(seqs):
        ids, cu = pack_prompts(seqs)
        return torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), cu

    sets = {"whole (prefix dropped)": (packed(whole), PREFIX), "clipped to W, prefix shared": (packed([s[:W] for s in whole]), PREFIX),
            "clipped to W, not shared": (packed([s[:W] for s in whole]), 0)}
    out = torch.empty(len(whole), 20, dtype=torch.float32, device="cuda")

    def arm(key):
        (ids_d, cu_d, cu), P = sets[key]
        return lambda: model.prefill_verbalize_packed(ids_d, cu_d, cu, lab, out=out, prefix_len=P)

    run = arm("whole (prefix dropped)")
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    L = lib()
    check(L.lr_profile_start(steps * (layers * 16 + 32)), "lr_profile_start")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    check(L.lr_profile_stop(), "lr_profile_stop")
    step_ms = e0.elapsed_time(e1) / steps
    split = {}
    for kind, kname in KINDS.items():
        ms, work, nl = C.c_double(), C.c_double(), C.c_int64()
        L.lr_profile_collect(kind, C.byref(ms), C.byref(work), C.byref(nl))
        if nl.value:
            split[kname] = dict(ms_per_step=ms.value / steps, share=ms.value / steps / step_ms,
                               tflops=work.value / max(ms.value, 1e-9) / 1e9, launches_per_step=nl.value / steps)
    assert torch.isfinite(out).all()
    tokens = int(sets["whole (prefix dropped)"][0][2][-1])
    print(f"gemma-3-1b shape ({layers} layers, random weights) prefill + verbalizer: {len(whole)} prompts, {tokens} tokens: "
          f"{step_ms:.2f} ms per step = {step_ms * 32768 / tokens:.2f} ms per 32 k rows", flush=True)
    for kname, v in split.items():
        print(f"  {kname:20s} {v['ms_per_step']:8.2f} ms/step {100 * v['share']:5.1f} % {v['tflops']:7.1f} TF/s "
              f"{v['launches_per_step']:6.1f} launches", flush=True)
    arms = {k: arm(k) for k in sets}
    for r in arms.values():
        r()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, r in arms.items():
            times[k].append(_event_ms(r))
    ab = {k: dict(_stats(v), tokens=int(sets[k][0][2][-1])) for k, v in times.items()}
    for k, v in ab.items():
        print(f"  step, {k:28s} {v['ms']:8.2f} ms ({v['min_ms']:.2f} .. {v['max_ms']:.2f}) {v['tokens']} tokens", flush=True)
    return dict(prompts=len(whole), tokens=tokens, layers=layers, step_ms=step_ms, ms_per_32k_rows=step_ms * 32768 / tokens,
                kernels=split, arms=ab)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from llamarec_amd.packing import TOKEN_BUDGET

    res = dict(window_attention=window_attention_table(args.reps), sweep=sweep_row(args.reps, TOKEN_BUDGET))
    if not args.no_step:
        res["step"] = gemma3_step(args.steps, args.layers, max(3, args.reps // 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
