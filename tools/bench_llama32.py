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
  3. --train (instead of 1 and 2): the training side, attention variant 6.
     a. backward rows for the shapes of 1: variant 6 backward against variant 1 backward at head_dim 64 (same buffers), variant 2
        backward at head_dim 128 with (nh / 2, nkv / 2), and the forward writing lse (variant 6) against variant 5. TF/s of the
        backward as lr_launch_attention_bwd counts it (10 nh hd T (T + 1) / 2 per prompt), lr_launch_rowdot included.
     b. a random-weight Llama-3.2-1B LoRA step (q_proj / v_proj, r = 8) over 16 prompts of 460 .. 1 125 tokens: fwd+bwd ms per
        micro-batch with attention variant 1 and variant 6 ALTERNATING in one process on one engine (median, min .. max of
        --steps >= 5), then one profiled pass per variant for the attention share (LrProfScope records).
  4. --prefix-ab (instead of 1 and 2): the shared-prefix and last-row arms of tools/prefix_ab.py at head_dim 64 -- the prefix
     kernel against variant 5 on the same whole prompts, the last-row launch against full attention + gather, and the
     Llama-3.2-1B step with the 36-token prefix shared against prefix_len = 0 and against every --ab-lib build (the parent
     commit's library: its step on the same prompts), arms alternating, median and min .. max of --reps.
Usage: python tools/bench_llama32.py [--reps 30] [--steps 5] [--layers 16] [--ab-lib qt4=path/to/lib.so] [--train] [--prefix-ab]"""
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


def _timed(run, reps):
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
    return float(np.median(times))


def time_attention_train(nh, nkv, hd, T, B, reps, variants):
    """{("fwd", v) / ("fwd_lse", v) / ("bwd", v): ms} on one set of buffers; the backward reads the out / lse of ITS forward."""
    L = lib()
    n = B * T
    g = torch.Generator(device="cuda").manual_seed(T + nh)
    qw = (nh + 2 * nkv) * hd
    qkv = torch.randn(n, qw, generator=g, device="cuda").to(torch.bfloat16)
    d_out = torch.randn(n, nh * hd, generator=g, device="cuda").to(torch.bfloat16)
    out = torch.empty(n, nh * hd, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(n, nh, dtype=torch.float32, device="cuda")
    dqkv = torch.empty(n, qw, dtype=torch.bfloat16, device="cuda")
    cu = np.arange(0, n + 1, T, dtype=np.int32)
    cud = torch.from_numpy(cu).cuda()
    sb = L.lr_attention_bwd_scratch_bytes(n, nh, nkv, hd)
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    res, grads = {}, {}

    def call(name, rc):
        if rc:
            raise RuntimeError(f"{name}: {rc} {L.lr_last_error()}")

    for v in variants:
        if v == 5:
            res[("fwd", 5)] = _timed(lambda: call("fwd", L.lr_attention_varlen(
                qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, 5, stream_ptr())), reps)
            continue
        res[("fwd_lse", v)] = _timed(lambda: call("fwd_lse", L.lr_attention_varlen_lse(
            qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, v, stream_ptr())), reps)
        res[("bwd", v)] = _timed(lambda: call("bwd", L.lr_attention_varlen_bwd(
            qkv.data_ptr(), out.data_ptr(), d_out.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), cud.data_ptr(), cu.ctypes.data, B,
            nh, nkv, hd, v, scratch.data_ptr(), sb, stream_ptr())), reps)
        grads[v] = dqkv.float().clone()
    return res, grads


def attention_train_table(reps):
    rows = []
    for nh, nkv in ((32, 8), (24, 8)):
        for T in LENGTHS:
            r64, g = time_attention_train(nh, nkv, 64, T, PROMPTS, reps, (5, 6, 1))
            r128, _ = time_attention_train(nh // 2, nkv // 2, 128, T, PROMPTS, reps, (2,))
            work = 10.0 * nh * 64 * PROMPTS * T * (T + 1) / 2
            b6, b1, b2 = r64[("bwd", 6)], r64[("bwd", 1)], r128[("bwd", 2)]
            diff = float((g[6] - g[1]).abs().max() / g[1].abs().max())
            row = dict(nh=nh, nkv=nkv, T=T, B=PROMPTS, bwd_v6_ms=b6, bwd_v6_tflops=work / b6 / 1e9, bwd_generic_ms=b1,
                       bwd_generic_tflops=work / b1 / 1e9, bwd_v2_hd128_ms=b2, bwd_v2_hd128_tflops=work / b2 / 1e9,
                       bwd_v6_over_generic=b1 / b6, bwd_v6_over_v2=b2 / b6, fwd_v5_ms=r64[("fwd", 5)],
                       fwd_lse_v6_ms=r64[("fwd_lse", 6)], fwd_lse_generic_ms=r64[("fwd_lse", 1)],
                       max_rel_v6_minus_generic=diff)
            rows.append(row)
            print(f"attention bwd nh={nh:2d} nkv={nkv} {PROMPTS} x {T:4d}: v6 hd64 {b6:8.3f} ms {work / b6 / 1e9:6.1f} TF/s | generic hd64 "
                  f"{b1:9.3f} ms {work / b1 / 1e9:6.2f} TF/s | v2 hd128 {b2:8.3f} ms {work / b2 / 1e9:6.1f} TF/s | v6/generic "
                  f"{b1 / b6:6.1f}x v6/v2 {b2 / b6:4.2f} | fwd v5 {r64[('fwd', 5)]:7.3f} ms, fwd+lse v6 {r64[('fwd_lse', 6)]:7.3f} ms, "
                  f"fwd+lse generic {r64[('fwd_lse', 1)]:8.3f} ms | max |v6 - generic| / max {diff:.4f}", flush=True)
    return rows


def lora_step(cfg, label, variants, steps):
    """The LoRA fwd+bwd of a random-weight Llama-format model `cfg` (printed as `label`) with the attention `variants`
    alternating on one engine; tools/bench_phi3.py --train runs it at Phi-3-mini's shape."""
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import LoraTrainEngine

    layers = cfg["num_hidden_layers"]
    ranker = LlamaRanker.random_init(cfg, seed=1)
    eng = LoraTrainEngine(ranker, dropout=0.05)
    init = eng.peft_init(3)
    for k in init:                    # non-zero B so that every kernel of the backward sees real numbers
        if k.endswith("lora_B"):
            init[k] = torch.randn(init[k].shape) * 0.01
    eng.load(init)
    rng = np.random.default_rng(0)
    lens = rng.integers(460, 1126, size=PROMPTS)
    seqs = [np.concatenate([[1], rng.integers(3, cfg["vocab_size"], size=n - 2), [2]]).astype(np.int32) for n in lens]
    labels = []
    for s in seqs:
        l = s.copy()
        l[:-2] = -100
        labels.append(l)
    losses = {}
    for v in variants:                # warm-up of both, sizes the workspace
        ranker.set_variants(0, v)
        losses[v] = float(eng.loss_and_grads(seqs, labels))
    torch.cuda.synchronize()
    times = {v: [] for v in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(max(steps, 5)):
        for v in variants:
            ranker.set_variants(0, v)
            e0.record()
            eng.loss_and_grads(seqs, labels)
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1))
    L = lib()
    res = dict(prompts=PROMPTS, tokens=int(lens.sum()), layers=layers, min_len=int(lens.min()), max_len=int(lens.max()))
    for v in variants:                # one profiled pass per variant: the kernel split
        ranker.set_variants(0, v)
        check(L.lr_profile_start(3 * (layers * 64 + 64)), "lr_profile_start")
        e0.record()
        for _ in range(3):
            eng.loss_and_grads(seqs, labels)
        e1.record()
        torch.cuda.synchronize()
        check(L.lr_profile_stop(), "lr_profile_stop")
        prof_ms = e0.elapsed_time(e1) / 3
        split = {}
        for kind, name in KINDS.items():
            ms, work, n = C.c_double(), C.c_double(), C.c_int64()
            L.lr_profile_collect(kind, C.byref(ms), C.byref(work), C.byref(n))
            if n.value:
                split[name] = dict(ms_per_step=ms.value / 3, tflops=work.value / max(ms.value, 1e-9) / 1e9, launches_per_step=n.value / 3)
        attn = sum(x["ms_per_step"] for k, x in split.items() if k.startswith("attention"))
        gemm = sum(x["ms_per_step"] for k, x in split.items() if k.startswith("gemm"))
        t = times[v]
        res[f"variant_{v}"] = dict(fwd_bwd_ms_median=float(np.median(t)), fwd_bwd_ms_min=min(t), fwd_bwd_ms_max=max(t), steps=len(t),
                                   loss=losses[v], profiled_step_ms=prof_ms, kernels=split, attention_ms=attn, gemm_ms=gemm,
                                   attention_share=attn / prof_ms, gemm_share=gemm / prof_ms)
        print(f"{label} ({layers} layers, random weights) LoRA fwd+bwd, attention variant {v}: {PROMPTS} prompts of "
              f"{lens.min()} .. {lens.max()}, {lens.sum()} tokens: median {np.median(t):.2f} ms per micro-batch (min {min(t):.2f}, max "
              f"{max(t):.2f}, {len(t)} alternating steps); profiled pass {prof_ms:.2f} ms: attention {attn:.2f} ms "
              f"({100 * attn / prof_ms:.1f} %), GEMMs {gemm:.2f} ms ({100 * gemm / prof_ms:.1f} %), loss {losses[v]:.4f}", flush=True)
        for name, x in split.items():
            print(f"  {name:18s} {x['ms_per_step']:8.2f} ms/step {x['tflops']:7.1f} TF/s {x['launches_per_step']:6.1f} launches", flush=True)
    return res


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
    ap.add_argument("--train", action="store_true", help="the training side instead: backward rows and the LoRA step")
    ap.add_argument("--prefix-ab", action="store_true", help="the shared-prefix / last-row arms instead (tools/prefix_ab.py)")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    _lib.lib()
    p = torch.cuda.get_device_properties(0)
    box = dict(device=p.name, compute_units=p.multi_processor_count, clock_mhz=clock_mhz(),
               method=f"HIP events, one process, median of {args.reps}")
    print(f"box: {box['device']}, {box['compute_units']} CUs, clock {box['clock_mhz'] or 'not readable here'} MHz at start; {box['method']}", flush=True)
    if args.train:
        res = dict(box=box, attention_bwd=attention_train_table(args.reps))
        from llamarec_amd.llm import LLAMA32_1B

        res["llama32_1b_lora_step"] = lora_step(dict(LLAMA32_1B, num_hidden_layers=args.layers), "llama-3.2-1b", (1, 6), args.steps)
        box["clock_mhz_end"] = clock_mhz()
        print(json.dumps(res))
        return
    if args.prefix_ab:
        from llamarec_amd.llm import LLAMA32_1B
        from tools import prefix_ab

        builds = {spec.split("=", 1)[0]: prefix_ab.load_build(spec.split("=", 1)[1]) for spec in args.ab_lib}
        res = dict(box=box, attention_prefix=prefix_ab.attention_prefix_table(64, 5, ((32, 8), (24, 8)), args.reps))
        res["llama32_1b_prefix_ab"] = prefix_ab.step_ab(dict(LLAMA32_1B, num_hidden_layers=args.layers), 1, args.reps, builds,
                                                        "llama-3.2-1b")
        box["clock_mhz_end"] = clock_mhz()
        print(json.dumps(res))
        return
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
