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
  4. --train (instead of 1 and 2): the training side, attention variant 8.
     a. over 16 prompts of 5, 64, 129, 600 and 1 125 tokens, the backward of variant 8 at (32, 32) x 96 against the generic
        backward on the same buffers (the parent's code path at this head size; every fourth repeat) and, at equal width,
        variant 6 at (48, 48) x 64 and variant 2 at (24, 24) x 128; the forward of variant 7 against variant 8 writing lse
        and the generic kernel writing lse. Each backward reads the out / lse of its own forward. TF/s of the backward as
        lr_launch_attention_bwd counts it (10 nh hd T (T + 1) / 2 per prompt), lr_launch_rowdot included.
     b. a random-weight Llama-format model of Phi-3-mini's shape (hidden 3072, 32 x 96 heads, intermediate 8192, --layers):
        LoRA fwd+bwd (q_proj / v_proj, r = 8) over 16 prompts of 460 .. 1 125 tokens with attention variant 1 and auto
        (variant 8) alternating on one engine, then one profiled pass per arm for the attention / GEMM split
        (tools/bench_llama32.py's lora_step).
Usage: python tools/bench_phi3.py [--reps 20] [--layers 32] [--steps 5] [--prefix-ab] [--train] [--no-step]"""
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


TRAIN_LENGTHS = (5, 64, 129, 600, 1125)
# arm -> (nh, nkv, hd, variant, take every n-th repeat, what it times)
TRAIN_ARMS = {"bwd_v8_hd96": (32, 32, 96, 8, 1, "bwd"), "bwd_generic_hd96": (32, 32, 96, 1, 4, "bwd"),
              "bwd_v6_hd64": (48, 48, 64, 6, 1, "bwd"), "bwd_v2_hd128": (24, 24, 128, 2, 1, "bwd"),
              "fwd_v7_hd96": (32, 32, 96, 7, 1, "fwd"), "fwd_lse_v8_hd96": (32, 32, 96, 8, 1, "fwd_lse"),
              "fwd_lse_generic_hd96": (32, 32, 96, 1, 4, "fwd_lse")}
# Llama-format: what train_ranker.py --llm_base_model loads; Phi-3-mini's shape with the fused Linears already split
PHI3_SHAPE_LLAMA = dict(model_type="llama", vocab_size=32064, hidden_size=3072, intermediate_size=8192, num_hidden_layers=32,
                        num_attention_heads=32, num_key_value_heads=32, max_position_embeddings=4096, rms_norm_eps=1e-5,
                        rope_theta=10000.0, tie_word_embeddings=False)


def attention_train_table(reps):
    L = lib()
    rows = []

    def call(name, rc):
        if rc:
            raise RuntimeError(f"{name}: {rc} {L.lr_last_error()}")

    for T in TRAIN_LENGTHS:
        n = PROMPTS * T
        cu = np.arange(0, n + 1, T, dtype=np.int32)
        cud = torch.from_numpy(cu).cuda()
        g = torch.Generator(device="cuda").manual_seed(T)
        qkv = torch.randn(n, 3 * 3072, generator=g, device="cuda").to(torch.bfloat16)   # every arm: nh = nkv, width 3 x 3072
        d_out = torch.randn(n, 3072, generator=g, device="cuda").to(torch.bfloat16)
        runs, grads = {}, {}
        for name, (nh, nkv, hd, v, _, what) in TRAIN_ARMS.items():
            out = torch.empty(n, 3072, dtype=torch.bfloat16, device="cuda")
            lse = torch.empty(n, nh, dtype=torch.float32, device="cuda")
            head = (cud.data_ptr(), cu.ctypes.data, PROMPTS, nh, nkv, hd, v)

            def fwd_lse(out=out, lse=lse, head=head):
                call("lr_attention_varlen_lse", L.lr_attention_varlen_lse(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), *head,
                                                                          stream_ptr()))

            if what == "fwd":
                runs[name] = lambda out=out, head=head: call("lr_attention_varlen", L.lr_attention_varlen(
                    qkv.data_ptr(), out.data_ptr(), *head, stream_ptr()))
            elif what == "fwd_lse":
                runs[name] = fwd_lse
            else:
                fwd_lse()                                   # the backward reads the out / lse of ITS forward
                dqkv = torch.empty(n, 3 * 3072, dtype=torch.bfloat16, device="cuda")
                sb = L.lr_attention_bwd_scratch_bytes(n, nh, nkv, hd)
                scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
                grads[name] = dqkv
                runs[name] = lambda out=out, lse=lse, head=head, dqkv=dqkv, scratch=scratch, sb=sb: call(
                    "lr_attention_varlen_bwd", L.lr_attention_varlen_bwd(qkv.data_ptr(), out.data_ptr(), d_out.data_ptr(),
                                                                         lse.data_ptr(), dqkv.data_ptr(), *head,
                                                                         scratch.data_ptr(), sb, stream_ptr()))
        for name, r in runs.items():
            for _ in range(1 if "generic" in name else 3):
                r()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for i in range(reps):
            for name, r in runs.items():
                if i % TRAIN_ARMS[name][4]:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        pairs = 3072.0 * PROMPTS * T * (T + 1) / 2
        row = dict(T=T, B=PROMPTS)
        print(f"attention training {PROMPTS} x {T:4d}, nh hd = 3072:", flush=True)
        for name, t in times.items():
            work = (10.0 if TRAIN_ARMS[name][5] == "bwd" else 4.0) * pairs
            med = float(np.median(t))
            row[name] = dict(ms_median=med, ms_min=min(t), ms_max=max(t), reps=len(t), tflops=work / med / 1e9)
            print(f"  {name:22s} {med:9.3f} ms ({min(t):.3f} .. {max(t):.3f}, n={len(t)}) {work / med / 1e9:8.2f} TF/s", flush=True)
        g8, g1 = grads["bwd_v8_hd96"].float(), grads["bwd_generic_hd96"].float()
        row["bwd_v8_over_generic"] = row["bwd_generic_hd96"]["ms_median"] / row["bwd_v8_hd96"]["ms_median"]
        row["bwd_ranges_disjoint"] = row["bwd_v8_hd96"]["ms_max"] < row["bwd_generic_hd96"]["ms_min"]
        row["max_rel_v8_minus_generic"] = float((g8 - g1).abs().max() / g1.abs().max())
        rows.append(row)
        print(f"  v8 / generic backward {row['bwd_v8_over_generic']:.1f}x (ranges disjoint: {row['bwd_ranges_disjoint']}), "
              f"max |v8 - generic| / max {row['max_rel_v8_minus_generic']:.4f}", flush=True)
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
    ap.add_argument("--steps", type=int, default=5, help="--train: alternating LoRA steps per arm (at least 5)")
    ap.add_argument("--train", action="store_true", help="the training side instead: backward rows and the LoRA step")
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
    if args.train:
        from tools import bench_llama32

        res["attention_train"] = attention_train_table(args.reps)
        if not args.no_step:
            res["phi3_shape_lora_step"] = bench_llama32.lora_step(dict(PHI3_SHAPE_LLAMA, num_hidden_layers=args.layers),
                                                                  "llama-format model of phi-3-mini's shape", (1, 0), args.steps)
        box["clock_mhz_end"] = clock_mhz()
        print(json.dumps(res))
        return
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
