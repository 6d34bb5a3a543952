"""Qwen2 ranker timings on one MI355X (prints a table and one JSON line). One process, HIP events around every
timed call -- each timed step is the only GPU work between its two events -- the arms of a shape ALTERNATING inside every
repeat, median and min .. max of --reps (20) after warm-up launches of the same shape, on model-like operands (unit-variance
activations, weights of width 0.02); the device name and its clock are printed beside the numbers.
  1. the ragged products of Qwen2-0.5B at M = 32 768 -- qkv (N 1152, K 896, rope + bias), o (896 x 896, residual), down
     (896 x 4864, residual) -- on three arms: GEMM variant 6 (the 256-tile body on ceil(N / 256) column tiles), the generic
     kernel (variant 1: where auto sends these shapes) and the yardstick, variant 4 on B zero-padded to N = 1280 / 1024 / 1024.
     TF/s of the useful work 2 M N K for all three (the yardstick's executed rate is that times padded N over N).
  2. the bias: variant 4's rope epilogue with and without a bias at N = 4608, K = 3584 (Qwen2-7B's qkv), M = 32 768.
  3. a random-weight Qwen2-0.5B and Qwen2-1.5B prefill + verbalizer (--layers as published) over a Beauty-sized token budget
     with the 36-token template prefix shared, split into GEMMs / attention / rest from the library's own LrProfScope records;
     for 0.5B on two arms, the family default (GEMM variant 6) and GEMM variant 0 (auto: generic on the ragged products).
Usage: python tools/bench_qwen2.py [--reps 20] [--m 32768] [--layers N] [--no-gemm] [--no-step]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llamarec_amd import _lib  # noqa: E402
from llamarec_amd._lib import check, lib, stream_ptr  # noqa: E402

T_ROPE = 2048
# name: (N, K, epilogue, bias, head_dim, rot_cols)
RAGGED = {"qkv": (1152, 896, 3, True, 64, 1024), "o": (896, 896, 1, False, 0, 0), "down": (896, 4864, 1, False, 0, 0)}


def _alternate(runs, reps):
    for r in runs.values():
        for _ in range(3):
            r()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, r in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def _rope_table(hd):
    L = lib()
    cs = torch.empty(L.lr_rope_table_bytes(T_ROPE, hd) // 4, dtype=torch.float32, device="cuda")
    check(L.lr_rope_table(cs.data_ptr(), T_ROPE, hd, 1e6, stream_ptr()), "lr_rope_table")
    return cs


def _gemm_call(A, B, Cc, R, M, N, K, epi, variant, pos, cs, hd, rot_cols, bias):
    L = lib()

    def run():
        rc = L.lr_gemm_bf16_nt_bias_epi(A.data_ptr(), B.data_ptr(), Cc.data_ptr(), R.data_ptr() if R is not None else None, M, N, K,
                                        epi, variant, pos.data_ptr() if pos is not None else None,
                                        cs.data_ptr() if cs is not None else None, T_ROPE if cs is not None else 0, hd, rot_cols, None, 0,
                                        bias.data_ptr() if bias is not None else None, stream_ptr())
        if rc:
            raise RuntimeError(f"lr_gemm_bf16_nt_bias_epi: {rc} {L.lr_last_error()}")

    return run


def _summary(times, flops):
    out = {}
    for k, t in times.items():
        med = float(np.median(t))
        out[k] = dict(ms_median=med, ms_min=min(t), ms_max=max(t), reps=len(t), useful_tflops=flops / med / 1e9)
    return out


def ragged_table(M, reps):
    g = torch.Generator(device="cuda").manual_seed(1)
    pos = (torch.arange(M, device="cuda", dtype=torch.int32) * 7) % T_ROPE
    rows = {}
    for name, (N, K, epi, with_bias, hd, rot_cols) in RAGGED.items():
        Np = (N + 255) // 256 * 256
        A = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
        Bp = torch.zeros(Np, K, dtype=torch.bfloat16, device="cuda")
        Bp[:N] = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        B = Bp[:N].contiguous()
        biasp = torch.zeros(Np, dtype=torch.bfloat16, device="cuda")
        biasp[:N] = (torch.randn(N, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
        bias = biasp[:N].contiguous()
        cs = _rope_table(hd) if epi == 3 else None
        R = torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16) if epi == 1 else None
        Rp = torch.zeros(M, Np, dtype=torch.bfloat16, device="cuda") if epi == 1 else None
        if epi == 1:
            Rp[:, :N] = R
        C6, C1, C4 = (torch.empty(M, n, dtype=torch.bfloat16, device="cuda") for n in (N, N, Np))
        p = pos if epi == 3 else None
        runs = {"variant6": _gemm_call(A, B, C6, R, M, N, K, epi, 6, p, cs, hd, rot_cols, bias if with_bias else None),
                "generic": _gemm_call(A, B, C1, R, M, N, K, epi, 1, p, cs, hd, rot_cols, bias if with_bias else None),
                "padded_v4": _gemm_call(A, Bp, C4, Rp, M, Np, K, epi, 4, p, cs, hd, rot_cols, biasp if with_bias else None)}
        times = _alternate(runs, reps)
        row = dict(M=M, N=N, K=K, N_padded=Np, epilogue=epi, bias=with_bias, arms=_summary(times, 2.0 * M * N * K))
        row["same_bits_as_padded_v4"] = bool(torch.equal(C6, C4[:, :N]))
        row["max_abs_minus_generic"] = float((C6.float() - C1.float()).abs().max())
        a = row["arms"]
        row["generic_over_variant6"] = a["generic"]["ms_median"] / a["variant6"]["ms_median"]
        row["variant6_over_padded_v4"] = a["variant6"]["ms_median"] / a["padded_v4"]["ms_median"]
        row["ranges_disjoint_vs_generic"] = a["variant6"]["ms_max"] < a["generic"]["ms_min"]
        rows[name] = row
        print(f"{name:5s} M={M} N={N} K={K} epi {epi}{' + bias' if with_bias else ''}: " +
              " | ".join(f"{k} {v['ms_median']:.3f} ms ({v['ms_min']:.3f} .. {v['ms_max']:.3f}) {v['useful_tflops']:.0f} useful TF/s"
                         for k, v in a.items()) +
              f" | generic / v6 {row['generic_over_variant6']:.2f}x, v6 / padded v4 {row['variant6_over_padded_v4']:.3f}, "
              f"v6 == padded v4 bits: {row['same_bits_as_padded_v4']}, max |v6 - generic| {row['max_abs_minus_generic']:.4f}", flush=True)
    return rows


def bias_cost(M, reps):
    N, K, hd, rot_cols = 4608, 3584, 128, 4096
    g = torch.Generator(device="cuda").manual_seed(2)
    A = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    pos = (torch.arange(M, device="cuda", dtype=torch.int32) * 7) % T_ROPE
    cs = _rope_table(hd)
    C0, C1 = (torch.empty(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    runs = {"rope": _gemm_call(A, B, C0, None, M, N, K, 3, 4, pos, cs, hd, rot_cols, None),
            "rope_bias": _gemm_call(A, B, C1, None, M, N, K, 3, 4, pos, cs, hd, rot_cols, bias)}
    times = _alternate(runs, reps)
    row = dict(M=M, N=N, K=K, arms=_summary(times, 2.0 * M * N * K))
    a = row["arms"]
    row["bias_over_plain"] = a["rope_bias"]["ms_median"] / a["rope"]["ms_median"]
    print(f"bias  M={M} N={N} K={K} variant 4 rope: " +
          " | ".join(f"{k} {v['ms_median']:.3f} ms ({v['ms_min']:.3f} .. {v['ms_max']:.3f}) {v['useful_tflops']:.0f} TF/s" for k, v in a.items()) +
          f" | with / without {row['bias_over_plain']:.4f}", flush=True)
    return row


def step(cfg, label, reps, arms):
    """arms: {name: GEMM variant}. One model, the variant switched in front of every call."""
    from llamarec_amd.llm import LlamaRanker, common_prefix_len, pack_prompts
    from tools.prefix_ab import _split, budget_prompts

    seqs = budget_prompts(cfg, 1)
    ids, cu = pack_prompts(seqs)
    P = common_prefix_len(ids, cu)
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    lab = torch.arange(100, 120, dtype=torch.int32, device="cuda")
    model = LlamaRanker.random_init(cfg, seed=1)
    outs = {k: torch.empty(len(seqs), 20, dtype=torch.float32, device="cuda") for k in arms}

    def call(name):
        def run():
            model.set_variants(arms[name], 0)
            model.prefill_verbalize_packed(ids_d, cu_d, cu, lab, out=outs[name], prefix_len=P)
        return run

    runs = {k: call(k) for k in arms}
    times = _alternate(runs, reps)
    L = lib()
    res = dict(prompts=len(seqs), tokens=int(cu[-1]), prefix=int(P), rows_shared=int(cu[-1] - (len(seqs) - 1) * P), reps=reps,
               layers=cfg["num_hidden_layers"], arms={})
    for name in arms:
        check(L.lr_profile_start(3 * (cfg["num_hidden_layers"] * 12 + 32)), "lr_profile_start")
        for _ in range(3):
            runs[name]()
        torch.cuda.synchronize()
        check(L.lr_profile_stop(), "lr_profile_stop")
        split = _split(L, 3)
        gemm = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("gemm"))
        attn = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("attention"))
        t = times[name]
        med = float(np.median(t))
        first = next(iter(arms))
        res["arms"][name] = dict(gemm_variant=arms[name], ms_median=med, ms_min=min(t), ms_max=max(t), gemm_ms=gemm, attention_ms=attn,
                                 rest_ms=med - gemm - attn, kernels=split,
                                 max_abs_minus_first_arm=float((outs[name] - outs[first]).abs().max()))
        assert torch.isfinite(outs[name]).all()
        print(f"{label} step, GEMM variant {arms[name]} ({name}): median {med:8.3f} ms (min {min(t):8.3f}, max {max(t):8.3f}, {reps} "
              f"alternating reps) | GEMMs {gemm:7.2f} attention {attn:6.2f} rest {med - gemm - attn:6.2f} ms | "
              f"{len(seqs) / med * 1e3:.1f} prompts/s | max |scores - {first}| {res['arms'][name]['max_abs_minus_first_arm']:.4f}", flush=True)
    print(f"{label} step: {res['prompts']} prompts, {res['tokens']} tokens, prefix {P}: {res['rows_shared']} rows", flush=True)
    return res


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(0))
    except Exception:   # no SMI binding in this Python: say so instead of guessing
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=0, help="layers of the step models (0: as published)")
    ap.add_argument("--no-gemm", action="store_true", help="skip tables 1 and 2")
    ap.add_argument("--no-step", action="store_true", help="skip the whole steps")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    _lib.lib()
    from llamarec_amd.llm import QWEN2_0_5B, QWEN2_1_5B

    p = torch.cuda.get_device_properties(0)
    box = dict(device=p.name, compute_units=p.multi_processor_count, clock_mhz=clock_mhz(),
               method=f"HIP events, one process, arms alternating, median of {args.reps}")
    print(f"box: {box['device']}, {box['compute_units']} CUs, clock {box['clock_mhz'] or 'not readable here'} MHz at start; "
          f"{box['method']}", flush=True)
    res = dict(box=box)
    if not args.no_gemm:
        res["ragged"] = ragged_table(args.m, args.reps)
        res["bias"] = bias_cost(args.m, args.reps)
    if not args.no_step:
        layers = lambda c: dict(c, num_hidden_layers=args.layers or c["num_hidden_layers"])  # noqa: E731
        res["qwen2_0_5b_step"] = step(layers(QWEN2_0_5B), "qwen2-0.5b", args.reps, {"default": 6, "auto": 0})
        res["qwen2_1_5b_step"] = step(layers(QWEN2_1_5B), "qwen2-1.5b", args.reps, {"default": 6})
    box["clock_mhz_end"] = clock_mhz()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
