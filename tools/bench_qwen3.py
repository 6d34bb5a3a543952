"""Qwen3 ranker timings on one MI355X (prints a table and one JSON line). One process, HIP events around every
timed call -- each timed step is the only GPU work between its two events -- the arms of a shape ALTERNATING inside every
repeat, median and min .. max of --reps (20) after warm-up launches of the same shape; the device name and its clock are
printed beside the numbers.
  1. the sweep alone (lr_qk_norm_rope_bf16) at M = 32 768 rows on the q | k widths of Qwen3-0.6B / 1.7B (16 + 8 heads of 128) and
     8B (32 + 8): ms and GB/s of the bytes it must move (every q / k element read and written once).
  2. a random-weight Qwen3-0.6B, 1.7B and 8B prefill + verbalizer (--layers as published) over a Beauty-sized token budget with
     the 36-token template prefix shared, on two arms of ONE handle: with its q/k norms (QKV products store plainly, the sweep
     follows) and after lr_llama_set_qk_norm(NULL, NULL) (Llama's layer: the rope epilogue). Their difference is the price of not
     fusing the norm into the epilogue; the split into GEMMs / attention / element-wise (the sweep, on this family the only
     kernel recorded there) is the library's own LrProfScope records.
  3. --train (instead of 1 and 2): a random-weight LoRA step (q_proj / v_proj, r = 8) on Qwen3-0.6B's shape over 16 prompts of
     460 .. 1 125 tokens, fwd + bwd ms per micro-batch with and without the norm pair, alternating on one engine.
Usage: python tools/bench_qwen3.py [--reps 20] [--m 32768] [--layers N] [--models 0.6b,1.7b,8b] [--no-sweep] [--no-step] [--train]"""
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
from tools.bench_qwen2 import _alternate, clock_mhz  # noqa: E402

T_ROPE = 2048
LR_PROF_ELEMENTWISE = 6


def _stats(t):
    return dict(ms_median=float(np.median(t)), ms_min=min(t), ms_max=max(t), reps=len(t))


def sweep_table(M, reps):
    L = lib()
    hd = 128
    cs = torch.empty(L.lr_rope_table_bytes(T_ROPE, hd) // 4, dtype=torch.float32, device="cuda")
    check(L.lr_rope_table(cs.data_ptr(), T_ROPE, hd, 1e6, stream_ptr()), "lr_rope_table")
    pos = (torch.arange(M, device="cuda", dtype=torch.int32) * 7) % T_ROPE
    g = torch.Generator(device="cuda").manual_seed(1)
    wq, wk = ((1.0 + torch.rand(hd, generator=g, device="cuda") - 0.5).to(torch.bfloat16) for _ in range(2))
    rows = {}
    for name, (nq, nk) in {"qwen3-0.6b/1.7b": (16, 8), "qwen3-8b": (32, 8)}.items():
        ld = (nq + 2 * nk) * hd
        src = torch.randn(M, ld, generator=g, device="cuda").to(torch.bfloat16)
        buf = src.clone()

        def run():
            rc = L.lr_qk_norm_rope_bf16(buf.data_ptr(), M, ld, 0, nq, nk, hd, wq.data_ptr(), wk.data_ptr(), 1e-6, pos.data_ptr(),
                                        cs.data_ptr(), stream_ptr())
            if rc:
                raise RuntimeError(f"lr_qk_norm_rope_bf16: {rc} {L.lr_last_error()}")

        t = _alternate({"sweep": run}, reps)["sweep"]   # in place: later repeats norm already-normed rows, the traffic is the same
        nbytes = 2.0 * M * (nq + nk) * hd * 2
        row = dict(M=M, nq=nq, nk=nk, head_dim=hd, bytes=nbytes, **_stats(t))
        row["gb_per_s"] = nbytes / row["ms_median"] / 1e6
        rows[name] = row
        print(f"sweep {name:16s} M={M} {nq}+{nk} heads of {hd}: {row['ms_median']:.3f} ms ({row['ms_min']:.3f} .. {row['ms_max']:.3f}), "
              f"{row['gb_per_s']:.0f} GB/s", flush=True)
    return rows


def _profile(L, run, layers, n=3):
    from tools.prefix_ab import _split

    check(L.lr_profile_start(n * (layers * 16 + 32)), "lr_profile_start")
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    check(L.lr_profile_stop(), "lr_profile_stop")
    split = _split(L, n)
    ms, work, cnt = C.c_double(), C.c_double(), C.c_int64()
    L.lr_profile_collect(LR_PROF_ELEMENTWISE, C.byref(ms), C.byref(work), C.byref(cnt))
    gemm = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("gemm"))
    attn = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("attention"))
    return gemm, attn, ms.value / n, work.value / n, cnt.value / n


def step(cfg, label, reps):
    from llamarec_amd.llm import LlamaRanker, common_prefix_len, pack_prompts
    from tools.prefix_ab import budget_prompts

    L = lib()
    seqs = budget_prompts(cfg, 1)
    ids, cu = pack_prompts(seqs)
    P = common_prefix_len(ids, cu)
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    lab = torch.arange(100, 120, dtype=torch.int32, device="cuda")
    model = LlamaRanker.random_init(cfg, seed=1)
    arms = ("qk_norm", "rope_epilogue")
    outs = {k: torch.empty(len(seqs), 20, dtype=torch.float32, device="cuda") for k in arms}

    def call(name):
        def run():
            qa, ka = model._qk_norm_arrs if name == "qk_norm" else (None, None)
            check(L.lr_llama_set_qk_norm(model._h, qa, ka), "lr_llama_set_qk_norm")
            model.prefill_verbalize_packed(ids_d, cu_d, cu, lab, out=outs[name], prefix_len=P)
        return run

    runs = {k: call(k) for k in arms}
    times = _alternate(runs, reps)
    layers = cfg["num_hidden_layers"]
    res = dict(prompts=len(seqs), tokens=int(cu[-1]), prefix=int(P), rows_shared=int(cu[-1] - (len(seqs) - 1) * P), layers=layers, arms={})
    for name in arms:
        gemm, attn, ew_ms, ew_bytes, ew_n = _profile(L, runs[name], layers)
        a = dict(**_stats(times[name]), gemm_ms=gemm, attention_ms=attn, sweep_ms=ew_ms, sweep_launches=ew_n,
                 sweep_gb_per_s=(ew_bytes / ew_ms / 1e6 if ew_ms else 0.0))
        a["sweep_share"] = ew_ms / a["ms_median"]
        a["ms_per_32k_rows"] = a["ms_median"] * 32768 / res["rows_shared"]
        res["arms"][name] = a
        assert torch.isfinite(outs[name]).all()
        print(f"{label} step ({name}): median {a['ms_median']:8.3f} ms (min {a['ms_min']:8.3f}, max {a['ms_max']:8.3f}, {reps} alternating "
              f"reps) = {a['ms_per_32k_rows']:.2f} ms per 32 k rows | GEMMs {gemm:7.2f} attention {attn:6.2f} sweep {ew_ms:6.3f} ms "
              f"({100 * a['sweep_share']:.2f} % of the step, {a['sweep_gb_per_s']:.0f} GB/s, {ew_n:.0f} launches)", flush=True)
    check(L.lr_llama_set_qk_norm(model._h, *model._qk_norm_arrs), "lr_llama_set_qk_norm")
    q, r = res["arms"]["qk_norm"], res["arms"]["rope_epilogue"]
    res["not_fusing_ms"] = q["ms_median"] - r["ms_median"]
    res["not_fusing_ratio"] = q["ms_median"] / r["ms_median"]
    res["ranges_disjoint"] = q["ms_min"] > r["ms_max"]
    res["sweep_over_attention"] = q["sweep_ms"] / q["attention_ms"] if q["attention_ms"] else None
    print(f"{label} step: {res['prompts']} prompts, {res['tokens']} tokens, prefix {P}: {res['rows_shared']} rows; norm + sweep against "
          f"the rope epilogue {res['not_fusing_ms']:+.3f} ms ({res['not_fusing_ratio']:.4f} x, ranges disjoint: {res['ranges_disjoint']}); "
          f"sweep / attention {res['sweep_over_attention']:.3f}", flush=True)
    return res


def lora_step(cfg, label, steps):
    """fwd + bwd ms per micro-batch of one engine with and without the base's q/k norms, alternating."""
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import LoraTrainEngine

    L = lib()
    ranker = LlamaRanker.random_init(cfg, seed=1)
    eng = LoraTrainEngine(ranker, dropout=0.05)
    init = eng.peft_init(3)
    for k in init:                    # non-zero B so that every kernel of the backward sees real numbers
        if k.endswith("lora_B"):
            init[k] = torch.randn(init[k].shape) * 0.01
    eng.load(init)
    rng = np.random.default_rng(0)
    lens = rng.integers(460, 1126, size=16)
    seqs = [np.concatenate([[1], rng.integers(3, cfg["vocab_size"], size=n - 2), [2]]).astype(np.int32) for n in lens]
    labels = []
    for s in seqs:
        l = s.copy()
        l[:-2] = -100
        labels.append(l)
    eng.loss_and_grads(seqs, labels)      # sizes the workspace with the save buffer of the norm pair

    def call(name):
        def run():
            qa, ka = ranker._qk_norm_arrs if name == "qk_norm" else (None, None)
            check(L.lr_llama_set_qk_norm(ranker._h, qa, ka), "lr_llama_set_qk_norm")
            eng.loss_and_grads(seqs, labels)
        return run

    times = _alternate({k: call(k) for k in ("qk_norm", "no_norm")}, max(steps, 5))
    check(L.lr_llama_set_qk_norm(ranker._h, *ranker._qk_norm_arrs), "lr_llama_set_qk_norm")
    res = dict(prompts=16, tokens=int(lens.sum()), layers=cfg["num_hidden_layers"], arms={k: _stats(t) for k, t in times.items()})
    q, r = res["arms"]["qk_norm"], res["arms"]["no_norm"]
    res["norm_pair_ms"] = q["ms_median"] - r["ms_median"]
    res["ratio"] = q["ms_median"] / r["ms_median"]
    print(f"{label} LoRA step, {res['tokens']} tokens, {res['layers']} layers: with the norm pair {q['ms_median']:.3f} ms "
          f"({q['ms_min']:.3f} .. {q['ms_max']:.3f}), without {r['ms_median']:.3f} ms ({r['ms_min']:.3f} .. {r['ms_max']:.3f}): "
          f"{res['norm_pair_ms']:+.3f} ms, {res['ratio']:.4f} x", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=0, help="layers of the step models (0: as published)")
    ap.add_argument("--models", type=str, default="0.6b,1.7b,8b")
    ap.add_argument("--no-sweep", action="store_true", help="skip table 1")
    ap.add_argument("--no-step", action="store_true", help="skip the whole steps")
    ap.add_argument("--train", action="store_true", help="the LoRA step instead")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    _lib.lib()
    from llamarec_amd.llm import QWEN3_0_6B, QWEN3_1_7B, QWEN3_8B

    p = torch.cuda.get_device_properties(0)
    box = dict(device=p.name, compute_units=p.multi_processor_count, clock_mhz=clock_mhz(),
               method=f"HIP events, one process, arms alternating, median of {args.reps}")
    print(f"box: {box['device']}, {box['compute_units']} CUs, clock {box['clock_mhz'] or 'not readable here'} MHz at start; "
          f"{box['method']}", flush=True)
    res = dict(box=box)
    layers = lambda c: dict(c, num_hidden_layers=args.layers or c["num_hidden_layers"])  # noqa: E731
    presets = {"0.6b": QWEN3_0_6B, "1.7b": QWEN3_1_7B, "8b": QWEN3_8B}
    if args.train:
        res["qwen3_0_6b_lora_step"] = lora_step(layers(QWEN3_0_6B), "qwen3-0.6b", args.steps)
    else:
        if not args.no_sweep:
            res["sweep"] = sweep_table(args.m, args.reps)
        if not args.no_step:
            for m in args.models.split(","):
                res[f"qwen3_{m.replace('.', '_')}_step"] = step(layers(presets[m]), f"qwen3-{m}", args.reps)
    box["clock_mhz_end"] = clock_mhz()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
