"""Gemma ranker timings on one MI355X (prints a table and one JSON line):
  1. attention: variant 4 (head_dim-256 MFMA) against the generic kernel at head_dim 256 and variant 2 at head_dim 128, on
     16 x 600 and 16 x 1 125-token batches at (nh, nkv) = (8, 1) and (16, 16); TF/s of the causal work as
     lr_launch_attention counts it (4 nh hd T (T + 1) / 2 per prompt), same process, median of the timed repeats.
  2. a random-weight Gemma-2B prefill + verbalizer over a Beauty-sized token budget (prompts of 460 .. 1 125 tokens,
     packing.TOKEN_BUDGET rows): ms per step and its kernel split from the library's LrProfScope records.
  3. --prefix-ab (instead of 1 and 2): the shared-prefix and last-row arms of tools/prefix_ab.py at head_dim 256 -- the prefix
     kernel against variant 4 on the same whole prompts, the last-row launch against full attention + gather, and the Gemma-2B
     step with the 36-token prefix shared against prefix_len = 0 and against every --ab-lib NAME=PATH build (the parent commit's
     library: its step on the same prompts), arms alternating, median and min .. max of --reps.
  4. --gemma2 (instead of 1 and 2): Gemma-2. The soft-capped head_dim-256 kernel against variant 4 uncapped and against the
     generic kernel with the cap on the same rows, arms alternating, median and min .. max of --reps (the generic arm: a
     quarter of them); the sandwich-norm kernel's GB/s at the step's row count; a random-weight Gemma-2-2B step (26 layers) on
     the Beauty token budget with its kernel split (the element-wise kernel from its own profile records).
  5. --train (instead of 1 and 2): the training side at head_dim 256, attention variant 9.
     a. over 16 prompts of 5, 64, 129, 600 and 1 125 tokens, one process, HIP events, the arms of a shape ALTERNATING inside
        every repeat, median and min .. max of --reps: the backward of variant 9 at (8, 1) x 256 and (16, 16) x 256 against the
        generic backward on the same buffers (what this route ran before variant 9; every fourth repeat, being slow), and at
        equal width nh hd = 2048 variant 9 at (8, 8) x 256 against variant 2 at (16, 16) x 128; the forward of variant 4 against
        variant 9 writing lse and the generic kernel writing lse. Each backward reads the out / lse of its own forward. TF/s of
        the backward as lr_launch_attention_bwd counts it (10 nh hd T (T + 1) / 2 per prompt), lr_launch_rowdot included.
     b. a random-weight Llama-format model of Gemma-2B's shape (hidden 2048, 8 x 256 heads on 1 KV head, intermediate 16384,
        --layers 18): LoRA fwd+bwd (q_proj / v_proj, r = 8) over 16 prompts of 460 .. 1 125 tokens with attention variant 1 and
        auto (variant 9) alternating on one engine, then one profiled pass per arm for the attention / GEMM split
        (tools/bench_llama32.py's lora_step).
Usage: python tools/bench_gemma.py [--reps 20] [--steps 5] [--layers 18] [--prefix-ab] [--gemma2] [--train] [--no-step]
       [--ab-lib parent=path/to/lib.so]"""
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

# kind 6's work is bytes, so its "TF/s" column reads TB/s
KINDS = {0: "gemm 256-tile", 1: "gemm generic", 2: "attention MFMA", 3: "attention generic", 6: "sandwich norm (TB/s)"}


def time_attention(nh, nkv, hd, T, B, variant, reps):
    n = B * T
    g = torch.Generator(device="cuda").manual_seed(T + nh)
    qkv = torch.randn(n, (nh + 2 * nkv) * hd, generator=g, device="cuda").to(torch.bfloat16)
    out = torch.empty(n, nh * hd, dtype=torch.bfloat16, device="cuda")
    cu = np.arange(0, n + 1, T, dtype=np.int32)
    cud = torch.from_numpy(cu).cuda()

    def run():
        check(lib().lr_attention_varlen(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, variant,
                                        stream_ptr()), "attention")

    for _ in range(3):
        run()
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
    return ms, work / ms / 1e9


def attention_table(reps):
    rows = []
    for nh, nkv in ((8, 1), (16, 16)):
        for T in (600, 1125):
            ms4, tf4 = time_attention(nh, nkv, 256, T, 16, 4, reps)
            ms1, tf1 = time_attention(nh, nkv, 256, T, 16, 1, max(3, reps // 4))
            ms2, tf2 = time_attention(nh, nkv, 128, T, 16, 2, reps)
            rows.append(dict(nh=nh, nkv=nkv, T=T, B=16, v4_ms=ms4, v4_tflops=tf4, generic_ms=ms1, generic_tflops=tf1,
                             v2_hd128_ms=ms2, v2_hd128_tflops=tf2, v4_over_generic=ms1 / ms4, v4_over_v2=tf4 / tf2))
            print(f"attention nh={nh:2d} nkv={nkv:2d} 16 x {T:4d}: v4 hd256 {ms4:7.3f} ms {tf4:6.1f} TF/s | generic hd256 "
                  f"{ms1:8.3f} ms {tf1:6.1f} TF/s | v2 hd128 {ms2:7.3f} ms {tf2:6.1f} TF/s | v4/generic {ms1 / ms4:5.1f}x "
                  f"v4/v2 {tf4 / tf2:4.2f}", flush=True)
    return rows


def _event_ms(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _stats(times):
    return dict(ms=float(np.median(times)), min_ms=float(np.min(times)), max_ms=float(np.max(times)))


def softcap_attention_table(reps, cap=50.0):
    """Capped MFMA kernel | variant 4 uncapped | generic kernel with the cap, same rows, arms alternating."""
    rows = []
    for nh, nkv in ((8, 1), (16, 16), (8, 4), (16, 8)):
        for T in (600, 1125):
            B, hd = 16, 256
            n = B * T
            g = torch.Generator(device="cuda").manual_seed(T + nh)
            qkv = torch.randn(n, (nh + 2 * nkv) * hd, generator=g, device="cuda").to(torch.bfloat16)
            out = torch.empty(n, nh * hd, dtype=torch.bfloat16, device="cuda")
            cu = np.arange(0, n + 1, T, dtype=np.int32)
            cud = torch.from_numpy(cu).cuda()

            def arm(c, variant):
                return lambda: check(lib().lr_attention_varlen_softcap(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(),
                                                                       cu.ctypes.data, B, 0, nh, nkv, hd, 0.0, c, variant,
                                                                       stream_ptr()), "attention")

            arms = dict(capped=arm(cap, 4), v4=arm(0.0, 4), generic_capped=arm(cap, 1))
            for run in arms.values():
                run()
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for i in range(reps):
                for k, run in arms.items():
                    if k != "generic_capped" or i % 4 == 0:
                        times[k].append(_event_ms(run))
            work = 4.0 * nh * hd * B * T * (T + 1) / 2
            st = {k: _stats(v) for k, v in times.items()}
            row = dict(nh=nh, nkv=nkv, T=T, B=B, cap=cap, **{k: dict(v, tflops=work / v["ms"] / 1e9) for k, v in st.items()},
                       capped_over_v4=st["capped"]["ms"] / st["v4"]["ms"],
                       generic_over_capped=st["generic_capped"]["ms"] / st["capped"]["ms"])
            rows.append(row)
            print(f"softcap attention nh={nh:2d} nkv={nkv:2d} 16 x {T:4d}: capped {st['capped']['ms']:7.3f} ms "
                  f"({st['capped']['min_ms']:.3f} .. {st['capped']['max_ms']:.3f}) {row['capped']['tflops']:6.1f} TF/s | v4 "
                  f"{st['v4']['ms']:7.3f} ms ({st['v4']['min_ms']:.3f} .. {st['v4']['max_ms']:.3f}) {row['v4']['tflops']:6.1f} TF/s | "
                  f"generic capped {st['generic_capped']['ms']:8.3f} ms | capped/v4 {row['capped_over_v4']:4.2f} "
                  f"generic/capped {row['generic_over_capped']:5.1f}x", flush=True)
    return rows


def postnorm_table(reps, rows_n):
    """The sandwich-norm kernel alone: with the next norm (3 row reads + 2 row writes of 2 d bytes) and without (2 + 1)."""
    res = []
    for d in (2304, 3584):
        g = torch.Generator(device="cuda").manual_seed(d)
        x = torch.randn(rows_n, d, generator=g, device="cuda").to(torch.bfloat16)
        h = torch.randn(rows_n, d, generator=g, device="cuda").to(torch.bfloat16)
        w = torch.zeros(2, d, dtype=torch.bfloat16, device="cuda")
        arms = dict(
            with_next=lambda: check(lib().lr_residual_postnorm_bf16(x.data_ptr(), h.data_ptr(), w[0].data_ptr(), w[1].data_ptr(),
                                                                    h.data_ptr(), rows_n, d, 1e-6, stream_ptr()), "postnorm"),
            without_next=lambda: check(lib().lr_residual_postnorm_bf16(x.data_ptr(), h.data_ptr(), w[0].data_ptr(), None, None,
                                                                       rows_n, d, 1e-6, stream_ptr()), "postnorm"),
            rmsnorm=lambda: check(lib().lr_rmsnorm_bf16(x.data_ptr(), w[1].data_ptr(), h.data_ptr(), rows_n, d, 1e-6, 1,
                                                        stream_ptr()), "rmsnorm"))

        def three_launches():      # the unfused form: norm(h) -> h, x += h (torch's add stands in: the library has none), norm(x)
            check(lib().lr_rmsnorm_bf16(h.data_ptr(), w[0].data_ptr(), h.data_ptr(), rows_n, d, 1e-6, 1, stream_ptr()), "rmsnorm")
            x.add_(h)
            check(lib().lr_rmsnorm_bf16(x.data_ptr(), w[1].data_ptr(), h.data_ptr(), rows_n, d, 1e-6, 1, stream_ptr()), "rmsnorm")

        def two_launches():        # norm + add fused, the next norm on its own
            arms["without_next"]()
            arms["rmsnorm"]()

        arms["three_launches"], arms["two_launches"] = three_launches, two_launches
        for run in arms.values():
            run()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(reps):
            for k, run in arms.items():
                times[k].append(_event_ms(run))
        row = dict(d=d, rows=rows_n)
        for k, passes in (("with_next", 5), ("without_next", 3), ("rmsnorm", 2), ("two_launches", 5), ("three_launches", 7)):
            st = _stats(times[k])
            row[k] = dict(st, gbytes_per_s=passes * rows_n * d * 2 / st["ms"] / 1e6)
        res.append(row)
        print(f"sandwich norm {rows_n} x {d}: with the next norm {row['with_next']['ms'] * 1e3:7.1f} us "
              f"({row['with_next']['min_ms'] * 1e3:.1f} .. {row['with_next']['max_ms'] * 1e3:.1f}) "
              f"{row['with_next']['gbytes_per_s']:6.0f} GB/s | without {row['without_next']['ms'] * 1e3:7.1f} us "
              f"{row['without_next']['gbytes_per_s']:6.0f} GB/s | rmsnorm alone {row['rmsnorm']['ms'] * 1e3:7.1f} us | "
              f"without + rmsnorm {row['two_launches']['ms'] * 1e3:7.1f} us ({row['two_launches']['min_ms'] * 1e3:.1f} .. "
              f"{row['two_launches']['max_ms'] * 1e3:.1f}) | rmsnorm, add, rmsnorm {row['three_launches']['ms'] * 1e3:7.1f} us "
              f"({row['three_launches']['min_ms'] * 1e3:.1f} .. {row['three_launches']['max_ms'] * 1e3:.1f})", flush=True)
    return res


def gemma2b_step(steps, layers, base=None, name="gemma-2b"):
    from llamarec_amd.llm import GEMMA_2B, LlamaRanker, pack_prompts
    from llamarec_amd.packing import TOKEN_BUDGET

    cfg = dict(base or GEMMA_2B, num_hidden_layers=layers)
    model = LlamaRanker.random_init(cfg, seed=1)
    rng = np.random.default_rng(0)
    seqs, total = [], 0
    while True:
        t = int(rng.integers(460, 1126))
        if total + t > TOKEN_BUDGET:
            break
        seqs.append(np.concatenate([[2], rng.integers(3, cfg["vocab_size"], size=t - 1)]).astype(np.int32))
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
    for kind, kname in KINDS.items():
        ms, work, n = C.c_double(), C.c_double(), C.c_int64()
        L.lr_profile_collect(kind, C.byref(ms), C.byref(work), C.byref(n))
        if n.value:
            split[kname] = dict(ms_per_step=ms.value / steps, tflops=work.value / max(ms.value, 1e-9) / 1e9,
                               launches_per_step=n.value / steps)
    assert torch.isfinite(out).all()
    print(f"{name} ({layers} layers, random weights) prefill + verbalizer: {len(seqs)} prompts, {total} tokens: "
          f"{step_ms:.2f} ms per step", flush=True)
    for kname, v in split.items():
        print(f"  {kname:18s} {v['ms_per_step']:8.2f} ms/step {v['tflops']:7.1f} TF/s {v['launches_per_step']:6.1f} launches",
              flush=True)
    attn = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("attention"))
    return dict(prompts=len(seqs), tokens=total, layers=layers, step_ms=step_ms, kernels=split,
                attention_share=attn / step_ms)


TRAIN_LENGTHS = (5, 64, 129, 600, 1125)
TRAIN_PROMPTS = 16
# group -> arm -> (nh, nkv, hd, variant, take every n-th repeat, what it times); the arms of a group share one qkv / d_out
TRAIN_GROUPS = {
    "(8, 1) x 256": {"bwd_v9": (8, 1, 256, 9, 1, "bwd"), "bwd_generic": (8, 1, 256, 1, 4, "bwd"),
                     "fwd_v4": (8, 1, 256, 4, 1, "fwd"), "fwd_lse_v9": (8, 1, 256, 9, 1, "fwd_lse"),
                     "fwd_lse_generic": (8, 1, 256, 1, 4, "fwd_lse")},
    "(16, 16) x 256": {"bwd_v9": (16, 16, 256, 9, 1, "bwd"), "bwd_generic": (16, 16, 256, 1, 4, "bwd"),
                       "fwd_v4": (16, 16, 256, 4, 1, "fwd"), "fwd_lse_v9": (16, 16, 256, 9, 1, "fwd_lse"),
                       "fwd_lse_generic": (16, 16, 256, 1, 4, "fwd_lse")},
    "width 2048": {"bwd_v9_hd256": (8, 8, 256, 9, 1, "bwd"), "bwd_v2_hd128": (16, 16, 128, 2, 1, "bwd"),
                   "fwd_lse_v9_hd256": (8, 8, 256, 9, 1, "fwd_lse"), "fwd_lse_v2_hd128": (16, 16, 128, 2, 1, "fwd_lse")},
}
# Llama-format: what train_ranker.py --llm_base_model loads; Gemma-2B's shape with Llama's arithmetic
GEMMA2B_SHAPE_LLAMA = dict(model_type="llama", vocab_size=32000, hidden_size=2048, intermediate_size=16384, num_hidden_layers=18,
                           num_attention_heads=8, num_key_value_heads=1, head_dim=256, max_position_embeddings=4096,
                           rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=False)


def attention_train_table(reps):
    L = lib()
    rows = []
    B = TRAIN_PROMPTS

    def call(name, rc):
        if rc:
            raise RuntimeError(f"{name}: {rc} {L.lr_last_error()}")

    for group, arms in TRAIN_GROUPS.items():
        for T in TRAIN_LENGTHS:
            n = B * T
            cu = np.arange(0, n + 1, T, dtype=np.int32)
            cud = torch.from_numpy(cu).cuda()
            g = torch.Generator(device="cuda").manual_seed(T)
            qw = max((nh + 2 * nkv) * hd for nh, nkv, hd, *_ in arms.values())
            ow = max(nh * hd for nh, nkv, hd, *_ in arms.values())
            assert all((nh + 2 * nkv) * hd == qw and nh * hd == ow for nh, nkv, hd, *_ in arms.values())
            qkv = torch.randn(n, qw, generator=g, device="cuda").to(torch.bfloat16)
            d_out = torch.randn(n, ow, generator=g, device="cuda").to(torch.bfloat16)
            runs, grads = {}, {}
            for name, (nh, nkv, hd, v, _, what) in arms.items():
                out = torch.empty(n, ow, dtype=torch.bfloat16, device="cuda")
                lse = torch.empty(n, nh, dtype=torch.float32, device="cuda")
                head = (cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd, v)

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
                    dqkv = torch.empty(n, qw, dtype=torch.bfloat16, device="cuda")
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
                    if i % arms[name][4] == 0:
                        times[name].append(_event_ms(r))
            pairs = float(ow) * B * T * (T + 1) / 2
            row = dict(group=group, T=T, B=B)
            print(f"attention training {group}, {B} x {T:4d}:", flush=True)
            for name, t in times.items():
                work = (10.0 if arms[name][5] == "bwd" else 4.0) * pairs
                med = float(np.median(t))
                row[name] = dict(ms_median=med, ms_min=min(t), ms_max=max(t), reps=len(t), tflops=work / med / 1e9)
                print(f"  {name:20s} {med:9.3f} ms ({min(t):.3f} .. {max(t):.3f}, n={len(t)}) {work / med / 1e9:8.2f} TF/s", flush=True)
            if "bwd_generic" in row:
                g9, g1 = grads["bwd_v9"].float(), grads["bwd_generic"].float()
                row["bwd_v9_over_generic"] = row["bwd_generic"]["ms_median"] / row["bwd_v9"]["ms_median"]
                row["bwd_ranges_disjoint"] = row["bwd_v9"]["ms_max"] < row["bwd_generic"]["ms_min"]
                row["fwd_lse_inside_v4_range"] = row["fwd_v4"]["ms_min"] <= row["fwd_lse_v9"]["ms_median"] <= row["fwd_v4"]["ms_max"]
                row["max_rel_v9_minus_generic"] = float((g9 - g1).abs().max() / g1.abs().max())
                print(f"  v9 / generic backward {row['bwd_v9_over_generic']:.1f}x (ranges disjoint: {row['bwd_ranges_disjoint']}), "
                      f"fwd+lse median inside variant 4's min .. max: {row['fwd_lse_inside_v4_range']}, "
                      f"max |v9 - generic| / max {row['max_rel_v9_minus_generic']:.4f}", flush=True)
            else:
                row["bwd_v9_over_v2_tflops"] = row["bwd_v9_hd256"]["tflops"] / row["bwd_v2_hd128"]["tflops"]
                print(f"  v9 hd256 / v2 hd128 backward TF/s {row['bwd_v9_over_v2_tflops']:.2f}", flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--prefix-ab", action="store_true", help="the shared-prefix / last-row arms instead (tools/prefix_ab.py)")
    ap.add_argument("--gemma2", action="store_true", help="the Gemma-2 tables instead: capped attention, sandwich norm, 2B step")
    ap.add_argument("--train", action="store_true", help="the training side instead: variant 9's backward rows and the LoRA step")
    ap.add_argument("--no-step", action="store_true", help="--train: skip the LoRA step")
    ap.add_argument("--ab-lib", action="append", default=[], metavar="NAME=PATH")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    _lib.lib()
    if args.train:
        from tools import bench_llama32

        p = torch.cuda.get_device_properties(0)
        res = dict(box=dict(device=p.name, compute_units=p.multi_processor_count,
                            method=f"HIP events, one process, arms alternating, median of {args.reps}"))
        print(f"box: {p.name}, {p.multi_processor_count} CUs; {res['box']['method']}", flush=True)
        res["attention_train"] = attention_train_table(args.reps)
        if not args.no_step:
            res["gemma2b_shape_lora_step"] = bench_llama32.lora_step(dict(GEMMA2B_SHAPE_LLAMA, num_hidden_layers=args.layers),
                                                                     "llama-format model of gemma-2b's shape", (1, 0), args.steps)
        print(json.dumps(res))
        return
    if args.gemma2:
        from llamarec_amd.llm import GEMMA2_2B
        from llamarec_amd.packing import TOKEN_BUDGET

        res = dict(softcap_attention=softcap_attention_table(args.reps))
        res["sandwich_norm"] = postnorm_table(args.reps, TOKEN_BUDGET)
        layers = 26 if args.layers == 18 else args.layers      # the default is Gemma-2B's 18; gemma-2-2b has 26
        step = gemma2b_step(args.steps, layers, GEMMA2_2B, "gemma-2-2b")
        # the element-wise kernel's own profile records (kind 6), inside the step
        step["sandwich_norm_ms_per_step"] = sum(v["ms_per_step"] for k, v in step["kernels"].items() if k.startswith("sandwich"))
        step["sandwich_norm_share"] = step["sandwich_norm_ms_per_step"] / step["step_ms"]
        gemm = sum(v["ms_per_step"] for k, v in step["kernels"].items() if k.startswith("gemm"))
        step["gemm_share"] = gemm / step["step_ms"]
        step["rest_share"] = 1.0 - step["gemm_share"] - step["attention_share"] - step["sandwich_norm_share"]
        print(f"  shares: GEMMs {step['gemm_share']:.3f}, attention {step['attention_share']:.3f}, sandwich norm "
              f"{step['sandwich_norm_share']:.3f}, rest {step['rest_share']:.3f}")
        res["gemma2_2b"] = step
        print(json.dumps(res))
        return
    if args.prefix_ab:
        from llamarec_amd.llm import GEMMA_2B
        from tools import prefix_ab

        builds = {spec.split("=", 1)[0]: prefix_ab.load_build(spec.split("=", 1)[1]) for spec in args.ab_lib}
        res = dict(attention_prefix=prefix_ab.attention_prefix_table(256, 4, ((8, 1), (16, 16)), args.reps))
        res["gemma2b_prefix_ab"] = prefix_ab.step_ab(dict(GEMMA_2B, num_hidden_layers=args.layers), 2, args.reps, builds, "gemma-2b")
        print(json.dumps(res))
        return
    res = dict(attention=attention_table(args.reps), gemma2b=gemma2b_step(args.steps, args.layers))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
