"""Shared-prefix / last-row A/B arms of tools/bench_llama32.py and tools/bench_gemma.py (DESIGN sections 9 and 10).
One process, HIP events, arms ALTERNATING inside every repeat, median and min .. max per arm.
  step arms       shared = the product library with the batch's common prefix handed over (prefix run once, last-row mode in
                  the pruned last layer); plain = the product library with prefix_len = 0 (pinned attention kernels on whole
                  prompts; the last-row mode stays); NAME = another BUILD of the library (--ab-lib NAME=PATH, e.g. the parent
                  commit's) on the same prompts with the same prefix_len handed over, through a handle of its own.
  attention arms  the prefix kernel on 16 x T-token prompts sharing 36 tokens (lr_attention_varlen_prefix) against the pinned
                  kernel on the same whole prompts (lr_attention_varlen); the last-row launch (lr_attention_last_rows) against
                  full attention followed by a gather of the 16 last rows."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np
import torch

from llamarec_amd import _lib
from llamarec_amd._lib import check, lib, stream_ptr

KINDS = {0: "gemm 256-tile", 1: "gemm generic", 2: "attention MFMA", 3: "attention generic"}
PREFIX = 36   # the template text in front of the first history item, in Llama tokens


def load_build(path):
    """Another build of the library with every prototype it has (an older build lacks the newest entry points)."""
    lib()   # torch and the product library first: the HIP runtime they bring in owns the devices
    l = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(l, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return l


@contextlib.contextmanager
def use_build(l):
    """Everything llamarec_amd calls inside the block goes to build `l` (None: the product library)."""
    if l is None:
        yield
        return
    keep = _lib._lib
    _lib._lib = l
    try:
        yield
    finally:
        _lib._lib = keep


def budget_prompts(cfg, bos, prefix=PREFIX, seed=0):
    """Prompts of 460 .. 1 125 tokens that share `prefix` tokens, as many as packing.TOKEN_BUDGET rows hold when the shared
    rows are counted once (token_budget_steps' credit)."""
    from llamarec_amd.packing import TOKEN_BUDGET

    rng = np.random.default_rng(seed)
    head = np.concatenate([[bos], rng.integers(3, cfg["vocab_size"], size=prefix - 1)])
    seqs, rows = [], prefix
    while True:
        t = int(rng.integers(460, 1126))
        if rows + t - prefix > TOKEN_BUDGET:
            break
        seqs.append(np.concatenate([head, rng.integers(3, cfg["vocab_size"], size=t - prefix)]).astype(np.int32))
        rows += t - prefix
    return seqs


def _split(L, steps):
    out = {}
    for kind, name in KINDS.items():
        ms, work, n = C.c_double(), C.c_double(), C.c_int64()
        L.lr_profile_collect(kind, C.byref(ms), C.byref(work), C.byref(n))
        if n.value:
            out[name] = dict(ms_per_step=ms.value / steps, launches_per_step=n.value / steps)
    return out


def step_ab(cfg, bos, reps, builds, label):
    """{arm: median / min / max ms per step, profile split}, the scores' agreement, and the row counts."""
    from llamarec_amd.llm import LlamaRanker, common_prefix_len, pack_prompts

    seqs = budget_prompts(cfg, bos)
    ids, cu = pack_prompts(seqs)
    P = common_prefix_len(ids, cu)
    ids_d, cu_d = torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda()
    lab = torch.arange(100, 120, dtype=torch.int32, device="cuda")
    arms = {"shared": (None, P), "plain": (None, 0)}
    for name, l in builds.items():
        arms[name] = (l, P)
    models, outs = {}, {}
    for name, (l, _) in arms.items():
        key = id(l)
        if key not in models:
            with use_build(l):
                models[key] = LlamaRanker.random_init(cfg, seed=1)
    def run(name):
        l, p = arms[name]
        with use_build(l):
            models[id(l)].prefill_verbalize_packed(ids_d, cu_d, cu, lab, out=outs[name], prefix_len=p)
    for name in arms:
        outs[name] = torch.empty(len(seqs), 20, dtype=torch.float32, device="cuda")
        for _ in range(2):
            run(name)
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    res = dict(prompts=len(seqs), tokens=int(cu[-1]), prefix=int(P), rows_shared=int(cu[-1] - (len(seqs) - 1) * P), reps=reps,
               layers=cfg["num_hidden_layers"], arms={})
    for name, (l, _) in arms.items():
        L = l or lib()
        check(L.lr_profile_start(3 * (cfg["num_hidden_layers"] * 12 + 32)), "lr_profile_start")
        for _ in range(3):
            run(name)
        torch.cuda.synchronize()
        check(L.lr_profile_stop(), "lr_profile_stop")
        split = _split(L, 3)
        gemm = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("gemm"))
        attn = sum(v["ms_per_step"] for k, v in split.items() if k.startswith("attention"))
        t = times[name]
        med = float(np.median(t))
        res["arms"][name] = dict(ms_median=med, ms_min=min(t), ms_max=max(t), gemm_ms=gemm, attention_ms=attn,
                                 rest_ms=med - gemm - attn, kernels=split,
                                 same_bits_as_shared=bool(torch.equal(outs[name], outs["shared"])),
                                 max_abs_minus_shared=float((outs[name] - outs["shared"]).abs().max()))
        assert torch.isfinite(outs[name]).all()
        print(f"{label} step, {name:7s}: median {med:8.3f} ms (min {min(t):8.3f}, max {max(t):8.3f}, {reps} alternating reps) | "
              f"GEMMs {gemm:7.2f} attention {attn:6.2f} rest {med - gemm - attn:6.2f} ms | scores == shared: "
              f"{res['arms'][name]['same_bits_as_shared']} (max |diff| {res['arms'][name]['max_abs_minus_shared']:.4f})", flush=True)
    print(f"{label} step: {res['prompts']} prompts, {res['tokens']} tokens, prefix {P}: {res['rows_shared']} rows shared "
          f"({100.0 * (res['tokens'] - res['rows_shared']) / res['tokens']:.2f} % fewer)", flush=True)
    return res


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
    return {k: (float(np.median(t)), min(t), max(t)) for k, t in times.items()}


def attention_prefix_table(hd, variant, heads, reps, lengths=(600, 1125), B=16, P=PREFIX):
    """Rows of the attention arms for every (nh, nkv) of `heads` and prompt length."""
    L = lib()
    rows = []
    for nh, nkv in heads:
        for T in lengths:
            g = torch.Generator(device="cuda").manual_seed(T + nh)
            w = (nh + 2 * nkv) * hd
            whole = torch.randn(B * T, w, generator=g, device="cuda").to(torch.bfloat16).view(B, T, w)
            whole[:, :P] = whole[0, :P]
            whole = whole.reshape(B * T, w).contiguous()
            cu = np.arange(0, B * T + 1, T, dtype=np.int32)
            src = torch.cat([torch.arange(P)] + [torch.arange(b * T + P, (b + 1) * T) for b in range(B)]).cuda()
            packed = whole[src].contiguous()
            seg = np.concatenate([[0, P], P + np.cumsum([T - P] * B)]).astype(np.int32)
            cud, segd = torch.from_numpy(cu).cuda(), torch.from_numpy(seg).cuda()
            last = torch.from_numpy(cu[1:].astype(np.int64) - 1).cuda()
            out_w = torch.empty(B * T, nh * hd, dtype=torch.bfloat16, device="cuda")
            out_p = torch.empty(len(src), nh * hd, dtype=torch.bfloat16, device="cuda")
            kv = packed[:, nh * hd:].contiguous()
            q_last = whole[last, :nh * hd].contiguous()
            out_l = torch.empty(B, nh * hd, dtype=torch.bfloat16, device="cuda")
            out_g = torch.empty(B, nh * hd, dtype=torch.bfloat16, device="cuda")

            def pinned():
                check(L.lr_attention_varlen(whole.data_ptr(), out_w.data_ptr(), cud.data_ptr(), cu.ctypes.data, B, nh, nkv, hd,
                                            variant, stream_ptr()), "lr_attention_varlen")

            def prefix():
                check(L.lr_attention_varlen_prefix(packed.data_ptr(), out_p.data_ptr(), segd.data_ptr(), seg.ctypes.data, B + 1, P,
                                                   nh, nkv, hd, variant, stream_ptr()), "lr_attention_varlen_prefix")

            def last_rows():
                check(L.lr_attention_last_rows(kv.data_ptr(), q_last.data_ptr(), out_l.data_ptr(), segd.data_ptr(), seg.ctypes.data,
                                               B + 1, P, nh, nkv, hd, variant, stream_ptr()), "lr_attention_last_rows")

            def full_gather():
                pinned()
                torch.index_select(out_w, 0, last, out=out_g)

            t = _alternate(dict(pinned=pinned, prefix=prefix, last_rows=last_rows, full_gather=full_gather), reps)
            same = bool(torch.equal(out_p, out_w[src])) and bool(torch.equal(out_l, out_g))
            rows.append(dict(hd=hd, nh=nh, nkv=nkv, T=T, B=B, prefix=P, same_bits=same,
                             **{f"{k}_ms": v[0] for k, v in t.items()}, **{f"{k}_min_max": v[1:] for k, v in t.items()}))
            print(f"attention hd={hd} nh={nh:2d} nkv={nkv:2d} {B} x {T:4d}, prefix {P}: pinned {t['pinned'][0]:7.3f} ms "
                  f"({t['pinned'][1]:.3f} .. {t['pinned'][2]:.3f}) | prefix kernel {t['prefix'][0]:7.3f} ms ({t['prefix'][1]:.3f} .. "
                  f"{t['prefix'][2]:.3f}) | last rows {t['last_rows'][0]:7.3f} ms | full + gather {t['full_gather'][0]:7.3f} ms | "
                  f"same bits {same}", flush=True)
    return rows
