"""Same-process A/B of attention variant 4's workgroup shape at MQA / GQA: one head per workgroup
(128 query rows, the product) against two heads of one KV head per workgroup (64 rows each, one staged K/V tile serving
both). Builds tools/diag/attn_hd256_mqa_ab.hip into a shared library linked against the product library, checks both
forms give the same bits, and prints the median time of each, alternating the arms.
Usage: python tools/diag/attn_hd256_mqa_ab.py [--reps 30]"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from llamarec_amd import _lib  # noqa: E402


def build():
    libdir = os.path.dirname(_lib.LIB_PATH)
    out = os.path.join(tempfile.mkdtemp(), "libattn_hd256_ab.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                    os.path.join(REPO, "tools", "diag", "attn_hd256_mqa_ab.hip"), "-L", libdir, "-lllamarec_mi355x",
                    "-Wl,-rpath," + libdir, "-o", out], check=True)
    C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL)
    return C.CDLL(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    ab = build()
    ab.diag_attn_hd256.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]
    st = torch.cuda.current_stream().cuda_stream
    for nh, nkv in ((8, 1), (16, 1), (8, 2)):
        for T in (600, 1125):
            B = 16
            n = B * T
            g = torch.Generator(device="cuda").manual_seed(T + nh)
            qkv = torch.randn(n, (nh + 2 * nkv) * 256, generator=g, device="cuda").to(torch.bfloat16)
            cu = np.arange(0, n + 1, T, dtype=np.int32)
            cud = torch.from_numpy(cu).cuda()
            outs = {hpw: torch.empty(n, nh * 256, dtype=torch.bfloat16, device="cuda") for hpw in (1, 2)}

            def run(hpw):
                rc = ab.diag_attn_hd256(qkv.data_ptr(), outs[hpw].data_ptr(), cud.data_ptr(), cu.ctypes.data, B, n, nh, nkv, hpw, st)
                assert rc == 0, _lib.lib().lr_last_error()

            for hpw in (1, 2, 1, 2):
                run(hpw)
            torch.cuda.synchronize()
            same = torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16))
            times = {1: [], 2: []}
            for _ in range(args.reps):
                for hpw in (1, 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(hpw)
                    e1.record()
                    torch.cuda.synchronize()
                    times[hpw].append(e0.elapsed_time(e1))
            work = 4.0 * nh * 256 * B * T * (T + 1) / 2
            m1, m2 = float(np.median(times[1])), float(np.median(times[2]))
            print(f"nh={nh:2d} nkv={nkv} 16 x {T:4d}: one head/wg {m1:.4f} ms {work / m1 / 1e9:6.1f} TF/s | two heads/wg "
                  f"{m2:.4f} ms {work / m2 / 1e9:6.1f} TF/s | two/one time {m2 / m1:.3f} | same bits {same}", flush=True)


if __name__ == "__main__":
    main()
