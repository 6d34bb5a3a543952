"""CPU test of the top-K plan (llamarec_amd/csrc/lru_topk_plan.h): tests/topk_plan_sweep.cpp, compiled against the
host-only header, sweeps 18 catalog sizes x 10 batch sizes x 5 K x 6 L x exclude and checks that the workspace regions lie
in order, 256-byte aligned and disjoint, that the chunks of the exact pass and of the bf16 passes cover the catalog within
the kernels' limits, where the bound path must be off, and the claim above lr_topk_workspace_bytes: sized for (B, K, L) it
is large enough for every call with b <= B, k <= K, l <= L."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "llamarec_amd", "csrc")


def test_topk_plan_sweep(tmp_path):
    # the C++ driver of the compiler the oracle is built with (oracle/Makefile: CC ?= gcc), else any C++ compiler
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "topk_plan_sweep")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(HERE, "topk_plan_sweep.cpp"), "-o", exe],
                   check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LR_TOPK_CHUNKS", "LR_TOPK_BOUND", "LR_BF16_WGS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # 18 * 10 * 5 * 6 * 2 plans; dominated pairs: 55 (b <= B) * 15 (k <= K) * 21 (l <= L) * 2 per catalog size
    assert r.stdout.strip().splitlines()[-1] == "plans 10800 pairs 623700 fails 0"
