"""Build-time checks on the gfx950 code objects of the 256 x 256 x 64 GEMM kernel's new instantiations (llama_gemm.hip,
DESIGN.md section 13): a bias in the store and rope epilogues, the ragged last column tile of variant 6, and both. Code-object
metadata only, compiled with the Makefile's flags: each of them exists exactly once, uses no scratch and spills no register,
asks for no static LDS (the two 64 KiB stages are dynamic, as for the instantiation it stands beside), and its register counts
leave one 512-thread workgroup per CU -- two waves per SIMD, 256 VGPRs each. Runs without a GPU (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

from tests.test_isa_attn_hd64_train import _metadata, _symbol
from tests.test_isa_checks import CSRC, FLAGS, HIPCC

# mangled template arguments <EPI, FOLD, STAMP, RAGGED, Bias...> -> the instantiation without bias and ragged tile beside it
PLAIN = {0: "gemm256rb_kernelILi0ELb0ELb0ELb0EJEE", 1: "gemm256rb_kernelILi1ELb0ELb0ELb0EJEE", 3: "gemm256rb_kernelILi3ELb0ELb0ELb0EJEE"}
NEW = {
    "store + bias": (0, "gemm256rb_kernelILi0ELb0ELb0ELb0EJPKtEE"),
    "rope + bias": (3, "gemm256rb_kernelILi3ELb0ELb0ELb0EJPKtEE"),
    "ragged store": (0, "gemm256rb_kernelILi0ELb0ELb0ELb1EJEE"),
    "ragged store + bias": (0, "gemm256rb_kernelILi0ELb0ELb0ELb1EJPKtEE"),
    "ragged residual": (1, "gemm256rb_kernelILi1ELb0ELb0ELb1EJEE"),
    "ragged rope": (3, "gemm256rb_kernelILi3ELb0ELb0ELb1EJEE"),
    "ragged rope + bias": (3, "gemm256rb_kernelILi3ELb0ELb0ELb1EJPKtEE"),
}
VGPR_BUDGET = 256   # 512 VGPRs per SIMD lane, two waves of the workgroup per SIMD
SGPR_BUDGET = 102


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    path = tmp_path_factory.mktemp("isa") / "llama_gemm.s"
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, "llama_gemm.hip"), "-o", str(path)], check=True,
                   capture_output=True, cwd=CSRC)
    return path.read_text()


def _numbers(text, fragment):
    sym = _symbol(text, fragment)
    blk, note = _metadata(text, sym)
    get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, note).group(1))  # noqa: E731
    n = {k: get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                             "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")}
    n["scratch_in_descriptor"] = not re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk)
    return sym, n


def test_the_unit_holds_the_new_instantiations_and_no_ragged_gated_or_split_k_one(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    tile = [n for n in names if "gemm256rb_kernel" in n]
    ragged = [n for n in tile if "ELb1EJ" in n]
    assert len(ragged) == 5 and all(re.search(r"ILi[013]ELb0ELb0ELb1EJ", n) for n in ragged), ragged   # store, residual, rope only
    assert len([n for n in tile if "EJPKtEE" in n]) == 4, tile
    assert len([n for n in names if "gemm_generic_kernel" in n and "PKtEE" in n]) == 2          # generic: store and rope with bias
    assert len([n for n in names if "splitk_reduce_kernel" in n and "JPKtEE" in n]) == 2      # the reduce pass too


@pytest.mark.parametrize("what", sorted(NEW))
def test_new_gemm_instantiations_keep_scratch_lds_and_occupancy(asm, what):
    epi, fragment = NEW[what]
    sym, n = _numbers(asm, fragment)
    _, plain = _numbers(asm, PLAIN[epi])
    print(f"{what}: {n['vgpr_count']} VGPRs ({n['agpr_count']} AGPRs), {n['sgpr_count']} SGPRs, scratch {n['private_segment_fixed_size']}, "
          f"static LDS {n['group_segment_fixed_size']}; beside it: {plain['vgpr_count']} VGPRs, {plain['sgpr_count']} SGPRs")
    assert n["private_segment_fixed_size"] == 0 and not n["scratch_in_descriptor"], (sym, "uses scratch")
    assert n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, sym
    assert n["group_segment_fixed_size"] == plain["group_segment_fixed_size"] == 0, (sym, "static LDS beside the two dynamic stages")
    assert n["max_flat_workgroup_size"] == 512
    assert n["vgpr_count"] + n["agpr_count"] <= VGPR_BUDGET and n["sgpr_count"] <= SGPR_BUDGET, (sym, n)
