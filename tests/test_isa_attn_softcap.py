"""Build-time checks on the gfx950 code object of the soft-capped head_dim-256 attention (llama_attn_hd256_softcap.hip: the
SOFTCAP mode of llama_attn_hd256_body.h in variant 4's three forms), compiled with the Makefile's flags.
From the code-object metadata alone: the file holds exactly its three kernels; none uses scratch or spills a register; each
stays within 256 VGPRs (two waves per SIMD, one workgroup per CU, as variant 4); their static LDS is variant 4's (both take
their 128 KiB dynamically, with the same FA4_LDS_BYTES). Runs without a GPU (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

from tests.test_isa_attn_hd64_train import _metadata, _symbol
from tests.test_isa_checks import CSRC, FLAGS, HIPCC

SOFTCAP_KERNELS = ("attn_hd256_softcap_kernel", "attn_hd256_softcap_prefix_kernelILb0EE", "attn_hd256_softcap_prefix_kernelILb1EE")
VGPR_BUDGET = 256


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = {}
    for src in ("llama_attn_hd256_softcap.hip", "llama_attn_hd256.hip"):
        path = tmp_path_factory.mktemp("isa") / (src + ".s")
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(path)], check=True,
                       capture_output=True, cwd=CSRC)
        out[src] = path.read_text()
    return out


def _lds(text, fragment):
    blk, note = _metadata(text, _symbol(text, fragment))
    return int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", note).group(1))


def test_the_file_holds_exactly_the_three_capped_kernels(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm["llama_attn_hd256_softcap.hip"], flags=re.M)
    assert len(names) == 3 and all(any(f in n for n in names) for f in SOFTCAP_KERNELS), names
    # ... and variant 4's file still holds variant 4 alone
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm["llama_attn_hd256.hip"], flags=re.M)) == 1


@pytest.mark.parametrize("fragment", SOFTCAP_KERNELS)
def test_capped_kernels_fit_256_vgprs_without_scratch_and_with_variant_4s_lds(asm, fragment):
    text = asm["llama_attn_hd256_softcap.hip"]
    sym = _symbol(text, fragment)
    blk, note = _metadata(text, sym)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk), (sym, "uses scratch")
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", note).group(1))
    agprs = int(re.search(r"\.agpr_count:\s+(\d+)", note).group(1))
    print(f"{sym}: {vgprs} VGPRs ({agprs} of them AGPRs)")
    assert vgprs <= VGPR_BUDGET, (sym, vgprs)
    assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", note).group(1)) == 512, sym
    assert _lds(text, fragment) == _lds(asm["llama_attn_hd256.hip"], "attn_hd256_kernelILi1EE"), (sym, "static LDS differs from variant 4's")


def test_both_launchers_ask_for_the_same_dynamic_lds():
    """The 128 KiB are dynamic LDS: both files name the one macro of the shared body in every launch. A launch is a call of
    llama_kernels.h's launcher templates, which hand their BLOCK and LDS_BYTES arguments to the one hipLaunchKernelGGL."""
    body = open(os.path.join(CSRC, "llama_attn_hd256_body.h")).read()
    assert len(re.findall(r"^#define FA4_LDS_BYTES\b", body, flags=re.M)) == 1
    header = open(os.path.join(CSRC, "llama_kernels.h")).read()
    assert "hipLaunchKernelGGL(KERNEL, dim3((unsigned)pl.grid), dim3(BLOCK), LDS_BYTES, st, args...);" in header
    n = 0
    for src in ("llama_attn_hd256_softcap.hip", "llama_attn_hd256.hip", "llama_attn_hd256_prefix.hip"):
        text = open(os.path.join(CSRC, src)).read()
        assert "hipLaunchKernelGGL" not in text and "lr_attn_launch_kernel" not in text, src
        launches = re.findall(r"lr_attn_launch_(?:tiles|last)<(.*?)>\(", text, flags=re.S)
        assert launches and all(re.search(r"\b512, FA4_LDS_BYTES\b", l) for l in launches), src
        assert "#define FA4_LDS_BYTES" not in text, src
        n += len(launches)
    assert n == 6, n   # variant 4's three forms and the capped three: one launch per kernel
