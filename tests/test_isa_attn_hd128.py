"""Build-time checks on the gfx950 code objects of the four head_dim-128 MFMA attention kernels that share one body
(llama_attn_hd128_body.h): attn_mfma128_kernel<false, false / true> (llama_attn.hip) and attn_cached128_kernel<false / true>
(llama_attn_cached.hip), compiled with the Makefile's flags.
From the code-object metadata: no scratch, no spilled register, and a VGPR count within what `__launch_bounds__(256, 2)`
promises (512 registers per SIMD lane over two waves). From the instruction stream: a cached kernel holds as many MFMAs,
transposed and 128-bit LDS reads, exponentials and barriers as its whole-prompt counterpart -- one body must produce one
key block, whatever the source of its rows; the two builds are compared with each other, not with a number.
(The M0 / vmcnt discipline of the LDS-DMA in both files is tests/test_isa_checks.py's.) Runs without a GPU (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

from tests.test_isa_attn_hd64_train import _body, _metadata, _symbol
from tests.test_isa_checks import CSRC, FLAGS, HIPCC

# kernel name fragment -> source file
KERNELS = {
    "attn_mfma128_kernelILb0ELb0EE": "llama_attn.hip",          # whole prompts / shared prefix, query tiles
    "attn_mfma128_kernelILb0ELb1EE": "llama_attn.hip",          # one query row per prompt
    "attn_cached128_kernelILb0EE": "llama_attn_cached.hip",     # cached, query tiles
    "attn_cached128_kernelILb1EE": "llama_attn_cached.hip",     # cached, one query row per prompt
}
# cached kernel -> its whole-prompt counterpart: tiles with tiles, one row with one row
COUNTERPART = {"attn_cached128_kernelILb0EE": "attn_mfma128_kernelILb0ELb0EE", "attn_cached128_kernelILb1EE": "attn_mfma128_kernelILb0ELb1EE"}
COUNTED = ("v_mfma", "ds_read_b64_tr_b16", "ds_read_b128", "v_exp_f32", "s_barrier")
VGPR_BUDGET = 256   # 512 per SIMD lane / 2 waves per SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = {}
    for src in sorted(set(KERNELS.values())):
        path = tmp_path_factory.mktemp("isa") / (src + ".s")
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(path)], check=True,
                       capture_output=True, cwd=CSRC)
        out[src] = path.read_text()
    return out


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_hd128_kernels_fit_two_waves_per_simd_without_scratch(asm, fragment):
    text = asm[KERNELS[fragment]]
    sym = _symbol(text, fragment)
    blk, note = _metadata(text, sym)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk), (sym, "uses scratch")
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", note).group(1))
    print(f"{sym}: {vgprs} VGPRs, budget {VGPR_BUDGET}")
    assert vgprs <= VGPR_BUDGET, (sym, vgprs)


@pytest.mark.parametrize("cached", sorted(COUNTERPART))
def test_cached_kernel_holds_the_key_block_of_its_whole_prompt_counterpart(asm, cached):
    def counts(fragment):
        text = asm[KERNELS[fragment]]
        body = _body(text, _symbol(text, fragment))
        return {op: sum(1 for ln in body if re.match(re.escape(op) + r"\w*\b", ln)) for op in COUNTED}

    mine, theirs = counts(cached), counts(COUNTERPART[cached])
    print(cached, mine, COUNTERPART[cached], theirs)
    assert all(n > 0 for n in theirs.values()), theirs
    assert mine == theirs, (cached, mine, theirs)
