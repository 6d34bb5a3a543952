"""Build-time checks on the gfx950 code objects of attention variant 6: the two head_dim-64 backward
passes (llama_attn_bwd_hd64.hip) and the lse-writing instantiation of the head_dim-64 forward (llama_attn_hd64.hip), compiled
with the Makefile's flags. From the code-object metadata: no scratch, no spilled register, and a VGPR count at or below the
budget of the occupancy DESIGN states. From the instruction stream: the LDS-DMA requests of the streaming loop are invisible to
hipcc's counters, so every s_barrier must be preceded by an `s_waitcnt vmcnt(0)` with no other barrier in between.
Runs without a GPU (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

from tests.test_isa_checks import CSRC, FLAGS, HIPCC

# kernel name fragment -> (source file, VGPR budget): 512 registers per SIMD lane / workgroups per CU (one wave per SIMD each)
BUDGET = {
    "attn_bwd_hd64_dq_kernel": ("llama_attn_bwd_hd64.hip", 128),    # four workgroups per CU
    "attn_bwd_hd64_dkv_kernel": ("llama_attn_bwd_hd64.hip", 128),   # four
    "attn_hd64_kernelILb1EE": ("llama_attn_hd64_lse.hip", 168),     # the lse instantiation: three, as variant 5
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = {}
    for src in sorted({s for s, _ in BUDGET.values()}):
        path = tmp_path_factory.mktemp("isa") / (src + ".s")
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(path)], check=True,
                       capture_output=True, cwd=CSRC)
        out[src] = path.read_text()
    return out


def _symbol(text, fragment):
    names = [n for n in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M) if fragment in n]
    assert len(names) == 1, (fragment, names)
    return names[0]


def _metadata(text, symbol):
    """The .amdhsa_kernel block and the metadata note of one kernel."""
    blk = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(symbol), text, flags=re.M | re.S).group(1)
    notes = [c for c in re.split(r"^  - (?=\.agpr_count:)", text, flags=re.M)[1:] if re.search(r"\.name:\s+%s\n" % re.escape(symbol), c)]
    assert len(notes) == 1, symbol
    return blk, notes[0]


@pytest.mark.parametrize("fragment", sorted(BUDGET))
def test_hd64_training_kernels_fit_their_register_budget_without_scratch(asm, fragment):
    src, budget = BUDGET[fragment]
    text = asm[src]
    sym = _symbol(text, fragment)
    blk, note = _metadata(text, sym)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk), (sym, "uses scratch")
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", note).group(1))
    agprs = int(re.search(r"\.agpr_count:\s+(\d+)", note).group(1))
    print(f"{sym}: {vgprs} VGPRs ({agprs} of them AGPRs), budget {budget}")
    assert vgprs <= budget, (sym, vgprs, budget)


def _body(text, symbol):
    """The instruction lines of one kernel, up to the end of the function (an early exit's s_endpgm does not end it)."""
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(symbol), text, flags=re.M | re.S)
    assert m, symbol
    lines = [ln.split(";")[0].strip() for ln in m.group(1).splitlines()]
    return [ln for ln in lines if ln and not ln.startswith(".") and not ln.endswith(":")]


@pytest.mark.parametrize("fragment", sorted(BUDGET))
def test_hd64_training_kernels_wait_for_their_dma_in_front_of_every_barrier(asm, fragment):
    src, _ = BUDGET[fragment]
    text = asm[src]
    body = _body(text, _symbol(text, fragment))
    barriers = [i for i, ln in enumerate(body) if ln.startswith("s_barrier")]
    assert len(barriers) >= 2, (fragment, "the prologue's and the streaming loop's barriers")
    for i in barriers:
        for x in reversed(body[:i]):
            if re.match(r"s_waitcnt\b.*vmcnt\(0\)", x):
                break
            assert not x.startswith("s_barrier"), (fragment, "an s_barrier without `s_waitcnt vmcnt(0)` in front of it")
        else:
            raise AssertionError((fragment, "an s_barrier without `s_waitcnt vmcnt(0)` in front of it"))
