"""Build-time checks on the gfx950 code objects of the head_dim-64 and head_dim-256 attention kernels that share one body
per head size (llama_attn_hd64_body.h, llama_attn_hd256_body.h; DESIGN.md sections 9 and 10): the pinned kernels
(llama_attn_hd64.hip, llama_attn_hd256.hip) and the shared-prefix and last-row kernels (llama_attn_hd64_prefix.hip,
llama_attn_hd256_prefix.hip), compiled with the Makefile's flags.
From the code-object metadata: no scratch, no spilled register, and for the pinned and the prefix kernels a VGPR count within
the occupancy they are built for (three workgroups per CU at head_dim 64, two waves per SIMD at 256). From the instruction stream: the
LDS-DMA requests are inline asm that hipcc's counters do not see, so every s_barrier must have an `s_waitcnt vmcnt(0)` in front
of it with no LDS-DMA between the two, and every write of M0 (the DMA's LDS base) must be followed by the DMA it was made for.
Runs without a GPU (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

from tests.test_isa_attn_hd64_train import _body, _metadata, _symbol
from tests.test_isa_checks import CSRC, FLAGS, HIPCC

# kernel name fragment -> (source file, VGPR budget or None: spill-free is all the last-row kernels are held to)
KERNELS = {
    "attn_hd64_kernelILb0EE": ("llama_attn_hd64.hip", 168),                  # variant 5: 512 / 3 workgroups per CU
    "attn_hd256_kernelILi1EE": ("llama_attn_hd256.hip", 256),                # variant 4: two waves per SIMD
    "attn_hd64_prefix_kernelILb0EE": ("llama_attn_hd64_prefix.hip", 168),    # 512 / 3 workgroups per CU, as variant 5
    "attn_hd64_prefix_kernelILb1EE": ("llama_attn_hd64_prefix.hip", None),
    "attn_hd256_prefix_kernelILb0EE": ("llama_attn_hd256_prefix.hip", 256),  # two waves per SIMD, as variant 4
    "attn_hd256_prefix_kernelILb1EE": ("llama_attn_hd256_prefix.hip", None),
}
DMA = re.compile(r"(buffer_load_dword\w*\b.*\blds\b|global_load_lds_dword\w*)")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = {}
    for src in sorted({s for s, _ in KERNELS.values()}):
        path = tmp_path_factory.mktemp("isa") / (src + ".s")
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(path)], check=True,
                       capture_output=True, cwd=CSRC)
        out[src] = path.read_text()
    return out


def test_each_file_holds_exactly_its_two_kernels(asm):
    """Each file holds the kernels the table gives it and no other: two in the prefix files, one in the pinned files."""
    expected = {src: sorted(f for f, (s, _) in KERNELS.items() if s == src) for src in asm}
    assert len(expected["llama_attn_hd64.hip"]) == 1 and len(expected["llama_attn_hd256.hip"]) == 1
    for src, fragments in expected.items():
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm[src], flags=re.M)
        assert len(names) == len(fragments) and all(any(f in n for n in names) for f in fragments), (src, names)


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_prefix_kernels_fit_their_register_budget_without_scratch(asm, fragment):
    src, budget = KERNELS[fragment]
    text = asm[src]
    sym = _symbol(text, fragment)
    blk, note = _metadata(text, sym)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk), (sym, "uses scratch")
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", note).group(1))
    print(f"{sym}: {vgprs} VGPRs, budget {budget}")
    if budget is not None:
        assert vgprs <= budget, (sym, vgprs, budget)


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_prefix_kernels_wait_for_their_dma_in_front_of_every_barrier(asm, fragment):
    src, _ = KERNELS[fragment]
    text = asm[src]
    body = _body(text, _symbol(text, fragment))
    barriers = [i for i, ln in enumerate(body) if ln.startswith("s_barrier")]
    assert len(barriers) >= 2, (fragment, "the prologue's and the key-block loop's barriers")
    assert sum(1 for ln in body if DMA.match(ln)) >= 8, (fragment, "the one-home and the straddling staging paths")
    for i in barriers:
        for x in reversed(body[:i]):
            if re.match(r"s_waitcnt\b.*vmcnt\(0\)", x):
                break
            assert not DMA.match(x), (fragment, "an LDS-DMA between `s_waitcnt vmcnt(0)` and the s_barrier it serves")
            assert not x.startswith("s_barrier"), (fragment, "an s_barrier without `s_waitcnt vmcnt(0)` in front of it")
        else:
            raise AssertionError((fragment, "an s_barrier without `s_waitcnt vmcnt(0)` in front of it"))


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_every_m0_write_is_followed_by_its_dma(asm, fragment):
    src, _ = KERNELS[fragment]
    text = asm[src]
    body = _body(text, _symbol(text, fragment))
    writes = [i for i, ln in enumerate(body) if re.match(r"s_mov_b32\s+m0\b", ln)]
    assert writes, fragment
    for i in writes:
        j = i + 1
        while body[j].startswith("s_nop"):
            j += 1
        assert DMA.match(body[j]), (fragment, body[i:j + 1])
    assert len(writes) == sum(1 for ln in body if DMA.match(ln)), fragment
