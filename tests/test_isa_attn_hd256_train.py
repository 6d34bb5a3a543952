"""Build-time checks on the gfx950 code objects of attention variant 9 ("Training at head_dim 256"): the
two head_dim-256 backward passes (llama_attn_bwd_hd256.hip) and the lse-writing instantiation of the head_dim-256 forward
(llama_attn_hd256_lse.hip), compiled with the Makefile's flags, as tests/test_isa_attn_hd96_train.py checks variant 8. From the
code-object metadata: each translation unit holds exactly its kernels, no scratch, no spilled register, no static LDS beside the
ring asked for at launch, and a register count (VGPRs and AGPRs together) within the occupancy each kernel was designed for:
256 for two waves per SIMD (the dQ pass and the forward: 8 waves per workgroup, one workgroup per CU), 512 for one wave per SIMD
(the dK/dV pass: 4 waves per workgroup). From the instruction stream: the LDS-DMA requests are inline asm that hipcc's counters
do not see, so every s_barrier must have an `s_waitcnt vmcnt(0)` in front of it with no LDS-DMA between the two, and every write
of M0 (the DMA's LDS base) must be followed by the DMA it was made for. Runs without a GPU (hipcc cross-compiles)."""
import os
import re
import subprocess

import pytest

from tests.test_isa_attn_hd64_train import _body, _metadata, _symbol
from tests.test_isa_attn_hd96 import DMA
from tests.test_isa_checks import CSRC, FLAGS, HIPCC

# kernel name fragment -> (source file, register budget, LDS-DMA requests at least: pieces of two tiles per staging text, two texts)
KERNELS = {
    "attn_bwd_hd256_dq_kernel": ("llama_attn_bwd_hd256.hip", 256, 16),    # two waves per SIMD: 4 + 4 pieces per staging text
    "attn_bwd_hd256_dkv_kernel": ("llama_attn_bwd_hd256.hip", 512, 32),   # one wave per SIMD: 8 + 8 pieces per staging text
    "attn_hd256_lse_kernel": ("llama_attn_hd256_lse.hip", 256, 16),       # two waves per SIMD, as variant 4
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = {}
    for src in sorted({s for s, _, _ in KERNELS.values()}):
        path = tmp_path_factory.mktemp("isa") / (src + ".s")
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(path)], check=True,
                       capture_output=True, cwd=CSRC)
        out[src] = path.read_text()
    return out


def test_each_file_holds_exactly_its_kernels(asm):
    """The backward unit holds its two passes, the lse unit the one lse-writing forward kernel."""
    expected = {src: sorted(f for f, (s, _, _) in KERNELS.items() if s == src) for src in asm}
    assert len(expected["llama_attn_bwd_hd256.hip"]) == 2 and len(expected["llama_attn_hd256_lse.hip"]) == 1
    for src, fragments in expected.items():
        names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm[src], flags=re.M)
        assert len(names) == len(fragments) and all(any(f in n for n in names) for f in fragments), (src, names)


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_hd256_training_kernels_fit_their_occupancy_without_scratch(asm, fragment):
    src, budget, _ = KERNELS[fragment]
    text = asm[src]
    sym = _symbol(text, fragment)
    blk, note = _metadata(text, sym)
    assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk), (sym, "uses scratch")
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", note).group(1)) == 0, sym
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", note).group(1)) == 0, (sym, "static LDS beside the ring")
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", note).group(1))   # the unified file: VGPRs and AGPRs together
    agprs = int(re.search(r"\.agpr_count:\s+(\d+)", note).group(1))
    sgprs = int(re.search(r"\.sgpr_count:\s+(\d+)", note).group(1))
    print(f"{sym}: {vgprs} VGPRs ({agprs} of them AGPRs), {sgprs} SGPRs, budget {budget}")
    assert vgprs <= budget, (sym, vgprs, budget)


@pytest.mark.parametrize("fragment", sorted(KERNELS))
def test_hd256_training_kernels_wait_for_their_dma_in_front_of_every_barrier(asm, fragment):
    src, _, min_dma = KERNELS[fragment]
    text = asm[src]
    body = _body(text, _symbol(text, fragment))
    barriers = [i for i, ln in enumerate(body) if ln.startswith("s_barrier")]
    n_dma = sum(1 for ln in body if DMA.match(ln))
    print(f"{fragment}: {len(barriers)} s_barrier, {n_dma} LDS-DMA requests")
    assert len(barriers) >= 2, (fragment, "the prologue's and the streaming loop's barriers")
    assert n_dma >= min_dma, fragment
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
    src, _, _ = KERNELS[fragment]
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
