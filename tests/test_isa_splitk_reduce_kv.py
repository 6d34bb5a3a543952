"""Build-time check on the gfx950 code object of splitk_reduce_rope_kv_kernel (llama_gemm.hip, DESIGN 16 "Latency mode"), the
split-K reduce pass of the QKV product that stores K | V into the cache slot: code-object metadata only, compiled with the
Makefile's flags. The kernel exists exactly once, uses no scratch, spills nothing, asks for no LDS, and stays a small
element-wise kernel like splitk_reduce_kernel<rope> beside it. Runs without a GPU (hipcc cross-compiles)."""
from tests.test_isa_gemm_ragged import _numbers, asm  # noqa: F401  (asm: the module-scoped fixture that compiles llama_gemm.hip)

NEW = "splitk_reduce_rope_kv_kernel"
BESIDE = "splitk_reduce_kernelILi3EJEE"   # <LR_EPI_ROPE>, no bias
VGPR_BUDGET = 32                          # 8 waves of 256 threads per SIMD need <= 64; the sibling takes 15


def test_the_cache_writing_reduce_pass_uses_no_scratch_and_few_registers(asm):  # noqa: F811
    sym, n = _numbers(asm, NEW)
    _, beside = _numbers(asm, BESIDE)
    print(f"{sym}: {n['vgpr_count']} VGPRs ({n['agpr_count']} AGPRs), {n['sgpr_count']} SGPRs, scratch "
          f"{n['private_segment_fixed_size']}; beside it: {beside['vgpr_count']} VGPRs, {beside['sgpr_count']} SGPRs")
    assert n["private_segment_fixed_size"] == 0 and not n["scratch_in_descriptor"], (sym, "uses scratch")
    assert n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, sym
    assert n["group_segment_fixed_size"] == 0 and n["agpr_count"] == 0, sym
    assert n["max_flat_workgroup_size"] == 256
    assert n["vgpr_count"] <= VGPR_BUDGET, (sym, n)
