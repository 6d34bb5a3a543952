"""The 256x256x64 GEMM's K loop at the tile counts where its prologue, steady state and tail meet.

The loop holds one K tile per LDS stage and prefetches up to two tiles ahead (`more`, `more2` in RB_TILE of
llama_gemm.hip), two K tiles per trip. test_gpu_llama.py compares it bit for bit with the generic kernel at K = 512
(eight K tiles) only; here K runs over 1..5 tiles (odd and even, `more` / `more2` false in every position), M over one
ragged row tile, a nearly full one and full + ragged, N over one and two column tiles, for every fused epilogue; split-K
runs start at kt_first != 0 with an even and an odd tile count; and an integer product checks the kernel against numpy
alone. A race or a wrong wait count in the loop gives wrong numbers, not a fault: identical bits are the criterion.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, f32_to_bf16_bits, hash_uniform

HD, T_ROPE, ROT_COLS = 128, 700, 256   # one rotated 256-column tile; N = 512 adds a tile of plain (v) columns


@pytest.fixture(scope="module")
def rope_table():
    from llamarec_amd._lib import check, lib, stream_ptr

    L = lib()
    cs = torch.empty(L.lr_rope_table_bytes(T_ROPE, HD) // 4, dtype=torch.float32, device="cuda")
    check(L.lr_rope_table(cs.data_ptr(), T_ROPE, HD, 10000.0, stream_ptr()), "rope table")
    torch.cuda.synchronize()
    return cs


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320])
def test_every_epilogue_equals_generic_kernel_bit_for_bit_at_1_to_5_k_tiles(K, M, N, rope_table):
    """Operands and rotary set-up of test_gemm_epilogues_fast_kernel_equals_generic_kernel_bit_for_bit: every accumulator
    takes the same ascending 32-wide MFMA chunks over K in both kernels and rounds at the same points."""
    from llamarec_amd._lib import check, lib, stream_ptr

    L = lib()
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + K + N)
    A = (torch.randn(M, K, generator=g, device="cuda")).to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g, device="cuda") * 0.05).to(torch.bfloat16)
    R = torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16)
    cs = rope_table
    pos = torch.randint(0, T_ROPE, (M,), generator=g, device="cuda", dtype=torch.int32)

    def run(epi, variant, rope_positions=T_ROPE, in_place=False):
        n_out = N // 2 if epi == 2 else N
        C = R.clone() if in_place else torch.full((M, n_out), float("nan"), dtype=torch.bfloat16, device="cuda")
        r = C if in_place else R
        check(L.lr_gemm_bf16_nt_epi(A.data_ptr(), B.data_ptr(), C.data_ptr(), r.data_ptr() if epi == 1 else None, M, N, K, epi,
                                    variant, pos.data_ptr(), cs.data_ptr(), rope_positions, HD, ROT_COLS if epi == 3 else 0, None, 0,
                                    stream_ptr()), "gemm")
        torch.cuda.synchronize()
        return C.view(torch.int16)

    for epi in (0, 1, 2, 3):
        ref = run(epi, 1)
        assert not torch.isnan(ref.view(torch.bfloat16).float()).any(), epi
        assert torch.equal(ref, run(epi, 4)), (epi, K, M, N)
    assert torch.equal(run(1, 4, in_place=True), run(1, 1)), ("residual in place", K, M, N)
    assert torch.equal(run(3, 4, rope_positions=0), run(3, 1)), ("rotary without the packed table", K, M, N)


def dev_bf16(x):
    return torch.from_numpy(f32_to_bf16_bits(x).view(np.int16)).cuda()


def gemm_ws(A, B, variant):
    from llamarec_amd._lib import check, lib, stream_ptr

    M, K = A.shape
    N = B.shape[0]
    a, b = dev_bf16(A), dev_bf16(B)
    c = torch.full((M, N), 0x7FC0, dtype=torch.int16, device="cuda")  # NaN poison
    ws = torch.full(((8 << 20) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    check(lib().lr_gemm_bf16_nt_ws(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, variant, ws.data_ptr(), ws.numel() * 4,
                                   stream_ptr()), "gemm")
    torch.cuda.synchronize()
    return bf16_bits_to_f32(c.cpu().numpy().view(np.uint16))


def test_splitk_runs_of_16_and_17_k_tiles_starting_past_tile_0():
    """Latency mode on one 256 x 256 tile with K = 2112 = 33 K tiles: the policy splits in two (>= 16 tiles per split), K tiles
    [0, 16) and [16, 33) -- an even and an odd run, the second with kt_first = 16. Against the generic kernel within the
    bound of test_gemm_splitk_latency_mode: one bf16 ulp of the result plus fp32 accumulation noise 2e-6 sum_k |a||b| (the
    two kernels add the same products in a different association), and more than 0.9 of the values identical."""
    M, N, K = 256, 256, 2112
    A = bf16_round(hash_uniform(M * 7 + K, (M, K), 1.0))
    B = bf16_round(hash_uniform(N * 13 + K, (N, K), 1.0))
    ref = gemm_ws(A, B, 1)
    got = gemm_ws(A, B, 5)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    err = np.abs(got - ref)
    tol = np.maximum(np.abs(ref), 1e-3) * 2.0 ** -7 + 2e-6 * (np.abs(A) @ np.abs(B).T)
    print(f"split-K vs generic: max err {err.max():.3e}, worst err/tol {(err / tol).max():.3f}, equal {(got == ref).mean():.4f}")
    assert (err <= tol).all(), f"max err {err.max()} (worst ratio {(err / tol).max()})"
    assert (got == ref).mean() > 0.9


def test_small_integer_product_equals_numpy_int64():
    """|a| <= 4, |b| <= 2, K = 320 (five K tiles), M = 257, N = 512: every partial sum is an integer below 2^24, so the fp32
    accumulation is exact in any order and the only rounding is the bf16 store of the exact sum. The reference is numpy's int64
    product, rounded to bf16 the same way (sums beyond 256 need more than bf16's 8 significant bits): independent of the
    generic kernel, and any stale or half-landed LDS tile gives a different integer."""
    M, N, K = 257, 512, 320
    rng = np.random.default_rng(320)
    Ai = rng.integers(-4, 5, size=(M, K), dtype=np.int64)
    Bi = rng.integers(-2, 3, size=(N, K), dtype=np.int64)
    ref = bf16_round((Ai @ Bi.T).astype(np.float32))
    got = gemm_ws(Ai.astype(np.float32), Bi.astype(np.float32), 4)
    assert np.array_equal(got, ref), f"{(got != ref).sum()} of {got.size} values differ"
