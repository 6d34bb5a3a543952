"""The 256x256x64 GEMM's K loop where a global->LDS DMA piece, its counted wait and the drain of a run meet.

test_gpu_gemm_two_phase.py covers 1..5 K tiles and split-K runs of 16 and 17. Here: six and seven K tiles (K = 384, 448),
so that the pieces of tiles t+1 and t+2 exist in every combination of `more` / `more2` (RB_TILE of llama_gemm.hip) for an
even and an odd trip end, for every epilogue; split-K runs of one and two K tiles starting at even and odd kt_first (the
shortest runs there are: prologue, in-flight pieces and drain in one or two tiles); and one product with more workgroups
than CUs and sixteen K tiles, run twice, against the generic kernel and numpy's int64 product. A wrong wait count or a race
gives wrong numbers, not a fault: identical bits are the criterion everywhere.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llamarec_amd.synth import f32_to_bf16_bits

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
@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("K", [384, 448])
def test_every_epilogue_equals_generic_kernel_bit_for_bit_at_6_and_7_k_tiles(K, M, N, rope_table):
    """Call pattern of test_gpu_gemm_two_phase.py: variant 4 against variant 1 for store, residual, SwiGLU, rotary and
    GeGLU, the residual also in place and the rotary also without the packed table."""
    from llamarec_amd._lib import check, lib, stream_ptr

    L = lib()
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + K + N)
    A = (torch.randn(M, K, generator=g, device="cuda")).to(torch.bfloat16)
    B = (torch.randn(N, K, generator=g, device="cuda") * 0.05).to(torch.bfloat16)
    R = torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16)
    cs = rope_table
    pos = torch.randint(0, T_ROPE, (M,), generator=g, device="cuda", dtype=torch.int32)

    def run(epi, variant, rope_positions=T_ROPE, in_place=False):
        n_out = N // 2 if epi in (2, 5) else N
        C = R.clone() if in_place else torch.full((M, n_out), float("nan"), dtype=torch.bfloat16, device="cuda")
        r = C if in_place else R
        check(L.lr_gemm_bf16_nt_epi(A.data_ptr(), B.data_ptr(), C.data_ptr(), r.data_ptr() if epi == 1 else None, M, N, K, epi,
                                    variant, pos.data_ptr(), cs.data_ptr(), rope_positions, HD, ROT_COLS if epi == 3 else 0, None, 0,
                                    stream_ptr()), "gemm")
        torch.cuda.synchronize()
        return C.view(torch.int16)

    for epi in (0, 1, 2, 3, 5):
        ref = run(epi, 1)
        assert not torch.isnan(ref.view(torch.bfloat16).float()).any(), epi
        assert torch.equal(ref, run(epi, 4)), (epi, K, M, N)
    assert torch.equal(run(1, 4, in_place=True), run(1, 1)), ("residual in place", K, M, N)
    assert torch.equal(run(3, 4, rope_positions=0), run(3, 1)), ("rotary without the packed table", K, M, N)


def dev_bf16(x):
    return torch.from_numpy(f32_to_bf16_bits(x).view(np.int16)).cuda()


def gemm_ws(a, b, M, N, K, variant):
    from llamarec_amd._lib import check, lib, stream_ptr

    c = torch.full((M, N), 0x7FC0, dtype=torch.int16, device="cuda")  # NaN poison
    ws = torch.full(((8 << 20) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    check(lib().lr_gemm_bf16_nt_ws(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, variant, ws.data_ptr(), ws.numel() * 4,
                                   stream_ptr()), "gemm")
    torch.cuda.synchronize()
    return c.cpu().numpy().view(np.uint16)


def small_ints(seed, M, N, K):
    """|a| <= 4, |b| <= 2: every partial sum is an integer below 2^24 for K <= 2^21, so fp32 accumulation is exact in any
    order and association; the only rounding is the bf16 store of the exact sum."""
    rng = np.random.default_rng(seed)
    Ai = rng.integers(-4, 5, size=(M, K), dtype=np.int64)
    Bi = rng.integers(-2, 3, size=(N, K), dtype=np.int64)
    if M * N * K <= 1 << 28:
        P = Ai @ Bi.T
    else:
        # numpy multiplies int64 matrices with a plain loop (tens of seconds at 4352 x 4096 x 1024): take the product in
        # float64 through BLAS -- exact as well, every partial sum is an integer below 2^53 -- and hold 64 rows spread over
        # the row tiles against the int64 loop
        P = (Ai.astype(np.float64) @ Bi.T.astype(np.float64)).astype(np.int64)
        rows = np.arange(0, M, M // 64)
        assert np.array_equal(P[rows], Ai[rows] @ Bi.T)
    ref = f32_to_bf16_bits(P.astype(np.float32))
    return dev_bf16(Ai.astype(np.float32)), dev_bf16(Bi.astype(np.float32)), ref


# K tiles T and the least tiles per split: one 256 x 256 tile splits S = min(8, T / least) ways, split s takes K tiles
# [s T / S, (s + 1) T / S).
#   T =  8, least 1: eight runs of one tile, kt_first = 0 .. 7 (four of them odd)
#   T = 16, least 2: eight runs of two tiles
#   T = 15, least 1: runs of 1, 2, 2, 2, 2, 2, 2, 2 tiles starting at kt_first = 0, 1, 3, 5, 7, 9, 11, 13
#   T = 23, least 1: runs of 2, 3, 3, 3, 3, 3, 3, 3 tiles starting at 0, 2, 5, 8, 11, 14, 17, 20
@pytest.mark.parametrize("T,least", [(8, 1), (16, 2), (15, 1), (23, 1)])
@pytest.mark.parametrize("M", [1, 256])
def test_splitk_runs_of_one_to_three_k_tiles_equal_numpy_int64(M, T, least, monkeypatch):
    """Small-integer operands make the sum exact whatever the association, so split-K (fp32 partial planes summed in order)
    has to give the bits of numpy's int64 product, and of the generic kernel. LR_GEMM_SPLITK_MIN_TILES (read per call)
    lowers the policy's 16 K tiles per split for this test."""
    N, K = 256, 64 * T
    a, b, ref = small_ints(T * 100 + M, M, N, K)
    monkeypatch.setenv("LR_GEMM_SPLITK_MIN_TILES", str(least))
    got = gemm_ws(a, b, M, N, K, 5)
    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES")
    assert np.array_equal(got, ref), f"{(got != ref).sum()} of {got.size} values differ from the int64 product"
    assert np.array_equal(gemm_ws(a, b, M, N, K, 1), ref)


def test_more_workgroups_than_cus_16_k_tiles_twice_equal_generic_and_numpy_int64():
    """M = 4352, N = 4096: 272 tiles on 256 CUs, so CUs run a second workgroup while others still run their first;
    K = 1024 = sixteen K tiles. Small-integer operands: the int64 product is the reference, the generic kernel has to agree
    with it too, and two runs of the fast kernel have to give the same bits."""
    M, N, K = 4352, 4096, 1024
    a, b, ref = small_ints(4352, M, N, K)
    first = gemm_ws(a, b, M, N, K, 4)
    second = gemm_ws(a, b, M, N, K, 4)
    generic = gemm_ws(a, b, M, N, K, 1)
    assert np.array_equal(generic, ref), f"generic kernel: {(generic != ref).sum()} of {ref.size} values differ from the int64 product"
    assert np.array_equal(first, ref), f"run 1: {(first != ref).sum()} of {ref.size} values differ from the int64 product"
    assert np.array_equal(second, ref), f"run 2: {(second != ref).sum()} of {ref.size} values differ from the int64 product"
    assert np.array_equal(first, generic) and np.array_equal(first, second)
