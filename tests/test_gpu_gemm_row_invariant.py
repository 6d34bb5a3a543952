"""GPU: GEMM variant 7, split-K whose arithmetic for a row does not depend on the launch's row count (llama_gemm.hip, DESIGN
16 "Latency mode"). Its split is what variant 5 chooses at one row tile, and its rows are launched in chunks of as many
256-row tiles as the split-K workspace holds. So variant 7 on M rows must give, BIT FOR BIT, what variant 5 gives on each
256-row slice run as a product of its own, whatever the workspace makes the chunk boundaries.

Shape: N = 512, K = 1024 with LR_GEMM_SPLITK_MIN_TILES=2 -- two column tiles, 16 K tiles, S = 8 runs of two K tiles. One row
tile's planes are 8 x 256 x 512 x 4 bytes = 4 MiB: with exactly that the 600-row product is three launches, with 16 MiB it is
one launch of three row tiles. No tolerance here: variant 7 equals variant 5 slice by slice, so it inherits the float64 bounds
tests/test_gpu_stage2_bounds.py asserts for variant 5."""
import ctypes as C

import numpy as np
import pytest
import torch

from llamarec_amd.synth import f32_to_bf16_bits, hash_uniform

pytestmark = pytest.mark.gpu

LR_EWORKSPACE = -4
N, K, HD, ROT_COLS, T = 512, 1024, 128, 256, 700
MS = [1, 200, 256, 257, 600]
ONE_TILE = 8 * 256 * N * 4
STORE, RESIDUAL, SWIGLU, ROPE = 0, 1, 2, 3
_DATA = {}


@pytest.fixture
def two_k_tile_runs(monkeypatch):
    monkeypatch.setenv("LR_GEMM_SPLITK_MIN_TILES", "2")   # monkeypatch puts the environment back
    yield


def _dev(x):
    return torch.from_numpy(f32_to_bf16_bits(np.asarray(x, np.float32)).view(np.int16)).cuda()


def _data():
    """Operands for the largest M, on the device, built once: every smaller product reads their first rows."""
    if not _DATA:
        from llamarec_amd._lib import check, lib, stream_ptr

        M = max(MS)
        L = lib()
        cs = torch.full((L.lr_rope_table_bytes(T, HD) // 4,), float("nan"), dtype=torch.float32, device="cuda")
        check(L.lr_rope_table(cs.data_ptr(), T, HD, 10000.0, stream_ptr()), "rope table")
        pos = np.random.default_rng(3).permutation(T)[:M].astype(np.int32)   # shuffled, not monotone
        _DATA.update(A=_dev(hash_uniform(71, (M, K), 1.0)), B=_dev(hash_uniform(72, (N, K), 0.05)),
                     R=_dev(hash_uniform(73, (M, N), 2.0)), w=_dev(hash_uniform(74, (N,), 0.5) + 1.0), cs=cs,
                     pos=torch.from_numpy(pos).cuda(), ws=torch.empty(16 << 20, dtype=torch.uint8, device="cuda"), ref={})
        torch.cuda.synchronize()
    return _DATA


def _epi(d, epi, variant, lo, hi, ws_bytes, fill=0x7FC0):
    """Rows lo .. hi - 1 as one product. Returns (rc, C [hi - lo][n_out] int16 on the host)."""
    from llamarec_amd._lib import lib, stream_ptr

    M = hi - lo
    out = torch.full((M, N // 2 if epi == SWIGLU else N), fill, dtype=torch.int16, device="cuda")
    rc = lib().lr_gemm_bf16_nt_epi(d["A"][lo:hi].data_ptr(), d["B"].data_ptr(), out.data_ptr(),
                                   d["R"][lo:hi].data_ptr() if epi == RESIDUAL else None, M, N, K, epi, variant,
                                   d["pos"][lo:hi].data_ptr() if epi == ROPE else None, d["cs"].data_ptr() if epi == ROPE else None,
                                   T if epi == ROPE else 0, HD if epi == ROPE else 0, ROT_COLS if epi == ROPE else 0,
                                   d["ws"].data_ptr(), ws_bytes, stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _norm(d, variant, lo, hi, ws_bytes):
    """Residual + RMSNorm in the reduce pass. Returns (rc, was_fused, C, norm_out)."""
    from llamarec_amd._lib import lib, stream_ptr

    M = hi - lo
    out = torch.full((M, N), 0x7FC0, dtype=torch.int16, device="cuda")
    xn = torch.full((M, N), 0x7FC0, dtype=torch.int16, device="cuda")
    was = C.c_int32(-1)
    rc = lib().lr_gemm_bf16_nt_residual_rmsnorm_ex(d["A"][lo:hi].data_ptr(), d["B"].data_ptr(), out.data_ptr(),
                                                   d["R"][lo:hi].data_ptr(), M, N, K, variant, d["w"].data_ptr(), xn.data_ptr(),
                                                   1e-5, 0, 1, C.byref(was), d["ws"].data_ptr(), ws_bytes, stream_ptr())
    torch.cuda.synchronize()
    return rc, was.value, out.cpu().numpy(), xn.cpu().numpy()


def _slices(M):
    return [(lo, min(lo + 256, M)) for lo in range(0, M, 256)]


def _variant5(d, what, lo, hi):
    """Variant 5 on the slice as a product of its own (one row tile: S = 8), computed once per slice."""
    key = (what, lo, hi)
    if key not in d["ref"]:
        if what == "norm":
            rc, was, c, xn = _norm(d, 5, lo, hi, 16 << 20)
            assert rc == 0 and was == 1
            d["ref"][key] = (c, xn)
        else:
            rc, c = _epi(d, what, 5, lo, hi, 16 << 20)
            assert rc == 0
            d["ref"][key] = (c,)
    return d["ref"][key]


def _plan(variant, M, ws_bytes):
    from llamarec_amd._lib import lib

    s, r = C.c_int32(0), C.c_int32(0)
    return lib().lr_gemm_splitk_plan(variant, M, N, K, ws_bytes, C.byref(s), C.byref(r)), s.value, r.value


def test_the_shape_splits_as_the_docstring_says(two_k_tile_runs):
    for M in MS:
        assert _plan(7, M, ONE_TILE) == (0, 8, 256) and _plan(7, M, 16 << 20) == (0, 8, 1024), M
    assert _plan(5, 256, 16 << 20) == (0, 8, 256) and _plan(5, 88, 16 << 20) == (0, 8, 88)


@pytest.mark.parametrize("ws_bytes", [ONE_TILE, 16 << 20], ids=["ws4MiB", "ws16MiB"])
@pytest.mark.parametrize("epi", [STORE, RESIDUAL, ROPE, SWIGLU], ids=["store", "residual", "rope", "swiglu"])
def test_variant_7_equals_variant_5_slice_by_slice(two_k_tile_runs, epi, ws_bytes):
    d = _data()
    bad = []
    for M in MS:
        rc, got = _epi(d, epi, 7, 0, M, ws_bytes)
        assert rc == 0, (M, rc)
        assert not (got == 0x7FC0).all(axis=1).any(), (M, "a row was not written")
        for lo, hi in _slices(M):
            if not np.array_equal(got[lo:hi], _variant5(d, epi, lo, hi)[0]):
                bad.append((M, lo, hi))
    assert not bad, f"(M, slice) whose bits differ from variant 5 on the slice alone: {bad}"


@pytest.mark.parametrize("ws_bytes", [ONE_TILE, 16 << 20], ids=["ws4MiB", "ws16MiB"])
def test_variant_7_residual_with_fused_rmsnorm_equals_variant_5_slice_by_slice(two_k_tile_runs, ws_bytes):
    d = _data()
    bad = []
    for M in MS:
        rc, was, got_c, got_xn = _norm(d, 7, 0, M, ws_bytes)
        assert rc == 0 and was == 1, (M, rc, was)
        for lo, hi in _slices(M):
            c, xn = _variant5(d, "norm", lo, hi)
            if not (np.array_equal(got_c[lo:hi], c) and np.array_equal(got_xn[lo:hi], xn)):
                bad.append((M, lo, hi))
        # and the fused norm's C is the plain residual epilogue's
        assert np.array_equal(got_c, _epi(d, RESIDUAL, 7, 0, M, ws_bytes)[1]), M
    assert not bad, bad


def test_a_workspace_one_byte_short_of_a_row_tile_is_refused_before_any_launch(two_k_tile_runs):
    from llamarec_amd._lib import lib

    d = _data()
    for M in (1, 600):
        for epi in (STORE, ROPE):
            rc, got = _epi(d, epi, 7, 0, M, ONE_TILE - 1, fill=0x1234)
            assert rc == LR_EWORKSPACE and b"variant 7" in lib().lr_last_error(), (M, epi, rc)
            assert (got == 0x1234).all(), (M, epi, "C was written")
        rc, was, c, xn = _norm(d, 7, 0, M, ONE_TILE - 1)
        assert rc == LR_EWORKSPACE and was == -1 and (c == 0x7FC0).all() and (xn == 0x7FC0).all()


def test_variant_7_refuses_a_width_off_the_tile_where_variant_5_falls_back():
    """N = 320: variant 5 runs the generic kernel (variant 1's bits), variant 7 returns LR_EINVAL and writes nothing."""
    from llamarec_amd._lib import lib, stream_ptr

    d = _data()
    M, n = 130, 320
    outs = {}
    for variant in (1, 5, 7):
        out = torch.full((M, n), 0x1234, dtype=torch.int16, device="cuda")
        rc = lib().lr_gemm_bf16_nt_epi(d["A"].data_ptr(), d["B"].data_ptr(), out.data_ptr(), None, M, n, K, STORE, variant, None,
                                       None, 0, 0, 0, d["ws"].data_ptr(), 16 << 20, stream_ptr())
        torch.cuda.synchronize()
        outs[variant] = (rc, out.cpu().numpy())
    assert outs[1][0] == 0 and outs[5][0] == 0 and np.array_equal(outs[1][1], outs[5][1])
    assert outs[7][0] == -1 and (outs[7][1] == 0x1234).all()


def test_variant_7_without_the_override_does_not_split_and_equals_variant_4():
    """16 K tiles are one run of 16: S = 1, the product runs as variant 4 with no workspace at all."""
    import os

    assert "LR_GEMM_SPLITK_MIN_TILES" not in os.environ
    d = _data()
    assert _plan(7, 600, 0) == (0, 1, 600)
    for epi in (STORE, ROPE):
        rc7, got7 = _epi(d, epi, 7, 0, 600, 0)
        rc4, got4 = _epi(d, epi, 4, 0, 600, 0)
        assert rc7 == 0 and rc4 == 0 and np.array_equal(got7, got4)
