"""CPU: lr_gemm_splitk_plan, what lr_launch_gemm does with a product under the split-K variants (include/llamarec_mi355x.h,
DESIGN 16 "Latency mode"). Variant 5 chooses its number of K splits from ceil(M / 256) * (N / 256); variant 7 takes what
variant 5 chooses at ONE row tile, whatever M is, and launches the rows in chunks of as many 256-row tiles as the split-K
workspace holds. The library is loaded without a GPU; the function launches nothing."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_EINVAL, LR_EWORKSPACE = -1, -4
WS = 64 << 20   # LR_SPLITK_WS_BYTES, what a prefill workspace carries
# Llama-2-7b (hidden 4096, intermediate 11008, 32 heads of 128): (N, K) of the four products
LLAMA2_7B = {"qkv": (12288, 4096), "o_proj": (4096, 4096), "gate_up": (22016, 4096), "down": (4096, 11008)}
ROWS = [1, 160, 256, 257, 460, 2048]


def _plan(variant, M, N, K, ws=WS):
    from llamarec_amd import _lib

    s, r = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.lib().lr_gemm_splitk_plan(variant, M, N, K, ws, C.byref(s), C.byref(r))
    return rc, s.value, r.value


def test_header_prototype_and_library_agree():
    from llamarec_amd import _lib

    header = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    decl = re.search(r"\bint lr_gemm_splitk_plan\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert decl
    assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(_lib.PROTOTYPES["lr_gemm_splitk_plan"][1]) == 7
    assert hasattr(_lib.lib(), "lr_gemm_splitk_plan")


def test_variant_7_splits_by_the_weights_shape_alone(monkeypatch):
    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES", raising=False)
    want = {"qkv": 4, "o_proj": 4, "gate_up": 2, "down": 8}
    for name, (N, K) in LLAMA2_7B.items():
        for M in ROWS:
            rc, s7, rows = _plan(7, M, N, K)
            assert rc == 0 and s7 == want[name], (name, M, rc, s7)
            # the rows of a launch: whole row tiles, at least one, and their S planes fit the workspace; one tile more would not
            assert rows > 0 and rows % 256 == 0 and s7 * rows * N * 4 <= WS < s7 * (rows + 256) * N * 4, (name, M, rows)
            if M <= 256:   # one row tile: variant 5's split by construction, all rows in its one launch
                assert _plan(5, M, N, K) == (0, s7, M), (name, M)


def test_variant_5_splits_by_the_row_count_which_is_why_7_exists(monkeypatch):
    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES", raising=False)
    N, K = LLAMA2_7B["qkv"]
    assert _plan(5, 300, N, K) == (0, 2, 300)     # 2 row tiles x 48 column tiles: 256 // 96
    assert _plan(7, 300, N, K)[:2] == (0, 4)      # 48 column tiles: min(256 // 48, 4096 / 64 / 16)
    assert _plan(5, 160, N, K)[:2] == (0, 4)      # the session's 160 new rows and its 460-row whole prompt differ under 5 ...
    assert _plan(5, 460, N, K)[:2] == (0, 2)
    assert _plan(7, 160, N, K)[:2] == _plan(7, 460, N, K)[:2] == (0, 4)   # ... and agree under 7


def test_products_that_do_not_split(monkeypatch):
    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES", raising=False)
    for variant in (5, 7):
        assert _plan(variant, 300, 4096, 1024) == (0, 1, 300)      # 16 K tiles: fewer than 2 runs of 16
        assert _plan(variant, 300, 256 * 129, 4096) == (0, 1, 300)  # more than 128 tiles in one row of tiles
        assert _plan(variant, 300, 4096, 1024, ws=0) == (0, 1, 300)  # and an unsplit product needs no workspace
    assert _plan(5, 40000, 4096, 4096) == (0, 1, 40000)            # 157 x 16 tiles fill the card ...
    assert _plan(7, 40000, 4096, 4096)[:2] == (0, 4)                # ... variant 7 splits all the same: the price of its contract


def test_widths_off_the_tile_fall_back_under_5_and_are_refused_under_7(monkeypatch):
    """Variant 5 sends them to the generic kernel as auto does (no split); variant 7 names one route and returns LR_EINVAL."""
    from llamarec_amd import _lib

    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES", raising=False)
    for N, K in ((896, 4096), (320, 192), (4096, 4000)):   # N off the 256 tile, both, K off the 64 tile
        assert _plan(5, 300, N, K) == (0, 1, 300), (N, K)
        assert _plan(7, 300, N, K) == (LR_EINVAL, -7, -7), (N, K)
        assert b"256 tile" in _lib.lib().lr_last_error()


def test_workspace_below_one_row_tile_is_refused(monkeypatch):
    from llamarec_amd import _lib

    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES", raising=False)
    N, K = LLAMA2_7B["o_proj"]
    one_tile = 4 * 256 * N * 4
    assert _plan(7, 460, N, K, ws=one_tile) == (0, 4, 256)
    assert _plan(7, 460, N, K, ws=2 * one_tile - 1) == (0, 4, 256)
    assert _plan(7, 460, N, K, ws=2 * one_tile) == (0, 4, 512)
    for ws in (one_tile - 1, 0):
        rc, s, rows = _plan(7, 460, N, K, ws=ws)
        assert rc == LR_EWORKSPACE and (s, rows) == (-7, -7), (ws, rc, s, rows)
        msg = _lib.lib().lr_last_error()
        assert b"variant 7" in msg and str(one_tile).encode() in msg, msg
    # variant 5 needs all M rows at once
    assert _plan(5, 160, N, K, ws=4 * 160 * N * 4) == (0, 4, 160)
    assert _plan(5, 160, N, K, ws=4 * 160 * N * 4 - 1)[0] == LR_EWORKSPACE
    assert b"variant 5" in _lib.lib().lr_last_error()


@pytest.mark.parametrize("min_tiles,want", [("1", 8), ("2", 8), ("4", 4), ("8", 2), ("16", 1), ("0", 1), ("junk", 1)])
def test_min_tiles_override_moves_both_variants_alike(monkeypatch, min_tiles, want):
    """N = 512, K = 1024: 2 column tiles and 16 K tiles. Without the override 16 K tiles are one run: no split."""
    monkeypatch.setenv("LR_GEMM_SPLITK_MIN_TILES", min_tiles)
    for M in (1, 200, 256):
        assert _plan(5, M, 512, 1024)[:2] == _plan(7, M, 512, 1024)[:2] == (0, want), (M, min_tiles)
    assert _plan(7, 600, 512, 1024)[:2] == (0, want)
    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES")
    assert _plan(5, 200, 512, 1024)[:2] == _plan(7, 200, 512, 1024)[:2] == (0, 1)


def test_bad_arguments():
    from llamarec_amd import _lib

    for variant in (0, 1, 4, 6, 8):
        assert _plan(variant, 160, 4096, 4096)[0] == LR_EINVAL
    for M, N, K in ((0, 4096, 4096), (160, 0, 4096), (160, 4096, -64)):
        assert _plan(7, M, N, K)[0] == LR_EINVAL
    s = C.c_int32(0)
    assert _lib.lib().lr_gemm_splitk_plan(7, 160, 4096, 4096, WS, None, C.byref(s)) == LR_EINVAL
    assert _lib.lib().lr_gemm_splitk_plan(7, 160, 4096, 4096, WS, C.byref(s), None) == LR_EINVAL
