"""GPU: sliding-window causal attention (Gemma-3's sliding layers) through lr_attention_varlen_window and
lr_attention_last_rows_window: the windowed head_dim-256 MFMA kernels (llama_attn_hd256_window.hip; variants 0 / 4) and the
generic kernel with a window (variant 1, and any other head_dim), against the float64 reference of tests/gemma3_ref.py within
its element-wise bound. The batches are tests/test_gemma3_host.py's too, which proves from the reference alone that they meet
every hazard of the block walk and that each mutant of the reference is outside the bound."""
import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, f32_to_bf16_bits
from tests import gemma3_ref as G3

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
WINDOWS = [1, 16, 17, 63, 64, 65, 100, 128, 200]
LENS = [1, 15, 64, 65, 127, 128, 129, 200, 321, 450]      # 1 500 rows per call
LAST_LENS = [1, 15, 63, 64, 65, 100, 127, 129, 200, 321]  # both sides of every window above and of the 64-key block
HEADS = [(4, 1), (2, 2), (8, 4)]
MUTANT_W = 16       # the small window the mutants are shown on
POISON = 0x7FC0     # bf16 NaN
GUARD = 3           # rows behind `out` that must keep their bits


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def spike_case(W=100, T=450, row=400):
    """(cu, row, key inside the window, key just outside it): the tile of `row` (rows 384..) first visits block
    (384 - W + 1) // 64 = 4; key 350 lies in block 5, behind it, and key row - W = 300 is the last one outside the window."""
    return cu_of([70, T]), row, 350, row - W


def spiked(qkv, cu, nh, nkv, hd, row, key, gain=2.0):
    """qkv with K[key] = gain * Q[row] for every KV head (its group's first query head): that one score is about
    gain * |q|^2 / sqrt(hd) ~ 16 gain natural units, far past the deferred-maximum threshold of 2^8."""
    out = qkv.copy()
    s0 = int(cu[1])
    rep = nh // nkv
    for g in range(nkv):
        q = out[s0 + row, g * rep * hd:(g * rep + 1) * hd]
        out[s0 + key, (nh + g) * hd:(nh + g + 1) * hd] = gain * q
    return bf16_bits_to_f32(f32_to_bf16_bits(out))


def _bits(x):
    return torch.from_numpy(f32_to_bf16_bits(x).view(np.int16)).cuda()


def _lib():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def _window_call(qkv_d, cu, nh, nkv, hd, W, variant, prefix_len=0):
    L, st = _lib()
    n = int(cu[-1])
    out = torch.full((n + GUARD, nh * hd), POISON, dtype=torch.int16, device="cuda")
    cud = torch.from_numpy(np.ascontiguousarray(cu, dtype=np.int32)).cuda()
    cu32 = np.ascontiguousarray(cu, dtype=np.int32)
    rc = L.lr_attention_varlen_window(qkv_d.data_ptr(), out.data_ptr(), cud.data_ptr(), cu32.ctypes.data, len(cu) - 1, prefix_len,
                                      nh, nkv, hd, W, variant, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:].view(np.uint16) == POISON).all(), "guard rows written"
    return rc, got[:n]


def _check(got_bits, ref, bound, what):
    """Finiteness first, on its own; then the bound."""
    got = bf16_bits_to_f32(got_bits.view(np.uint16))
    bad = np.flatnonzero(~np.isfinite(got).all(axis=1))
    assert bad.size == 0, (what, "rows with NaN / inf", bad[:8])
    r = G3.ratio(got, ref, bound)
    print(f"{what}: max(err / bound) {r:.3f}")
    assert r <= 1.0, (what, r)
    return got


_REF = {}


def _ref(regime, lens, nh, nkv, hd, W, mutant=None):
    key = (regime, tuple(lens), nh, nkv, hd, W, mutant)
    if key not in _REF:
        cu = cu_of(lens)
        _REF[key] = G3.attention_window_ref64(G3.window_data(regime, cu, nh, nkv, hd), cu, nh, nkv, hd, W, mutant)
    return _REF[key]


@pytest.mark.parametrize("regime", ["flat", "peaked"])
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "%dx%d" % h)
def test_windowed_attention_at_head_dim_256_is_within_the_float64_bound(heads, regime):
    nh, nkv = heads
    hd = 256
    cu = cu_of(LENS)
    assert cu[-1] <= 2000
    qkv_d = _bits(G3.window_data(regime, cu, nh, nkv, hd))
    for W in WINDOWS:
        ref, bound = _ref(regime, LENS, nh, nkv, hd, W)
        for variant in (4, 0, 1):
            rc, got = _window_call(qkv_d, cu, nh, nkv, hd, W, variant)
            assert rc == 0, (W, variant, _lib()[0].lr_last_error())
            _check(got, ref, bound, f"window attention {regime} {nh}x{nkv} W={W} v{variant}")


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_the_references_window_mutants_are_outside_the_bound_of_the_kernels_output(regime):
    nh, nkv, hd, W = 4, 1, 256, MUTANT_W
    cu = cu_of(LENS)
    qkv_d = _bits(G3.window_data(regime, cu, nh, nkv, hd))
    for variant in (4, 1):
        rc, got = _window_call(qkv_d, cu, nh, nkv, hd, W, variant)
        assert rc == 0
        got = bf16_bits_to_f32(got.view(np.uint16))
        for m in G3.WINDOW_MUTANTS:
            mref, mbound = _ref(regime, LENS, nh, nkv, hd, W, m)
            r = G3.ratio(got, mref, mbound)
            print(f"mutant {m} {regime} v{variant}: max(err / bound) {r:.1f}")
            assert r > 1.0, (m, variant, r)


@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "%dx%d" % h)
def test_a_spiked_key_moves_the_deferred_maximum_inside_the_window_and_does_nothing_outside_it(heads):
    nh, nkv = heads
    hd, W = 256, 100
    cu, row, key_in, key_out = spike_case(W)
    base = G3.window_data("flat", cu, nh, nkv, hd)
    for where, key in (("inside", key_in), ("outside", key_out)):
        qkv = spiked(base, cu, nh, nkv, hd, row, key)
        ref, bound = G3.attention_window_ref64(qkv, cu, nh, nkv, hd, W)
        if where == "outside":   # the reference itself: the spiked key changes no row's output but through its own row's K
            plain, _ = G3.attention_window_ref64(base, cu, nh, nkv, hd, W)
            assert np.array_equal(ref[int(cu[1]) + row], plain[int(cu[1]) + row])
        for variant in (4, 1):
            rc, got = _window_call(_bits(qkv), cu, nh, nkv, hd, W, variant)
            assert rc == 0
            _check(got, ref, bound, f"spike {where} the window {nh}x{nkv} v{variant}")


@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "%dx%d" % h)
def test_last_row_mode_writes_the_bits_of_each_prompts_last_row(heads):
    nh, nkv = heads
    hd = 256
    L, st = _lib()
    cu = cu_of(LAST_LENS)
    B = len(LAST_LENS)
    qkv = G3.window_data("peaked", cu, nh, nkv, hd)
    qkv_d = _bits(qkv)
    kv_d = _bits(np.ascontiguousarray(qkv[:, nh * hd:]))
    q_d = _bits(np.ascontiguousarray(qkv[cu[1:] - 1, :nh * hd]))
    cud = torch.from_numpy(cu).cuda()
    for W in WINDOWS:
        rc, whole = _window_call(qkv_d, cu, nh, nkv, hd, W, 4)
        assert rc == 0
        for variant in (4, 0):
            out = torch.full((B + GUARD, nh * hd), POISON, dtype=torch.int16, device="cuda")
            rc = L.lr_attention_last_rows_window(kv_d.data_ptr(), q_d.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, B,
                                                 0, nh, nkv, hd, W, variant, st)
            torch.cuda.synchronize()
            assert rc == 0, (W, variant, L.lr_last_error())
            got = out.cpu().numpy()
            assert (got[B:].view(np.uint16) == POISON).all(), "guard rows written"
            diff = np.flatnonzero((got[:B] != whole[cu[1:] - 1]).any(axis=1))
            assert diff.size == 0, (W, variant, "prompts whose last row differs", diff, [LAST_LENS[i] for i in diff])


def test_a_window_that_masks_nothing_writes_variant_4s_bits_and_bad_requests_are_refused():
    nh, nkv, hd = 4, 1, 256
    L, st = _lib()
    lens = [15, 129, 200, 70]
    cu = cu_of(lens)
    qkv_d = _bits(G3.window_data("flat", cu, nh, nkv, hd))
    cud = torch.from_numpy(cu).cuda()
    pinned = torch.full((int(cu[-1]), nh * hd), POISON, dtype=torch.int16, device="cuda")
    assert L.lr_attention_varlen(qkv_d.data_ptr(), pinned.data_ptr(), cud.data_ptr(), cu.ctypes.data, len(lens), nh, nkv, hd, 4,
                                 st) == 0
    torch.cuda.synchronize()
    pinned = pinned.cpu().numpy()
    for W in (0, -7, max(lens), max(lens) + 1, 1 << 30):
        rc, got = _window_call(qkv_d, cu, nh, nkv, hd, W, 4)
        assert rc == 0 and np.array_equal(got, pinned), W
    # one key fewer than the longest prompt: the windowed kernel, and other bits in that prompt's last row only
    rc, got = _window_call(qkv_d, cu, nh, nkv, hd, max(lens) - 1, 4)
    assert rc == 0 and not np.array_equal(got, pinned)
    # refusals: nothing is launched, the output keeps its bits
    for kw, want in ((dict(variant=2), LR_EUNSUPPORTED), (dict(variant=5), LR_EUNSUPPORTED), (dict(variant=9), LR_EUNSUPPORTED),
                     (dict(variant=3), LR_EUNSUPPORTED), (dict(prefix_len=15), LR_EUNSUPPORTED)):
        rc, got = _window_call(qkv_d, cu, nh, nkv, hd, 64, kw.get("variant", 4), kw.get("prefix_len", 0))
        assert rc == want and (got.view(np.uint16) == POISON).all(), (kw, rc)
    for bad in ([0, 15, 15, 200], [1, 15, 100, 200], [0, 100, 50, 200]):
        rc, got = _window_call(qkv_d, np.asarray(bad, np.int32), nh, nkv, hd, 64, 4)
        assert rc == LR_EINVAL and (got.view(np.uint16) == POISON).all(), bad
    out = torch.full((len(lens), nh * hd), POISON, dtype=torch.int16, device="cuda")
    for hd_, variant in ((128, 0), (256, 1), (256, 2)):   # the one-row mode with a window: head_dim 256 and variants 0 / 4 only
        rc = L.lr_attention_last_rows_window(qkv_d.data_ptr(), qkv_d.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data,
                                             len(lens), 0, nh, nkv, hd_, 64, variant, st)
        assert rc == LR_EUNSUPPORTED, (hd_, variant, rc)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint16) == POISON).all()


@pytest.mark.parametrize("hd", [64, 128])
def test_the_generic_kernel_with_a_window_is_within_the_bound_off_head_dim_256(hd):
    nh, nkv = 4, 2
    cu = cu_of(LENS)
    for regime in ("flat", "peaked"):
        qkv_d = _bits(G3.window_data(regime, cu, nh, nkv, hd))
        for W in (1, 17, 64, 100):
            ref, bound = _ref(regime, LENS, nh, nkv, hd, W)
            for variant in (1, 0):   # auto off head_dim 256 is the generic kernel too
                rc, got = _window_call(qkv_d, cu, nh, nkv, hd, W, variant)
                assert rc == 0, (W, variant, _lib()[0].lr_last_error())
                _check(got, ref, bound, f"generic window attention {regime} hd={hd} W={W} v{variant}")
