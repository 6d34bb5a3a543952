"""GPU: the two small kernels Gemma-3 adds beside its attention -- the q/k norm + rotation sweep in Gemma's rounding
(lr_qk_norm_rope_ex_bf16, norm_style 1) against the float64 restatement of tests/gemma3_ref.py within its bound, norm_style 0
against lr_qk_norm_rope_bf16 bit for bit, and the linearly scaled rotary table (lr_rope_table_ex, kind 2) inside
tests/stage2_ref.py's acceptance band computed with inv_freq / factor."""
import ctypes

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, f32_to_bf16_bits, hash_uniform
from tests import gemma3_ref as G3

pytestmark = pytest.mark.gpu

LR_EINVAL = -1
ROWS, NQ, NK, TMAX = 70, 3, 2, 400     # 70 rows x 5 heads: more than one workgroup at either head_dim, a ragged last one


def sweep_data(hd):
    """x [rows][nq + nk][hd] (bf16 values, rows of very different size), w [hd] around 0 with a wide spread (packed order),
    positions, HF's bf16 table of theta 10 000, eps."""
    from tests.stage2_ref import rope_table_hf

    x = hash_uniform(9100 + hd, (ROWS, NQ + NK, hd), 1.0) * (2.0 ** hash_uniform(9200 + hd, (ROWS, 1, 1), 2.0))
    w = hash_uniform(9300 + hd, (hd,), 0.75)
    pos = (np.arange(ROWS) * 37 % TMAX).astype(np.int32)
    cos, sin, _, _ = rope_table_hf(TMAX, hd, 10000.0)
    return bf16_round(x.astype(np.float32)), bf16_round(w), pos, cos, sin, 1e-6


def _bits(x):
    return torch.from_numpy(f32_to_bf16_bits(np.ascontiguousarray(x, dtype=np.float32)).view(np.int16)).cuda()


def _lib():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def _table(hd):
    L, st = _lib()
    cs = torch.empty(L.lr_rope_table_bytes(TMAX, hd), dtype=torch.uint8, device="cuda")
    assert L.lr_rope_table(cs.data_ptr(), TMAX, hd, 10000.0, st) == 0
    return cs


def _sweep(hd, style, ex=True, tail_cols=8):
    """The sweep on [rows][(nq + nk) hd + tail_cols] (the tail must keep its bits): bf16 bits of the head columns."""
    L, st = _lib()
    x, w, pos, _, _, eps = sweep_data(hd)
    ld = (NQ + NK) * hd + tail_cols
    buf = np.full((ROWS, ld), 3.0, np.float32)
    buf[:, :(NQ + NK) * hd] = x.reshape(ROWS, -1)
    buf_d, w_d, pos_d, cs = _bits(buf), _bits(w), torch.from_numpy(pos).cuda(), _table(hd)
    args = (buf_d.data_ptr(), ROWS, ld, 0, NQ, NK, hd, w_d.data_ptr(), w_d.data_ptr(), eps, pos_d.data_ptr(), cs.data_ptr(), st)
    rc = L.lr_qk_norm_rope_ex_bf16(*args, style) if ex else L.lr_qk_norm_rope_bf16(*args)
    torch.cuda.synchronize()
    got = buf_d.cpu().numpy()
    if rc == 0:
        assert (bf16_bits_to_f32(got[:, (NQ + NK) * hd:].view(np.uint16)) == 3.0).all(), "columns behind the heads written"
    return rc, got[:, :(NQ + NK) * hd]


@pytest.mark.parametrize("hd", [256, 128])
def test_sweep_in_gemmas_rounding_is_within_the_float64_bound_and_the_llama_mutant_is_not(hd):
    x, w, pos, cos, sin, eps = sweep_data(hd)
    rc, bits = _sweep(hd, 1)
    assert rc == 0, _lib()[0].lr_last_error()
    got = bf16_bits_to_f32(bits.view(np.uint16)).reshape(ROWS, NQ + NK, hd)
    assert np.isfinite(got).all()
    ref, bound = G3.qk_norm_rope_ref64(x, w, eps, pos, cos, sin)
    r = G3.ratio(got, ref, bound)
    print(f"q/k norm sweep, norm_style 1, head_dim {hd}: max(err / bound) {r:.3f}")
    assert r <= 1.0, r
    mref, mbound = G3.qk_norm_rope_ref64(x, w, eps, pos, cos, sin, "llama_qk_norm")
    assert G3.ratio(got, mref, mbound) > 1.0


@pytest.mark.parametrize("hd", [256, 128, 64])
def test_style_0_is_the_existing_call_bit_for_bit_and_other_styles_are_refused(hd):
    rc0, old = _sweep(hd, 0, ex=False)
    rc1, new = _sweep(hd, 0)
    assert rc0 == 0 and rc1 == 0 and np.array_equal(old, new)
    rc2, gemma = _sweep(hd, 1)
    assert rc2 == 0 and not np.array_equal(gemma, old)
    for style in (2, -1):
        rc, untouched = _sweep(hd, style)
        x = sweep_data(hd)[0]
        assert rc == LR_EINVAL and np.array_equal(untouched.view(np.uint16), f32_to_bf16_bits(x.reshape(ROWS, -1)))


@pytest.mark.parametrize("hd, theta, factor", [(256, 1000000.0, 8.0), (128, 1000000.0, 8.0), (256, 10000.0, 2.5)])
def test_linear_rope_table_sits_inside_the_acceptance_band(hd, theta, factor, monkeypatch):
    from llamarec_amd import _abi as A
    from tests import stage2_ref as R

    T = 700
    plain = R.rope_table_hf

    def scaled(T_, hd_, theta_):     # HF: inv_freq / factor in fp32, then the angles
        inv = (plain(T_, hd_, theta_)[2] / np.float32(factor)).astype(np.float32)
        ang = (np.arange(T_, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
        return bf16_round(np.cos(ang).astype(np.float32)), bf16_round(np.sin(ang).astype(np.float32)), inv, ang

    monkeypatch.setattr(R, "rope_table_hf", scaled)
    clo, chi, slo, shi = R.rope_band(T, hd, theta)
    L, st = _lib()
    cs = torch.empty(L.lr_rope_table_bytes(T, hd), dtype=torch.uint8, device="cuda")
    words = A.LrRopeScaling(kind=2, factor=factor)
    assert L.lr_rope_table_ex(cs.data_ptr(), T, hd, theta, ctypes.byref(words), st) == 0, L.lr_last_error()
    torch.cuda.synchronize()
    raw = cs.cpu().numpy()
    f = raw[: T * hd * 4].view(np.float32).reshape(T, hd // 2, 2).astype(np.float64)
    assert ((f[..., 0] >= clo) & (f[..., 0] <= chi)).all() and ((f[..., 1] >= slo) & (f[..., 1] <= shi)).all()
    packed = raw[T * hd * 4:].view(np.uint32).reshape(T, hd // 2)      # the same values as bf16 pairs
    assert np.array_equal(bf16_bits_to_f32((packed & 0xFFFF).astype(np.uint16)), f[..., 0].astype(np.float32))
    assert np.array_equal(bf16_bits_to_f32((packed >> 16).astype(np.uint16)), f[..., 1].astype(np.float32))
    # the unscaled table is far outside this band at large positions
    one = torch.empty_like(cs)
    ref = torch.empty_like(cs)
    assert L.lr_rope_table(ref.data_ptr(), T, hd, theta, st) == 0
    torch.cuda.synchronize()
    g = ref.cpu().numpy()[: T * hd * 4].view(np.float32).reshape(T, hd // 2, 2).astype(np.float64)
    assert not ((g[..., 0] >= clo) & (g[..., 0] <= chi)).all()
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        assert L.lr_rope_table_ex(one.data_ptr(), T, hd, theta, ctypes.byref(A.LrRopeScaling(kind=2, factor=bad)), st) == LR_EINVAL
    for unread in (dict(low_freq_factor=1.0), dict(high_freq_factor=4.0), dict(original_max_positions=8192)):   # must be zero
        words = A.LrRopeScaling(kind=2, factor=factor, **unread)
        assert L.lr_rope_table_ex(one.data_ptr(), T, hd, theta, ctypes.byref(words), st) == LR_EINVAL, unread
