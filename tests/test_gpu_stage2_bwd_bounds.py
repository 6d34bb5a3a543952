"""GPU: the attention backward kernels (llama_attn_bwd.hip: the head_dim-128 MFMA passes, the generic kernel, the
deterministic owner kernel, each with and without the inverse rotation) against attention_bwd_ref64 of tests/stage2_ref.py,
element by element within the bound derived in that module's docstring. The reference is a function of the kernel's own
inputs (qkv, d_out and the forward's out / lse as handed over), so the forward's error is not part of the bound. Every run goes
through lr_attention_varlen_bwd_ex on a NaN-poisoned gradient with guard rows and a 0xFF-filled scratch of exactly the
advertised size with a guard behind it; every run prints max(err / bound) for dq, dk and dv, and each data set shows that the
mutants of the reference (one plausible kernel bug each) exceed the bound."""
import functools

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, f32_to_bf16_bits
from tests import stage2_ref as R

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED, LR_EWORKSPACE = -1, -2, -4
EDGE_BWD = [1, 63, 64, 65, 127, 128, 129, 191, 193, 256, 257, 600]   # 64-key / 128-query block edges, both ring parities
GENERIC_LENS = [1, 63, 64, 65, 129, 300]
REGIMES = ("flat", "peaked", "large_v", "last_block")
GUARD_ROWS, SCRATCH_GUARD, GUARD_BITS = 3, 4096, 0x5A5A

# (variant, deterministic): every way the kernels are reached, each run with and without the rotary table
RUNS_128 = [(2, 0), (0, 0), (3, 0), (1, 0), (1, 1)]          # 0 and 3 resolve to 2 at head_dim 128
RUNS_GENERIC = [(1, 0), (1, 1), (0, 0)]                      # 0 resolves to 1 elsewhere
RUNS = [(v, det, rope) for v, det in RUNS_128 for rope in (False, True)]


def _dev_bf16(x):
    return torch.from_numpy(f32_to_bf16_bits(x).view(np.int16)).cuda()


def _host(t):
    return bf16_bits_to_f32(t.cpu().numpy().view(np.uint16))


class _Inputs:
    """One data set on the device: qkv, d_out, the forward's out / lse, segments, each row's position inside its prompt."""

    def __init__(self, qkv, d_out, out, lse, cu, nh, nkv, hd):
        self.nh, self.nkv, self.hd = nh, nkv, hd
        self.cu = np.ascontiguousarray(cu, dtype=np.int32)
        self.n, self.B = int(cu[-1]), len(cu) - 1
        self.qkv, self.d_out, self.out = _dev_bf16(qkv), _dev_bf16(d_out), _dev_bf16(out)
        self.lse = torch.from_numpy(np.ascontiguousarray(lse, dtype=np.float32)).cuda()
        self.cud = torch.from_numpy(self.cu).cuda()
        self.pos = np.concatenate([np.arange(T) for T in np.diff(self.cu)]).astype(np.int32)
        self.pos_d = torch.from_numpy(self.pos).cuda()


def _bwd(x, variant, rope=None, det=0, entry="ex", tok_pos=True, short=0):
    """One backward call: (rc, dqkv as float32 [n][qw], its bits). dqkv is NaN-poisoned with guard rows behind it; scratch is
    exactly lr_attention_bwd_scratch_bytes (minus `short`) bytes of 0xFF with a guard behind it; both guards must survive.
    rope: (table tensor, positions) or None; entry "plain": the old entry point (no rope, not deterministic)."""
    from llamarec_amd._lib import lib, stream_ptr

    L = lib()
    qw = (x.nh + 2 * x.nkv) * x.hd
    buf = torch.full((x.n + GUARD_ROWS, qw), 0x7FC0, dtype=torch.int16, device="cuda")
    buf[x.n:] = GUARD_BITS
    sb = L.lr_attention_bwd_scratch_bytes(x.n, x.nh, x.nkv, x.hd)
    scratch = torch.full((sb + SCRATCH_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    args = (x.qkv.data_ptr(), x.out.data_ptr(), x.d_out.data_ptr(), x.lse.data_ptr(), buf.data_ptr(), x.cud.data_ptr(),
            x.cu.ctypes.data, x.B, x.nh, x.nkv, x.hd, variant, scratch.data_ptr(), sb - short)
    if entry == "plain":
        assert rope is None and not det
        rc = L.lr_attention_varlen_bwd(*args, stream_ptr())
    else:
        cs, positions = rope if rope is not None else (None, 0)
        rc = L.lr_attention_varlen_bwd_ex(*args, x.pos_d.data_ptr() if tok_pos else None,
                                          cs.data_ptr() if cs is not None else None, positions, det, stream_ptr())
    torch.cuda.synchronize()
    assert bool((buf[x.n:] == GUARD_BITS).all()), "rows behind dqkv were written"
    assert bool((scratch[sb:] == 0xFF).all()), "bytes behind the scratch were written"
    bits = buf[:x.n].cpu().numpy().view(np.uint16)
    return rc, bf16_bits_to_f32(bits), bits


def _rope_table(T, hd):
    """lr_rope_table for T positions: (device table, cos, sin as read back [T][hd/2])."""
    from llamarec_amd._lib import check, lib, stream_ptr

    L = lib()
    cs = torch.full((L.lr_rope_table_bytes(T, hd) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    check(L.lr_rope_table(cs.data_ptr(), T, hd, 10000.0, stream_ptr()), "rope table")
    torch.cuda.synchronize()
    f = cs[: T * hd].view(T, hd // 2, 2).cpu().numpy()
    return cs, f[..., 0].copy(), f[..., 1].copy()


@functools.lru_cache(maxsize=None)
def _dataset(regime, lens, nh, nkv, hd):
    """Inputs and references of one data set, computed once and shared (nothing below writes to them): out / lse are the float64
    forward rounded to bf16 / fp32; ref[False] / ref[True]: (dqkv, bound) without / with the rotation."""
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    qkv = R.attention_data(regime, cu, nh, nkv, hd)
    d_out = R.attention_bwd_data(cu, nh, hd)
    out64, lse64, _, _ = R.attention_ref64(qkv, cu, nh, nkv, hd)
    out, lse = bf16_round(out64.astype(np.float32)), lse64.astype(np.float32)
    x = _Inputs(qkv, d_out, out, lse, cu, nh, nkv, hd)
    T = int(max(lens))
    cs, cos, sin = _rope_table(T, hd)                     # exactly as many positions as the longest prompt has rows
    rope_ref = (x.pos, cos, sin)
    ref = {False: R.attention_bwd_ref64(qkv, d_out, out, lse, cu, nh, nkv, hd),
           True: R.attention_bwd_ref64(qkv, d_out, out, lse, cu, nh, nkv, hd, rope=rope_ref)}
    return dict(x=x, qkv=qkv, d_out=d_out, out=out, lse=lse, cu=cu, rope_dev=(cs, T), rope_ref=rope_ref, ref=ref)


def _report(tag, got, ref, bound, nh, nkv, hd, bad):
    r = R.bwd_ratios(got, ref, bound, nh, nkv, hd)
    print(f"{tag}: err/bound dq {r['dq']:.3f} dk {r['dk']:.3f} dv {r['dv']:.3f}")
    if not (np.isfinite(got).all() and max(r.values()) <= 1.0):
        bad.append((tag, r))


def _mutant_check(d, nh, nkv, hd):
    """Every applicable mutant of the reference, on the data set's longest prompt, exceeds the bound there (rows of a prompt
    depend on no other prompt, so the batch's reference and bound are sliced, not recomputed). In a one-prompt data set that
    prompt's last partial block lies inside the zero-d_out rows and contributes nothing: `tail` is the correct computation there
    and is left out, like gqa_mod where h % nkv is the group."""
    cu = d["cu"]
    b = int(np.argmax(np.diff(cu)))
    s0, e0 = int(cu[b]), int(cu[b + 1])
    z = R.zero_dout_rows(cu)
    tail_is_zero = z is not None and z.stop == e0 and (e0 - s0) % 64 <= R.ZERO_DOUT_ROWS
    one = np.array([0, e0 - s0])
    pos, cos, sin = d["rope_ref"]
    for with_rope in (False, True):
        rope = (pos[s0:e0], cos, sin) if with_rope else None
        ref, bound = d["ref"][with_rope]
        for m in R.BWD_MUTANTS:
            if not R.bwd_mutant_applies(m, nh, nkv, rope) or (m == "tail" and tail_is_zero):
                continue
            mo, _ = R.attention_bwd_ref64(d["qkv"][s0:e0], d["d_out"][s0:e0], d["out"][s0:e0], d["lse"][s0:e0], one, nh, nkv, hd,
                                          m, rope)
            r = max(R.bwd_ratios(mo, ref[s0:e0], bound[s0:e0], nh, nkv, hd).values())
            print(f"  reference mutant '{m}'{' rope' if with_rope else ''}: {r:.1f} x bound")
            assert r > 1.0, (m, r)


def _check_zero_rows(tag, got, cu, bad):
    """d_out is zero on these rows and on every later row of their prompt: their dq, and their dk / dv as keys, are exact
    zeros -- anything else is a contribution that crossed the causal mask or came from another row."""
    z = R.zero_dout_rows(cu)
    if z is not None and not (got[z] == 0.0).all():
        bad.append((tag, "zero-d_out rows", int(np.count_nonzero(got[z]))))


def _check_bwd(regime, lens, nh, nkv, hd, runs, kernel_forward=()):
    d = _dataset(regime, tuple(lens), nh, nkv, hd)
    x = d["x"]
    bad = []
    base = f"bwd {regime} hd={hd} nh={nh} nkv={nkv} T<={max(lens)}"
    for variant, det, with_rope in runs:
        rc, got, bits = _bwd(x, variant, d["rope_dev"] if with_rope else None, det)
        assert rc == 0, (variant, det, with_rope, rc)
        tag = f"{base} v{variant}{' det' if det else ''}{' rope' if with_rope else ''}"
        _report(tag, got, *d["ref"][with_rope], nh, nkv, hd, bad)
        _check_zero_rows(tag, got, d["cu"], bad)
        if (variant, det, with_rope) == (2, 0, False):   # the old entry point: the same bits (variant 2 has one owner per element)
            rc, _, bits_plain = _bwd(x, 2, entry="plain")
            assert rc == 0 and np.array_equal(bits, bits_plain), "lr_attention_varlen_bwd differs from the _ex call"
    # out / lse from the forward KERNEL instead: the reference is recomputed from the arrays read back
    for variant in kernel_forward:
        from llamarec_amd._lib import lib, stream_ptr

        out_d = torch.full((x.n, nh * hd), 0x7FC0, dtype=torch.int16, device="cuda")
        lse_d = torch.full((x.n, nh), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib().lr_attention_varlen_lse(x.qkv.data_ptr(), out_d.data_ptr(), lse_d.data_ptr(), x.cud.data_ptr(),
                                           x.cu.ctypes.data, x.B, nh, nkv, hd, variant, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        out, lse = _host(out_d), lse_d.cpu().numpy()
        assert np.isfinite(out).all() and np.isfinite(lse).all()
        xk = _Inputs(d["qkv"], d["d_out"], out, lse, d["cu"], nh, nkv, hd)
        rc, got, _ = _bwd(xk, variant)
        assert rc == 0, rc
        ref, bound = R.attention_bwd_ref64(d["qkv"], d["d_out"], out, lse, d["cu"], nh, nkv, hd)
        tag = f"{base} v{variant} forward=kernel"
        _report(tag, got, ref, bound, nh, nkv, hd, bad)
        _check_zero_rows(tag, got, d["cu"], bad)
    _mutant_check(d, nh, nkv, hd)
    assert not bad, bad


@pytest.mark.parametrize("regime,nh,nkv", [(r, nh, nkv) for nh, nkv in ((4, 2), (8, 1)) for r in REGIMES]
                         + [("flat", 4, 4), ("flat", 8, 2)])
def test_attention_bwd_hd128_within_bound(regime, nh, nkv):
    _check_bwd(regime, EDGE_BWD, nh, nkv, 128, RUNS, kernel_forward=(2, 1))


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_attention_bwd_hd128_workload_length_within_bound(regime):
    _check_bwd(regime, [1125], 2, 1, 128, [(2, 0, False), (2, 0, True), (1, 0, False)])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv,hd", [(4, 2, 16), (2, 2, 64), (2, 1, 256)])
def test_attention_bwd_generic_within_bound(regime, nh, nkv, hd):
    """hd 16 leaves lanes idle, hd 256 uses all four dims per lane."""
    _check_bwd(regime, GENERIC_LENS, nh, nkv, hd, [(v, det, rope) for v, det in RUNS_GENERIC for rope in (False, True)],
               kernel_forward=(1,))


@pytest.mark.parametrize("variant,det,with_rope", [(2, 0, False), (2, 0, True), (1, 1, False), (1, 1, True)])
def test_attention_bwd_every_element_has_one_owner(variant, det, with_rope):
    """The MFMA passes and the deterministic generic path have no atomics: the same bits twice, and the 193-row prompt's
    gradient rows are the same bits whether it runs alone or inside the batch."""
    nh, nkv, hd = 4, 2, 128
    d = _dataset("flat", tuple(EDGE_BWD), nh, nkv, hd)
    x = d["x"]
    rope = d["rope_dev"] if with_rope else None
    rc, _, first = _bwd(x, variant, rope, det)
    rc2, _, second = _bwd(x, variant, rope, det)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(first, second), "two runs differ"
    b = EDGE_BWD.index(193)
    s0, e0 = int(d["cu"][b]), int(d["cu"][b + 1])
    alone = _Inputs(d["qkv"][s0:e0], d["d_out"][s0:e0], d["out"][s0:e0], d["lse"][s0:e0], np.array([0, 193]), nh, nkv, hd)
    rc, _, bits = _bwd(alone, variant, rope, det)
    assert rc == 0
    assert np.array_equal(bits, first[s0:e0]), "a prompt's gradient depends on the batch around it"


def test_attention_bwd_refusals_leave_dqkv_untouched():
    from llamarec_amd._lib import lib

    d = _dataset("flat", (65, 130), 2, 2, 128)
    x = d["x"]
    cs, T = d["rope_dev"]
    d64 = _dataset("flat", (65, 130), 2, 2, 64)
    cases = {
        "variant 4": (lambda: _bwd(x, 4), LR_EINVAL, b"variant"),
        "variant 2 at head_dim 64": (lambda: _bwd(d64["x"], 2), LR_EUNSUPPORTED, b"head_dim 128"),
        "rope_cs without tok_pos (MFMA)": (lambda: _bwd(x, 2, (cs, T), tok_pos=False), LR_EINVAL, b"token positions"),
        "rope_cs without tok_pos (generic)": (lambda: _bwd(x, 1, (cs, T), tok_pos=False), LR_EINVAL, b"token positions"),
        "rope_cs without tok_pos (generic, deterministic)": (lambda: _bwd(x, 1, (cs, T), det=1, tok_pos=False), LR_EINVAL,
                                                              b"token positions"),
        "segment longer than rope_positions": (lambda: _bwd(x, 2, (cs, T - 1)), LR_EINVAL, b"positions"),
        "scratch one byte short": (lambda: _bwd(x, 2, short=1), LR_EWORKSPACE, b"scratch"),
    }
    for name, (call, code, word) in cases.items():
        rc, _, bits = call()
        assert rc == code, (name, rc)
        assert word in lib().lr_last_error(), (name, lib().lr_last_error())
        assert (bits == 0x7FC0).all(), name
    rc, got, _ = _bwd(x, 2, (cs, T))                      # a segment of exactly rope_positions rows is served
    assert rc == 0 and np.isfinite(got).all()
