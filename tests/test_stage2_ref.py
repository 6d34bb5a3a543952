"""CPU: the float64 stage-2 references of tests/stage2_ref.py, pinned before any GPU result depends on them. The attention
bounds (forward and backward) must hold for a numpy emulation of the kernels' arithmetic and must be beaten at least 4x by
every mutant; the backward reference must be torch.autograd's gradient in float64 and its rotation the adjoint of the
forward's; the epilogue and RoPE references must reject their mutants; the HF RoPE table must be the oracle's, bit for bit."""
import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_round, hash_uniform
from oracle import llama_oracle as LO
from tests import stage2_ref as R

LENS = [1, 63, 64, 65, 128, 129, 256, 257, 300, 600, 1125]
CU = np.concatenate([[0], np.cumsum(LENS)])
REGIMES = ("flat", "peaked", "large_v", "last_block")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv,hd", [(4, 2, 128), (2, 1, 256), (2, 2, 64)])
def test_attention_bound_holds_for_the_emulation_and_mutants_exceed_it(regime, nh, nkv, hd):
    qkv = R.attention_data(regime, CU, nh, nkv, hd)
    out, lse, bound, lse_bound = R.attention_ref64(qkv, CU, nh, nkv, hd)
    for l_bf16 in (False, True):                       # variants 1 / 3 and 2 / 4 sum l differently
        emu, emu_lse = R.attention_emul32(qkv, CU, nh, nkv, hd, l_bf16)
        r, rl = R.ratio(emu, out, bound), R.ratio(emu_lse, lse, lse_bound)
        print(f"{regime} nh={nh} nkv={nkv} hd={hd} l_bf16={l_bf16}: err/bound {r:.3f}, lse {rl:.3f}")
        assert r <= 1.0 and rl <= 1.0, (r, rl)
    for m in R.ATTN_MUTANTS:
        if m == "gqa_mod" and nkv in (1, nh):          # h % nkv == h // (nh / nkv) there: not a distinct bug
            continue
        mo, _, _, _ = R.attention_ref64(qkv, CU, nh, nkv, hd, m)
        r = R.ratio(mo, out, bound)
        print(f"  mutant {m}: {r:.1f} x bound")
        assert r >= 4.0, (m, r)


def test_attention_bound_at_long_prompts():
    cu = np.array([0, 4096, 4096 + 2049])
    qkv = R.attention_data("flat", cu, 1, 1, 128)
    out, lse, bound, lse_bound = R.attention_ref64(qkv, cu, 1, 1, 128)
    emu, emu_lse = R.attention_emul32(qkv, cu, 1, 1, 128, True)
    assert R.ratio(emu, out, bound) <= 1.0 and R.ratio(emu_lse, lse, lse_bound) <= 1.0
    mo, _, _, _ = R.attention_ref64(qkv, cu, 1, 1, 128, "diag")
    assert R.ratio(mo, out, bound) >= 4.0


def test_attention_ref_matches_the_plain_formula_on_one_prompt():
    """The chunked float64 reference equals softmax(q k^T / sqrt(hd)) v written out whole, and lse = log sum exp."""
    cu = np.array([0, 700])
    qkv = R.attention_data("peaked", cu, 2, 1, 64)
    out, lse, _, _ = R.attention_ref64(qkv, cu, 2, 1, 64)
    x = qkv.astype(np.float64)
    q, k, v = x[:, :128].reshape(700, 2, 64), x[:, 128:192], x[:, 192:]
    for h in range(2):
        s = q[:, h] @ k.T / 8.0
        s = np.where(np.tril(np.ones((700, 700), bool)), s, -np.inf)
        want_lse = np.log(np.exp(s).sum(-1))
        p = np.exp(s - want_lse[:, None])
        assert np.allclose(out[:, h * 64:(h + 1) * 64], p @ v, rtol=1e-12, atol=1e-12)
        assert np.allclose(lse[:, h], want_lse, rtol=1e-12, atol=1e-12)


def test_rope_table_hf_is_the_oracles():
    for T, hd in ((4096, 128), (8192, 256)):
        c, s, _, _ = R.rope_table_hf(T, hd, 1e4)
        oc, os_ = LO.rope_tables(T, hd, 1e4, bf16_round)
        assert np.array_equal(c.view(np.uint32), oc.view(np.uint32))
        assert np.array_equal(s.view(np.uint32), os_.view(np.uint32))


@pytest.mark.parametrize("T,hd", [(4096, 128), (8192, 256)])
def test_rope_band_holds_hf_and_rejects_table_bugs(T, hd):
    c, s, inv, ang = R.rope_table_hf(T, hd, 1e4)
    clo, chi, slo, shi = R.rope_band(T, hd, 1e4)
    assert ((c >= clo) & (c <= chi) & (s >= slo) & (s <= shi)).all()
    # the band is narrow: a table one position or one frequency off leaves it almost everywhere
    c1, s1 = np.roll(c, -1, axis=0)[:-1], np.roll(c, -1, axis=1)[:, :-1]
    assert ((c1 < clo[:-1]) | (c1 > chi[:-1])).mean() > 0.5
    assert ((s1 < clo[:, :-1]) | (s1 > chi[:, :-1])).mean() > 0.5
    # angles computed in float64 from an exact inv_freq stay inside (the kernel may compute it differently)
    inv64 = 1.0 / (1e4 ** (np.arange(0, hd, 2) / hd))
    a64 = np.arange(T)[:, None] * inv64[None, :]
    c64, s64 = bf16_round(np.cos(a64).astype(np.float32)), bf16_round(np.sin(a64).astype(np.float32))
    assert ((c64 >= clo) & (c64 <= chi) & (s64 >= slo) & (s64 <= shi)).mean() > 0.999


def _packed_qkv_acc(M, n_heads, hd, seed):
    return bf16_round(hash_uniform(seed, (M, n_heads * hd), 2.0)).astype(np.float64)


@pytest.mark.parametrize("hd", [128, 256])
def test_rope_reference_rejects_its_mutants(hd):
    T = 8192
    c, s, _, _ = R.rope_table_hf(T, hd, 1e4)
    M = 257
    acc = _packed_qkv_acc(M, 6, hd, hd)
    pos = np.arange(M) * 31 % T
    want = R.epi_rope(acc, pos, c, s, hd, 4 * hd)
    assert np.array_equal(want[:, 4 * hd:], bf16_round(acc[:, 4 * hd:].astype(np.float32)))   # v columns: store
    # against HF's rotate_half on the un-interleaved heads (the oracle's _rope), fp32 arithmetic
    x = bf16_round(acc[:, :4 * hd].astype(np.float32)).reshape(M, 4, hd)
    hf = np.concatenate([x[..., 0::2], x[..., 1::2]], axis=-1)
    rot = LO._rope(hf, np.concatenate([c, c], 1)[pos][:, :hd // 2], np.concatenate([s, s], 1)[pos][:, :hd // 2], bf16_round)
    back = np.empty_like(rot)
    back[..., 0::2], back[..., 1::2] = rot[..., :hd // 2], rot[..., hd // 2:]
    assert np.array_equal(want[:, :4 * hd], back.reshape(M, 4 * hd))
    for m in R.ROPE_MUTANTS:
        bad = R.epi_rope(acc, pos, c, s, hd, 4 * hd, m)
        frac = (bad != want).mean()
        print(f"rope mutant {m}: {frac:.3f} of the outputs differ")
        assert frac > 0.2, (m, frac)


@pytest.mark.parametrize("fn", [R.epi_swiglu, R.epi_geglu])
def test_gated_references_reject_swapped_gate_and_up(fn):
    M, N = 64, 512
    acc = bf16_round(hash_uniform(3, (M, N), 3.0)).astype(np.float64)
    acc[:, :8] = 0.0
    acc[0, :32] = np.linspace(-100, 100, 32)
    want = fn(acc)
    assert np.isfinite(want).all()
    rel = np.abs(fn(acc, swap=True) - want) / np.maximum(np.abs(want), 1e-3)
    assert (rel > 2.0 ** -7).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------
# attention backward
# ---------------------------------------------------------------------------------------------------------------------
BWD_LENS = [1, 63, 64, 65, 128, 129, 257, 300]
BWD_CU = np.concatenate([[0], np.cumsum(BWD_LENS)])
BWD_POS = np.concatenate([np.arange(T) for T in BWD_LENS])


def _f64_forward_rounded(qkv, cu, nh, nkv, hd):
    out, lse, _, _ = R.attention_ref64(qkv, cu, nh, nkv, hd)
    return bf16_round(out.astype(np.float32)), lse.astype(np.float32)


def test_attention_bwd_ref_is_autograd_in_float64():
    """Fed the exact float64 out and lse, the reference is the gradient torch.autograd takes of the whole-matrix formula
    softmax(mask(q k^T / sqrt(hd))) v (grouped-query: k / v repeated over the group), ragged batch, nh / nkv = 4.
    Tolerance: float64 sums of at most 130 x 4 terms of magnitude <= the tensor's maximum, each carrying a few 2^-53 relative
    roundings, stay below 1e-12 of that maximum; 1e-10 leaves two orders for the exp and the two different summation orders."""
    nh, nkv, hd = 8, 2, 32
    lens = [1, 37, 70, 130]
    cu = np.concatenate([[0], np.cumsum(lens)])
    n = int(cu[-1])
    qkv = R.attention_data("peaked", cu, nh, nkv, hd).astype(np.float64)
    d_out = hash_uniform(11, (n, nh * hd), 1.0).astype(np.float64)
    out, lse, _, _ = R.attention_ref64(qkv, cu, nh, nkv, hd)
    got, _ = R.attention_bwd_ref64(qkv, d_out, out, lse, cu, nh, nkv, hd)
    x = torch.from_numpy(qkv)
    q = x[:, :nh * hd].reshape(n, nh, hd).clone().requires_grad_(True)
    k = x[:, nh * hd:(nh + nkv) * hd].reshape(n, nkv, hd).clone().requires_grad_(True)
    v = x[:, (nh + nkv) * hd:].reshape(n, nkv, hd).clone().requires_grad_(True)
    outs, s0 = [], 0
    for T in lens:
        ks, vs = k[s0:s0 + T].repeat_interleave(nh // nkv, 1), v[s0:s0 + T].repeat_interleave(nh // nkv, 1)
        s = torch.einsum("qhd,khd->hqk", q[s0:s0 + T], ks) / np.sqrt(hd)
        s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool))[None], float("-inf"))
        outs.append(torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), vs))
        s0 += T
    o = torch.cat(outs)
    assert np.allclose(o.detach().numpy().reshape(n, -1), out, rtol=0, atol=1e-12 * np.abs(out).max())
    o.backward(torch.from_numpy(d_out).reshape(n, nh, hd))
    want = torch.cat([q.grad.reshape(n, -1), k.grad.reshape(n, -1), v.grad.reshape(n, -1)], 1).numpy()
    for name, a, b in (("dq", 0, nh * hd), ("dk", nh * hd, (nh + nkv) * hd), ("dv", (nh + nkv) * hd, (nh + 2 * nkv) * hd)):
        err, scale = np.abs(got[:, a:b] - want[:, a:b]).max(), np.abs(want[:, a:b]).max()
        print(f"{name}: max |ref - autograd| = {err:.3g} at scale {scale:.3g}")
        assert scale > 0 and err <= 1e-10 * scale, (name, err, scale)


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_transpose_is_the_adjoint_of_the_epilogue_rotation(hd):
    """rope_rotate64 is epi_rope's rotation without its rounding, and its transpose (what attention_bwd_ref64 applies) is
    that rotation's adjoint: <R x, y> = <x, R^T y>."""
    T, M, heads = 512, 97, 3
    c, s, _, _ = R.rope_table_hf(T, hd, 1e4)
    pos = np.arange(M) * 37 % T
    x = bf16_round(hash_uniform(5, (M, heads * hd), 1.0))
    y = hash_uniform(6, (M, heads, hd), 1.0).astype(np.float64)
    Rx = R.rope_rotate64(x.reshape(M, heads, hd), pos, c, s)
    rounded = R.epi_rope(x.astype(np.float64), pos, c, s, hd, heads * hd).reshape(M, heads, hd)
    assert np.abs(Rx - rounded).max() <= 2.0 ** -8 * np.abs(Rx).max() and (bf16_round(Rx.astype(np.float32)) == rounded).mean() > 0.99
    Rty = R.rope_rotate64(y, pos, c, s, transpose=True)
    lhs, rhs = (Rx * y).sum(), (x.reshape(M, heads, hd).astype(np.float64) * Rty).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(Rx * y).sum()), (lhs, rhs)
    assert abs((R.rope_rotate64(y, pos, c, s) * x.reshape(M, heads, hd)).sum() - lhs) > 1e-3 * abs(lhs)   # R is not its own adjoint


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv,hd", [(4, 2, 128), (8, 1, 128), (2, 2, 64), (2, 1, 256)])
def test_attention_bwd_bound_holds_for_the_emulation_and_mutants_exceed_it(regime, nh, nkv, hd):
    """Both forward sources (the float64 forward rounded to bf16 / fp32, and attention_emul32's own outputs), with and without
    the rotation: the emulation of the MFMA passes (bf16 P / dS) and of the generic path (fp32 P / dS, bf16 before the rotation)
    stays inside the bound for dq, dk and dv separately; every applicable mutant leaves it by 4x or more."""
    qkv = R.attention_data(regime, BWD_CU, nh, nkv, hd)
    d_out = R.attention_bwd_data(BWD_CU, nh, hd)
    z = R.zero_dout_rows(BWD_CU)
    assert z is not None and not d_out[z].any() and d_out[:z.start].any()
    cos, sin, _, _ = R.rope_table_hf(max(BWD_LENS), hd, 1e4)
    sources = {"exact": _f64_forward_rounded(qkv, BWD_CU, nh, nkv, hd), "emul32": R.attention_emul32(qkv, BWD_CU, nh, nkv, hd, True)}
    bad = []
    for src, (out, lse) in sources.items():
        for rope in (None, (BWD_POS, cos, sin)):
            tag = f"{regime} nh={nh} nkv={nkv} hd={hd} forward={src} rope={rope is not None}"
            ref, bound = R.attention_bwd_ref64(qkv, d_out, out, lse, BWD_CU, nh, nkv, hd, rope=rope)
            assert (bound > 0).all() and np.isfinite(bound).all()
            for bf16_ops, pre_round in ((True, False), (False, True)):
                emu = R.attention_bwd_emul32(qkv, d_out, out, lse, BWD_CU, nh, nkv, hd, bf16_ops, rope, pre_round)
                r = R.bwd_ratios(emu, ref, bound, nh, nkv, hd)
                print(f"{tag} bf16_operands={bf16_ops}: err/bound dq {r['dq']:.3f} dk {r['dk']:.3f} dv {r['dv']:.3f}")
                if not max(r.values()) <= 1.0:
                    bad.append((tag, bf16_ops, r))
                assert not emu[z].any()                # the zero-d_out rows: dq, and dk / dv as keys, exactly zero
            for m in R.BWD_MUTANTS:
                if not R.bwd_mutant_applies(m, nh, nkv, rope):
                    continue
                mo, _ = R.attention_bwd_ref64(qkv, d_out, out, lse, BWD_CU, nh, nkv, hd, m, rope)
                r = R.bwd_ratios(mo, ref, bound, nh, nkv, hd)
                print(f"  mutant {m}: dq {r['dq']:.1f} dk {r['dk']:.1f} dv {r['dv']:.1f} x bound")
                if not max(r.values()) >= 4.0:
                    bad.append((tag, m, r))
    assert not bad, bad
