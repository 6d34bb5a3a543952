"""CPU: the float64 stage-2 references of tests/stage2_ref.py, pinned before any GPU result depends on them. The attention
bound must hold for a numpy emulation of the kernels' arithmetic and must be beaten at least 4x by every mutant; the
epilogue and RoPE references must reject their mutants; the HF RoPE table must be the oracle's, bit for bit."""
import numpy as np
import pytest

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
