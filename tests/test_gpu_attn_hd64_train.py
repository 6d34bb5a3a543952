"""GPU: attention variant 6, the head_dim-64 MFMA pair for training -- variant 5's forward writing lse (llama_attn_hd64.hip)
and the head_dim-64 backward passes (llama_attn_bwd_hd64.hip) -- against the float64 references of tests/stage2_ref.py, element
by element within the bounds derived there, through the procedure of tests/test_gpu_stage2_bwd_bounds.py (NaN-poisoned
outputs, guard rows, a 0xFF scratch of exactly the advertised size, mutants of the reference that must exceed the bound); then
the LoRA step on a head_dim-64 base against the float64 training oracle, and on the Llama-3 scaled golden."""
import functools

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_round, hash_uniform
from tests import stage2_ref as R
from tests.test_gpu_stage2_bwd_bounds import (EDGE_BWD, GUARD_BITS, GUARD_ROWS, LR_EINVAL, LR_EUNSUPPORTED, LR_EWORKSPACE,
                                              REGIMES, _Inputs, _bwd, _check_bwd, _dataset, _dev_bf16, _host)

pytestmark = pytest.mark.gpu

HEADS = [(4, 2), (8, 1), (2, 2)]
RUNS_6 = [(6, det, rope) for det in (0, 1) for rope in (False, True)]


@functools.lru_cache(maxsize=None)
def _fwd_ref(regime, nh, nkv):
    cu = np.concatenate([[0], np.cumsum(EDGE_BWD)]).astype(np.int64)
    qkv = R.attention_data(regime, cu, nh, nkv, 64)
    return (cu, qkv) + tuple(R.attention_ref64(qkv, cu, nh, nkv, 64))


def _forward(qkv, cu, nh, nkv, hd, variant, with_lse):
    """(rc, out float32, lse or None): out NaN-poisoned, lse NaN-poisoned, GUARD_ROWS guard rows behind both."""
    from llamarec_amd._lib import lib, stream_ptr

    n, B = int(cu[-1]), len(cu) - 1
    cu32 = np.ascontiguousarray(cu, dtype=np.int32)
    cud = torch.from_numpy(cu32).cuda()
    q = _dev_bf16(qkv)
    out = torch.full((n + GUARD_ROWS, nh * hd), 0x7FC0, dtype=torch.int16, device="cuda")
    out[n:] = GUARD_BITS
    lse = torch.full((n + GUARD_ROWS, nh), float("nan"), dtype=torch.float32, device="cuda")
    lse[n:] = 12345.0
    if with_lse:
        rc = lib().lr_attention_varlen_lse(q.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu32.ctypes.data, B, nh,
                                           nkv, hd, variant, stream_ptr())
    else:
        rc = lib().lr_attention_varlen(q.data_ptr(), out.data_ptr(), cud.data_ptr(), cu32.ctypes.data, B, nh, nkv, hd, variant,
                                       stream_ptr())
    torch.cuda.synchronize()
    assert bool((out[n:] == GUARD_BITS).all()), "rows behind out were written"
    assert bool((lse[n:] == 12345.0).all()), "lse rows behind the last token were written"
    if not with_lse:
        assert bool(torch.isnan(lse[:n]).all())
    return rc, out[:n].cpu().numpy().view(np.uint16), (lse[:n].cpu().numpy() if with_lse else None)


# ---- 1. forward + lse -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "peaked"])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_hd64_forward_with_lse_within_bound(regime, nh, nkv):
    from llamarec_amd.synth import bf16_bits_to_f32

    cu, qkv, ref, lse_ref, bound, lse_bound = _fwd_ref(regime, nh, nkv)
    rc5, bits5, _ = _forward(qkv, cu, nh, nkv, 64, 5, False)
    rc6, bits6, lse = _forward(qkv, cu, nh, nkv, 64, 6, True)
    rc6n, bits6n, _ = _forward(qkv, cu, nh, nkv, 64, 6, False)
    assert rc5 == 0 and rc6 == 0 and rc6n == 0
    assert np.array_equal(bits6, bits5), "variant 6 (lse) out differs from variant 5's bits"
    assert np.array_equal(bits6n, bits5), "variant 6 (no lse) out differs from variant 5's bits"
    r_out = R.ratio(bf16_bits_to_f32(bits6), ref, bound)
    r_lse = R.ratio(lse, lse_ref, lse_bound)
    print(f"hd64 fwd+lse {regime} ({nh}, {nkv}): err/bound out {r_out:.3f} lse {r_lse:.3f}")
    assert r_out <= 1.0 and r_lse <= 1.0, (r_out, r_lse)


# ---- 2. backward within the float64 bound -----------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_hd64_backward_within_bound(regime, nh, nkv):
    """Every run: with / without the rotary table, deterministic on / off, out / lse from the float64 forward; then out / lse
    from the variant-6 forward kernel; then the reference mutants on the same data set."""
    _check_bwd(regime, EDGE_BWD, nh, nkv, 64, RUNS_6, kernel_forward=(6,))


# ---- 3. one owner -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rope", [False, True])
def test_hd64_backward_every_element_has_one_owner(with_rope):
    nh, nkv, hd = 4, 2, 64
    d = _dataset("flat", tuple(EDGE_BWD), nh, nkv, hd)
    x = d["x"]
    rope = d["rope_dev"] if with_rope else None
    rc, _, first = _bwd(x, 6, rope, 0)
    rc2, _, second = _bwd(x, 6, rope, 0)
    rc3, _, det = _bwd(x, 6, rope, 1)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert np.array_equal(first, second), "two runs differ"
    assert np.array_equal(first, det), "the deterministic flag changes bits at variant 6"
    b = EDGE_BWD.index(193)
    s0, e0 = int(d["cu"][b]), int(d["cu"][b + 1])
    alone = _Inputs(d["qkv"][s0:e0], d["d_out"][s0:e0], d["out"][s0:e0], d["lse"][s0:e0], np.array([0, 193]), nh, nkv, hd)
    rc, _, bits = _bwd(alone, 6, rope, 0)
    assert rc == 0
    assert np.array_equal(bits, first[s0:e0]), "a prompt's gradient depends on the batch around it"


# ---- 4. workload length -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_hd64_backward_workload_length_within_bound(regime):
    _check_bwd(regime, [1125], 2, 1, 64, [(6, 0, False), (6, 0, True)], kernel_forward=(6,))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_hd64_train_refusals_leave_outputs_untouched():
    from llamarec_amd._lib import lib

    d128 = _dataset("flat", (65, 130), 2, 2, 128)
    d64 = _dataset("flat", (65, 130), 2, 2, 64)
    x = d64["x"]
    cs, T = d64["rope_dev"]
    zero_seg = _Inputs(d64["qkv"], d64["d_out"], d64["out"], d64["lse"], np.array([0, 65, 65, 195]), 2, 2, 64)
    cases = {
        "backward variant 6 at head_dim 128": (lambda: _bwd(d128["x"], 6), LR_EUNSUPPORTED, b"head_dim 64"),
        "scratch one byte short": (lambda: _bwd(x, 6, short=1), LR_EWORKSPACE, b"scratch"),
        "rope_cs without tok_pos": (lambda: _bwd(x, 6, (cs, T), tok_pos=False), LR_EINVAL, b"token positions"),
        "zero-length segment": (lambda: _bwd(zero_seg, 6), LR_EINVAL, b"segment"),
        "backward variant 4": (lambda: _bwd(x, 4), LR_EINVAL, b"variant"),
        "backward variant 5": (lambda: _bwd(x, 5), LR_EINVAL, b"variant"),
    }
    for name, (call, code, word) in cases.items():
        rc, _, bits = call()
        assert rc == code, (name, rc)
        assert word in lib().lr_last_error(), (name, lib().lr_last_error())
        assert (bits == 0x7FC0).all(), name
    # forward: variant 6 off head_dim 64, with and without lse; a zero-length segment
    for with_lse in (False, True):
        rc, bits, lse = _forward(d128["qkv"], d128["cu"], 2, 2, 128, 6, with_lse)
        assert rc == LR_EUNSUPPORTED and b"head_dim 64" in lib().lr_last_error(), (with_lse, rc)
        assert (bits == 0x7FC0).all() and (lse is None or np.isnan(lse).all())
    rc, bits, lse = _forward(d64["qkv"], np.array([0, 65, 65, 195]), 2, 2, 64, 6, True)
    assert rc == LR_EINVAL and (bits == 0x7FC0).all() and np.isnan(lse).all()
    rc, got, _ = _bwd(x, 6, (cs, T))                      # a segment of exactly rope_positions rows is served
    assert rc == 0 and np.isfinite(got).all()


# ---- 6. the LoRA step at head_dim 64 against the float64 oracle ---------------------------------------------------------
HD64_CFG = dict(vocab_size=320, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0)
LORA_R, LORA_LENS = 8, [129, 260, 33]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _lora_case(cfg, r=LORA_R, lens=LORA_LENS):
    from llamarec_amd.synth import synth_llama_state

    sd = synth_llama_state(cfg, 5)
    rng = np.random.default_rng(r)
    seqs = [np.concatenate([[1], rng.integers(3, cfg["vocab_size"], size=n - 2), [2]]).astype(np.int32) for n in lens]
    labels = [np.where(np.arange(len(s)) >= len(s) - 2, s, -100) for s in seqs]
    return sd, seqs, labels


def _lora_engine(sd, cfg, attention, r=LORA_R, deterministic=False):
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import LoraTrainEngine

    eng = LoraTrainEngine(LlamaRanker.from_state_dict(sd, cfg).set_variants(0, attention), r=r, alpha=2 * r, dropout=0.0)
    init = {k: bf16_round(hash_uniform(900 + i, tuple(v.shape), 0.05)) for i, (k, v) in enumerate(sorted(eng.named().items()))}
    eng.load(init)
    if deterministic:
        eng.set_deterministic(True)
    return eng, init


@functools.lru_cache(maxsize=None)
def _oracle_hd64():
    from oracle import llama_train_oracle as LO

    sd, seqs, labels = _lora_case(HD64_CFG)
    eng, init = _lora_engine(sd, HD64_CFG, 1)
    return LO.loss_and_grads(sd, HD64_CFG, init, [s.tolist() for s in seqs], [l.tolist() for l in labels], LORA_R, 2 * LORA_R)


def _lora_errors(attention):
    sd, seqs, labels = _lora_case(HD64_CFG)
    eng, init = _lora_engine(sd, HD64_CFG, attention)
    loss = float(eng.loss_and_grads(seqs, labels))
    ol, og = _oracle_hd64()
    assert abs(loss - ol) < 1e-2, (attention, loss, ol)
    got = eng.named(eng.grads)
    for n in sorted(init):
        assert _rel(got[n].cpu().numpy(), og[n]) < 4e-2, (attention, n, _rel(got[n].cpu().numpy(), og[n]))
    allg = np.concatenate([got[n].cpu().numpy().ravel() for n in sorted(init)])
    allr = np.concatenate([og[n].ravel() for n in sorted(init)])
    overall = _rel(allg, allr)
    print(f"LoRA step head_dim 64, attention {attention}: loss {loss:.5f} (oracle {ol:.5f}), overall rel L2 {overall:.5f}")
    assert overall < 2e-2, (attention, overall)
    return overall


def test_hd64_lora_step_matches_float64_oracle():
    e6 = _lora_errors(6)
    e1 = _lora_errors(1)
    # both run the same bf16 rounding points apart from P and dS
    assert e6 <= 1.5 * e1 + 2e-3, (e6, e1)


def _det_grads(cfg, attention):
    sd, seqs, labels = _lora_case(cfg)
    eng, _ = _lora_engine(sd, cfg, attention, deterministic=True)
    loss = float(eng.loss_and_grads(seqs, labels))
    assert np.isfinite(loss) and torch.isfinite(eng.grads).all() and float(eng.grads.abs().max()) > 0
    return loss, eng.grads.cpu().numpy().copy()


def test_hd64_lora_auto_is_variant_6_and_other_head_dims_keep_their_kernels():
    """Deterministic mode, so that bits can be compared at all (the generic backward adds with atomics otherwise). Two engines
    on variant 6 give identical gradients; auto at head_dim 64 is variant 6; auto at head_dim 128 / 32 is still 2 / 1."""
    l6, g6 = _det_grads(HD64_CFG, 6)
    l6b, g6b = _det_grads(HD64_CFG, 6)
    assert l6 == l6b and np.array_equal(g6, g6b), "two deterministic engines on variant 6 differ"
    l0, g0 = _det_grads(HD64_CFG, 0)
    assert l0 == l6 and np.array_equal(g0, g6), "the LoRA step's auto at head_dim 64 is not variant 6"
    l1, g1 = _det_grads(HD64_CFG, 1)
    assert not np.array_equal(g1, g6)                     # (the generic pair is a different computation)
    assert _rel(g1, g6) < 2e-2
    for heads, kv, explicit in ((2, 2, 2), (8, 4, 1)):    # head_dim 128 and 32
        cfg = dict(HD64_CFG, num_attention_heads=heads, num_key_value_heads=kv)
        la, ga = _det_grads(cfg, 0)
        le, ge = _det_grads(cfg, explicit)
        assert la == le and np.array_equal(ga, ge), (heads, kv, explicit)


def test_hd64_lora_engine_refuses_a_base_on_variant_5():
    from llamarec_amd._lib import LlamaRecError

    sd, seqs, labels = _lora_case(HD64_CFG, lens=[33])
    eng, _ = _lora_engine(sd, HD64_CFG, 5)
    with pytest.raises(LlamaRecError, match="lse"):
        eng.loss_and_grads(seqs, labels)


# ---- 7. Llama-3 scaled base ---------------------------------------------------------------------------------------------
def test_hd64_lora_on_the_llama3_scaled_golden(golden_dir):
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import IGNORE, LoraTrainEngine
    from tests.test_llama3_host import load_llama3_golden

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, "tiny_hd64_gqa")
    gap = float(z["bf16_gap"])
    label_ids = list(z["label_ids"])
    eng = LoraTrainEngine(LlamaRanker.from_state_dict(sd, cfg).set_variants(0, 6), dropout=0.0, seed=3)
    got = eng.scores(seqs, label_ids).cpu().numpy()
    print(f"variant-6 lora scores vs golden bf16 {np.abs(got - z['scores_bf16']).max():.4f}, fp32 {np.abs(got - z['scores_fp32']).max():.4f}")
    assert np.abs(got - z["scores_bf16"]).max() < 4 * gap and np.abs(got - z["scores_fp32"]).max() < 4 * gap
    train = [s for s in seqs if len(s) >= 2]
    labels = [np.concatenate([np.full(len(s) - 1, IGNORE), [label_ids[i % 20]]]) for i, s in enumerate(train)]
    loss = float(eng.loss_and_grads(train, labels))
    assert eng.bad_targets == 0 and np.isfinite(loss) and 0.0 < loss < 20.0
    assert torch.isfinite(eng.grads).all() and float(eng.grads.abs().max()) > 0
    norm = float(eng.apply(1e-3, 1.0))
    assert np.isfinite(norm) and norm > 0 and torch.isfinite(eng.params).all()
    assert np.isfinite(eng.scores(seqs, label_ids).cpu().numpy()).all()
