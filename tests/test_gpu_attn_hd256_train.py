"""GPU: attention variant 9, the head_dim-256 MFMA pair for training -- variant 4's forward writing lse
(llama_attn_hd256_lse.hip) and the head_dim-256 backward passes (llama_attn_bwd_hd256.hip) -- against the float64 references of
tests/stage2_ref.py, element by element within the bounds derived there, through the procedure of
tests/test_gpu_stage2_bwd_bounds.py (NaN-poisoned outputs, guard rows, a 0xFF scratch of exactly the advertised size, mutants of
the reference that must exceed the bound); the refusals; the shared-prefix and last-row entry points under variant 9; then the
LoRA step on a head_dim-256 base against the float64 training oracle. The counterpart of tests/test_gpu_attn_hd96_train.py;
(8, 1) is Gemma-2B's grouping, where the dK/dV pass walks eight query heads per KV head."""
import functools

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32
from tests import stage2_ref as R
from tests.test_gpu_attn_hd64_train import _forward, _lora_case, _lora_engine, _rel
from tests.test_gpu_stage2_bwd_bounds import (EDGE_BWD, LR_EINVAL, LR_EUNSUPPORTED, LR_EWORKSPACE, REGIMES, _Inputs, _bwd,
                                              _check_bwd, _dataset)

pytestmark = pytest.mark.gpu

HD = 256
HEADS = [(4, 2), (8, 1), (2, 2)]
RUNS_9 = [(9, det, rope) for det in (0, 1) for rope in (False, True)]


@functools.lru_cache(maxsize=None)
def _fwd_ref(regime, nh, nkv):
    cu = np.concatenate([[0], np.cumsum(EDGE_BWD)]).astype(np.int64)
    qkv = R.attention_data(regime, cu, nh, nkv, HD)
    return (cu, qkv) + tuple(R.attention_ref64(qkv, cu, nh, nkv, HD))


# ---- 1. forward + lse -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "peaked"])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_hd256_forward_with_lse_within_bound(regime, nh, nkv):
    cu, qkv, ref, lse_ref, bound, lse_bound = _fwd_ref(regime, nh, nkv)
    rc9, bits9, lse = _forward(qkv, cu, nh, nkv, HD, 9, True)
    rc9n, bits9n, _ = _forward(qkv, cu, nh, nkv, HD, 9, False)
    rc4, bits4, _ = _forward(qkv, cu, nh, nkv, HD, 4, False)
    assert rc4 == 0 and rc9 == 0 and rc9n == 0
    assert np.array_equal(bits9, bits4), "variant 9 (lse) out differs from variant 4's bits"
    assert np.array_equal(bits9n, bits4), "variant 9 (no lse) out differs from variant 4's bits"
    r_out = R.ratio(bf16_bits_to_f32(bits9), ref, bound)
    r_lse = R.ratio(lse, lse_ref, lse_bound)
    print(f"hd256 fwd+lse {regime} ({nh}, {nkv}): err/bound out {r_out:.3f} lse {r_lse:.3f}")
    assert r_out <= 1.0 and r_lse <= 1.0, (r_out, r_lse)


# ---- 2. backward within the float64 bound -----------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_hd256_backward_within_bound(regime, nh, nkv):
    """Every run: with / without the rotary table, deterministic on / off, out / lse from the float64 forward; then out / lse
    from the variant-9 forward kernel; then the reference mutants on the same data set."""
    _check_bwd(regime, EDGE_BWD, nh, nkv, HD, RUNS_9, kernel_forward=(9,))


# ---- 3. one owner -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rope", [False, True])
def test_hd256_backward_every_element_has_one_owner(with_rope):
    nh, nkv = 4, 2
    d = _dataset("flat", tuple(EDGE_BWD), nh, nkv, HD)
    x = d["x"]
    rope = d["rope_dev"] if with_rope else None
    rc, _, first = _bwd(x, 9, rope, 0)
    rc2, _, second = _bwd(x, 9, rope, 0)
    rc3, _, det = _bwd(x, 9, rope, 1)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert np.array_equal(first, second), "two runs differ"
    assert np.array_equal(first, det), "the deterministic flag changes bits at variant 9"
    b = EDGE_BWD.index(193)
    s0, e0 = int(d["cu"][b]), int(d["cu"][b + 1])
    alone = _Inputs(d["qkv"][s0:e0], d["d_out"][s0:e0], d["out"][s0:e0], d["lse"][s0:e0], np.array([0, 193]), nh, nkv, HD)
    rc, _, bits = _bwd(alone, 9, rope, 0)
    assert rc == 0
    assert np.array_equal(bits, first[s0:e0]), "a prompt's gradient depends on the batch around it"


# ---- 4. workload length -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_hd256_backward_workload_length_within_bound(regime):
    _check_bwd(regime, [1125], 2, 1, HD, [(9, 0, False), (9, 0, True)], kernel_forward=(9,))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_hd256_train_refusals_leave_outputs_untouched():
    from llamarec_amd._lib import lib, stream_ptr

    d256 = _dataset("flat", (65, 130), 2, 2, HD)
    x = d256["x"]
    cs, T = d256["rope_dev"]
    zero_seg = _Inputs(d256["qkv"], d256["d_out"], d256["out"], d256["lse"], np.array([0, 65, 65, 195]), 2, 2, HD)
    cases = {
        "scratch one byte short": (lambda: _bwd(x, 9, short=1), LR_EWORKSPACE, b"scratch"),
        "rope_cs without tok_pos": (lambda: _bwd(x, 9, (cs, T), tok_pos=False), LR_EINVAL, b"token positions"),
        "zero-length segment": (lambda: _bwd(zero_seg, 9), LR_EINVAL, b"segment"),
        "backward variant 4": (lambda: _bwd(x, 4), LR_EINVAL, b"variant"),
    }
    others = {hd: _dataset("flat", (65, 130), 2, 2, hd) for hd in (64, 96, 128)}
    for hd, d in others.items():
        cases[f"backward variant 9 at head_dim {hd}"] = (lambda d=d: _bwd(d["x"], 9), LR_EUNSUPPORTED, b"head_dim 256")
    for name, (call, code, word) in cases.items():
        rc, _, bits = call()
        assert rc == code, (name, rc)
        assert word in lib().lr_last_error(), (name, lib().lr_last_error())
        assert (bits == 0x7FC0).all(), name
    # forward: variant 9 off head_dim 256, with and without lse; variant 4 with lse; a zero-length segment
    for hd, d in others.items():
        for with_lse in (False, True):
            rc, bits, lse = _forward(d["qkv"], d["cu"], 2, 2, hd, 9, with_lse)
            assert rc == LR_EUNSUPPORTED and b"head_dim 256" in lib().lr_last_error(), (hd, with_lse, rc)
            assert (bits == 0x7FC0).all() and (lse is None or np.isnan(lse).all())
    rc, bits, lse = _forward(d256["qkv"], d256["cu"], 2, 2, HD, 4, True)
    assert rc == LR_EINVAL and b"lse" in lib().lr_last_error() and (bits == 0x7FC0).all() and np.isnan(lse).all()
    rc, bits, lse = _forward(d256["qkv"], np.array([0, 65, 65, 195]), 2, 2, HD, 9, True)
    assert rc == LR_EINVAL and (bits == 0x7FC0).all() and np.isnan(lse).all()
    # variant 9 has no soft-capped form
    cu = np.ascontiguousarray(d256["cu"], dtype=np.int32)
    out = torch.full((int(cu[-1]), 2 * HD), 0x1234, dtype=torch.int16, device="cuda")
    rc = lib().lr_attention_varlen_softcap(x.qkv.data_ptr(), out.data_ptr(), x.cud.data_ptr(), cu.ctypes.data, 2, 0, 2, 2, HD,
                                           float(HD) ** -0.5, 50.0, 9, stream_ptr())
    torch.cuda.synchronize()
    assert rc == LR_EUNSUPPORTED and b"soft" in lib().lr_last_error(), (rc, lib().lr_last_error())
    assert bool((out == 0x1234).all())
    rc, got, _ = _bwd(x, 9, (cs, T))                      # a segment of exactly rope_positions rows is served
    assert rc == 0 and np.isfinite(got).all()


# ---- 6. the shared-prefix and last-row entry points under variant 9 ----------------------------------------------------
def test_hd256_prefix_forms_under_variant_9_are_variant_4s_bits():
    from tests.test_gpu_attn_prefix import GUARD, POISON, _bits, _full, _lib, _prefix_call, _prefix_layout, _whole_prompts

    L, st = _lib()
    nh, nkv, P, tails = 4, 2, 36, [70, 130]
    qkv, cu = _whole_prompts("flat", P, tails, nh, nkv, HD)
    full = _full(_bits(qkv), cu, nh, nkv, HD, 4)
    rows, seg, src = _prefix_layout(qkv, cu, P)
    n, B = int(seg[-1]), len(tails)
    got = {}
    for v in (4, 9):
        rc, out = _prefix_call(_bits(rows), seg, P, nh, nkv, HD, v)
        assert rc == 0, (v, L.lr_last_error())
        assert (out[n:].view(np.uint16) == POISON).all(), (v, "guard rows written")
        got[v] = out[:n]
    assert np.array_equal(got[9], got[4]) and np.array_equal(got[9], full[src])
    kv = np.ascontiguousarray(rows[:, nh * HD:])
    q_last = np.ascontiguousarray(qkv[cu[1:] - 1, :nh * HD])
    kv_d, q_d, segd = _bits(kv), _bits(q_last), torch.from_numpy(seg).cuda()
    last = {}
    for v in (4, 9):
        out = torch.full((B + GUARD, nh * HD), POISON, dtype=torch.int16, device="cuda")
        rc = L.lr_attention_last_rows(kv_d.data_ptr(), q_d.data_ptr(), out.data_ptr(), segd.data_ptr(), seg.ctypes.data, len(seg) - 1,
                                      P, nh, nkv, HD, v, st)
        torch.cuda.synchronize()
        assert rc == 0, (v, L.lr_last_error())
        o = out.cpu().numpy()
        assert (o[B:].view(np.uint16) == POISON).all(), (v, "rows past the prompts written")
        last[v] = o[:B]
    assert np.array_equal(last[9], last[4]) and np.array_equal(last[9], full[cu[1:] - 1])


# ---- 7. the LoRA step at head_dim 256 against the float64 oracle --------------------------------------------------------
HD256_CFG = dict(vocab_size=320, hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                 num_key_value_heads=1, max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0)
LORA_R = 8


@functools.lru_cache(maxsize=None)
def _oracle_hd256():
    from oracle import llama_train_oracle as LO

    sd, seqs, labels = _lora_case(HD256_CFG)
    eng, init = _lora_engine(sd, HD256_CFG, 1)
    return LO.loss_and_grads(sd, HD256_CFG, init, [s.tolist() for s in seqs], [l.tolist() for l in labels], LORA_R, 2 * LORA_R)


def _lora_errors(attention):
    """Prints every figure before it is asserted; returns the overall relative L2 error of the gradients."""
    sd, seqs, labels = _lora_case(HD256_CFG)
    eng, init = _lora_engine(sd, HD256_CFG, attention)
    loss = float(eng.loss_and_grads(seqs, labels))
    ol, og = _oracle_hd256()
    got = eng.named(eng.grads)
    per = {n: _rel(got[n].cpu().numpy(), og[n]) for n in sorted(init)}
    allg = np.concatenate([got[n].cpu().numpy().ravel() for n in sorted(init)])
    allr = np.concatenate([og[n].ravel() for n in sorted(init)])
    overall = _rel(allg, allr)
    print(f"LoRA step head_dim 256, attention {attention}: loss {loss:.5f} (oracle {ol:.5f}), overall rel L2 {overall:.5f}, "
          f"worst tensor {max(per.values()):.5f}")
    assert all(float(np.linalg.norm(og[n])) > 0 for n in sorted(init)), "the oracle has a zero gradient tensor"
    assert abs(loss - ol) < 1e-2, (attention, loss, ol)
    for n, e in per.items():
        assert e < 4e-2, (attention, n, e)
    assert overall < 2e-2, (attention, overall)
    return overall


def test_hd256_lora_step_matches_float64_oracle():
    """The generic pair (variant 1) first: it is the code that ran this route before variant 9 existed."""
    e1 = _lora_errors(1)
    e9 = _lora_errors(9)
    # both run the same bf16 rounding points apart from P and dS
    assert e9 <= 1.5 * e1 + 2e-3, (e9, e1)


# ---- 8. auto, in deterministic mode -------------------------------------------------------------------------------------
def _det_grads(attention):
    sd, seqs, labels = _lora_case(HD256_CFG)
    eng, _ = _lora_engine(sd, HD256_CFG, attention, deterministic=True)
    loss = float(eng.loss_and_grads(seqs, labels))
    assert np.isfinite(loss) and torch.isfinite(eng.grads).all() and float(eng.grads.abs().max()) > 0
    return loss, eng.grads.cpu().numpy().copy()


def test_hd256_lora_auto_is_variant_9():
    """Deterministic mode, so that bits can be compared at all (the generic backward adds with atomics otherwise). Two engines
    on variant 9 give identical gradients; the LoRA step's auto at head_dim 256 is variant 9; the generic pair is another
    computation close to it."""
    l9, g9 = _det_grads(9)
    l9b, g9b = _det_grads(9)
    assert l9 == l9b and np.array_equal(g9, g9b), "two deterministic engines on variant 9 differ"
    l0, g0 = _det_grads(0)
    assert l0 == l9 and np.array_equal(g0, g9), "the LoRA step's auto at head_dim 256 is not variant 9"
    l1, g1 = _det_grads(1)
    assert not np.array_equal(g1, g9)
    assert _rel(g1, g9) < 2e-2


def test_hd256_lora_engine_refuses_a_base_on_variant_4():
    from llamarec_amd._lib import LlamaRecError

    sd, seqs, labels = _lora_case(HD256_CFG, lens=[33])
    eng, _ = _lora_engine(sd, HD256_CFG, 4)
    with pytest.raises(LlamaRecError, match="lse"):
        eng.loss_and_grads(seqs, labels)
