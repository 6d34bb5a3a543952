"""GPU: the Qwen2 ranker (--llm qwen2) through the C ABI: the bias epilogue of the GEMMs (lr_gemm_bf16_nt_bias_epi) against the
float64 epilogues of tests/stage2_ref.py, GEMM variant 6 (the 256-tile body on a ragged last column tile) bit for bit against
variant 4 on zero-padded operands, the scoring path on the committed Qwen2 goldens (tests/gen_goldens_qwen2.py) in every mode,
head_dim-64 attention at Qwen2-0.5B's GQA group of 7, lr_llama_set_qkv_bias and the refusals that go with it, from_pretrained,
and the train_ranker entry point."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_round, hash_uniform
from tests import stage2_ref as R
from tests.test_gpu_attn_prefix import _prefixed_prompts
from tests.test_gpu_stage2_bounds import _attn, _bf16_ulp, _dev_bf16, _host, _K, _operands, _report, _rope_table
from tests.test_qwen2_host import QWEN2_GOLDENS, load_qwen2_golden

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
POISON = 0x7FC0   # bf16 NaN
T_ROPE = 512


def _bias_epi(A_d, B_d, M, N, K, epi, variant, bias_d=None, R_d=None, pos_d=None, cs=None, rope_positions=0, hd=0, rot_cols=0,
              ws=None, want_rc=0):
    """One lr_gemm_bf16_nt_bias_epi call on a NaN-poisoned C with one guard row behind row M. Returns C[:M] as float32 after
    checking that the guard row kept its bits (a store past column N of the last row lands there; past column N of any other
    row it lands in the next row and shows as a mismatch)."""
    from llamarec_amd._lib import lib, stream_ptr

    n_out = N // 2 if epi in (2, 5) else N
    Cd = torch.full((M + 1, n_out), POISON, dtype=torch.int16, device="cuda")
    rc = lib().lr_gemm_bf16_nt_bias_epi(A_d.data_ptr(), B_d.data_ptr(), Cd.data_ptr(), R_d.data_ptr() if R_d is not None else None,
                                        M, N, K, epi, variant, pos_d.data_ptr() if pos_d is not None else None,
                                        cs.data_ptr() if cs is not None else None, rope_positions, hd, rot_cols,
                                        ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                        bias_d.data_ptr() if bias_d is not None else None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, (epi, variant, M, N, K, rc, lib().lr_last_error())
    bits = Cd.cpu().numpy().view(np.uint16)
    assert (bits[M] == POISON).all(), ("guard row written", epi, variant, M, N)
    if want_rc != 0:
        assert (bits == POISON).all(), ("a refused call wrote its output", epi, variant)
        return None
    return _host(Cd[:M])


def _table(hd):
    cs = _rope_table(T_ROPE, hd)
    cs_h = cs[: T_ROPE * hd].view(T_ROPE, hd // 2, 2).cpu().numpy()
    return cs, cs_h[..., 0], cs_h[..., 1]


def _positions(M):
    pos = ((np.arange(M) * 2654435761) % T_ROPE).astype(np.int32)
    pos[0] = T_ROPE - 1
    return pos


def _bias(kind, N, seed):
    """exact: small integers times 2^-3 (the sum with an exact accumulator is exact in fp32); random: bf16 of width 0.5"""
    if kind == "exact":
        return (np.round(hash_uniform(seed, (N,), 2.5)) * 0.125).astype(np.float32)
    return bf16_round(hash_uniform(seed, (N,), 0.5))


# ---- the bias epilogue ----------------------------------------------------------------------------------------------------
# (name, N, rot_cols, head_dim): the qkv widths of the published Qwen2 sizes
QKV_WIDTHS = [("qwen2-0.5b", 1152, 1024, 64), ("qwen2-1.5b", 2048, 1792, 128), ("qwen2-7b", 4608, 4096, 128)]
MS = [1, 7, 255, 257, 517]


def _variants_for(N):
    return (1, 4, 5, 6) if N % 256 == 0 else (1, 6)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("name,N,rot_cols,hd", QKV_WIDTHS)
def test_bias_epilogue_store_and_rope_within_bound(kind, name, N, rot_cols, hd):
    """x = bf16(fp32 acc + fp32 bias), then the rotation: bit-equal to the float64 epilogues on acc + bias for exact operands,
    within their bounds (plus 2^-24 (|acc| + |bias|) for the fp32 add) for random ones; generic, 256-tile, split-K and ragged
    routes. At M = 517 three mutants of the reference (bias dropped, added behind the rotation, shifted one column) each
    differ from the kernel's output in more than a tenth of the rotated elements."""
    cs, cos, sin = _table(hd)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    bias = _bias(kind, N, N + 5)
    bias_d = _dev_bf16(bias)
    bad = []
    for M in MS:
        pos = _positions(M)
        pos_d = torch.from_numpy(pos).cuda()
        cache = {}
        for variant in _variants_for(N):
            K = _K(kind, variant)
            if K not in cache:
                A, B, acc = _operands(kind, M, N, K, M + N)
                absum = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T if kind == "random" else None
                cache[K] = (_dev_bf16(A), _dev_bf16(B), acc, absum)
            A_d, B_d, acc, absum = cache[K]
            x = acc + bias[None, :].astype(np.float64)
            w = ws if variant == 5 else None
            tag = f"{name} {kind} M={M} v{variant}"
            got_s = _bias_epi(A_d, B_d, M, N, K, 0, variant, bias_d, ws=w)
            want_s = R.epi_store(x)
            rope_runs = []
            for rope_positions in ((T_ROPE, 0) if hd == 128 else (T_ROPE,)):   # packed-table (LDS) path and float-table path
                rope_runs.append((rope_positions, _bias_epi(A_d, B_d, M, N, K, 3, variant, bias_d, pos_d=pos_d, cs=cs,
                                                            rope_positions=rope_positions, hd=hd, rot_cols=rot_cols, ws=w)))
            want_r = R.epi_rope(x, pos, cos, sin, hd, rot_cols)
            if kind == "exact":
                assert np.array_equal(x.astype(np.float32).astype(np.float64), x)          # acc + bias is exact in fp32
                if not np.array_equal(got_s, want_s):
                    bad.append(("store", tag, _report(f"store {tag}", got_s, want_s, None)))
                for rp, got_r in rope_runs:
                    if not np.array_equal(got_r, want_r):
                        bad.append(("rope", rp, tag, _report(f"rope({rp}) {tag}", got_r, want_r, None)))
                if M == 517 and variant in (1, 6):
                    got_r = rope_runs[0][1]
                    mutants = {"dropped": R.epi_rope(acc, pos, cos, sin, hd, rot_cols),
                               "after_rotation": bf16_round(R.epi_rope(acc, pos, cos, sin, hd, rot_cols) + bias[None, :]),
                               "shifted": R.epi_rope(acc + np.roll(bias, 1)[None, :], pos, cos, sin, hd, rot_cols)}
                    for m, mut in mutants.items():
                        frac = float((mut[:, :rot_cols] != got_r[:, :rot_cols]).mean())
                        print(f"  mutant {m} {tag}: {frac:.2f} of the rotated elements differ")
                        assert frac > 0.1, (m, tag, frac)
            else:
                acc_err = K * 2.0 ** -24 * absum + 2.0 ** -24 * (np.abs(acc) + np.abs(bias)[None, :])
                x_ulp = _bf16_ulp(x) + acc_err
                if _report(f"store {tag}", got_s, x, x_ulp) > 1:
                    bad.append(("store", tag))
                pair = 2 * np.maximum(x_ulp, np.maximum(np.roll(x_ulp, -1, axis=1), np.roll(x_ulp, 1, axis=1))) + _bf16_ulp(want_r)
                for rp, got_r in rope_runs:
                    if _report(f"rope({rp}) {tag}", got_r, want_r, pair) > 1:
                        bad.append(("rope", rp, tag))
    assert not bad, bad[:10]


def test_a_bias_with_another_epilogue_is_refused_and_writes_nothing():
    M, N, K = 130, 512, 128
    A, B, _ = _operands("exact", M, N, K, 3)
    A_d, B_d, bias_d = _dev_bf16(A), _dev_bf16(B), _dev_bf16(_bias("exact", N, 1))
    R_d = _dev_bf16(np.zeros((M, N), np.float32))
    ws = torch.empty(8 << 20, dtype=torch.uint8, device="cuda")
    for variant in (0, 1, 4, 5, 6):
        for epi in (1, 2, 5):
            _bias_epi(A_d, B_d, M, N, K, epi, variant, bias_d, R_d=R_d, ws=ws, want_rc=LR_EINVAL)
    # a misaligned bias, and without a bias the entry point is lr_gemm_bf16_nt_epi
    from llamarec_amd._lib import lib, stream_ptr

    odd = torch.zeros(N + 4, dtype=torch.int16, device="cuda")[1:]
    Cd = torch.full((M, N), POISON, dtype=torch.int16, device="cuda")
    rc = lib().lr_gemm_bf16_nt_bias_epi(A_d.data_ptr(), B_d.data_ptr(), Cd.data_ptr(), None, M, N, K, 0, 1, None, None, 0, 0, 0, None,
                                        0, odd.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    assert rc == LR_EINVAL and (Cd.cpu().numpy().view(np.uint16) == POISON).all()
    plain = _bias_epi(A_d, B_d, M, N, K, 1, 4, None, R_d=R_d)
    assert np.array_equal(plain, R.epi_residual(A.astype(np.float64) @ B.astype(np.float64).T, np.zeros((M, N), np.float32)))


# ---- variant 6: the ragged last column tile ----------------------------------------------------------------------------------
# (N, head_dim, rot_cols): one slab, one tile and a slab, Qwen2-0.5B's hidden and qkv widths (the latter at both head sizes:
# head_dim 128 with rot_cols a multiple of 256 stages its rope table through LDS)
RAGGED = [(64, 32, 32), (320, 64, 256), (896, 64, 768), (1152, 64, 1024), (1152, 128, 1024)]
RAGGED_MS = [128, 255, 257, 517]


@pytest.mark.parametrize("N,hd,rot_cols", RAGGED)
def test_ragged_tile_is_variant_4_on_padded_operands(N, hd, rot_cols):
    """Variant 6 at N % 256 != 0, exact operands: bit-equal to the float64 epilogue and to variant 4 on B (and bias, R) zero-padded
    to the next multiple of 256, cut to N columns -- the same arithmetic. Every element of C[:M, :N] is written and the guard
    row behind row M keeps its bits. K = 64 (one K tile) at M = 128, else 192 (an odd number of K tiles)."""
    cs, cos, sin = _table(hd)
    Np = (N + 255) // 256 * 256
    bias = _bias("exact", N, N + hd)
    bias_d, biasp_d = _dev_bf16(bias), _dev_bf16(np.concatenate([bias, np.zeros(Np - N, np.float32)]))
    bad = []
    for M in RAGGED_MS:
        K = 64 if M == 128 else 192
        A, B, acc = _operands("exact", M, N, K, M + N)
        Bp = np.concatenate([B, np.zeros((Np - N, K), np.float32)])
        A_d, B_d, Bp_d = _dev_bf16(A), _dev_bf16(B), _dev_bf16(Bp)
        Rr = bf16_round(hash_uniform(M * 3 + 1, (M, N), 4.0))
        R_d, Rp_d = _dev_bf16(Rr), _dev_bf16(np.concatenate([Rr, np.zeros((M, Np - N), np.float32)], axis=1))
        pos = _positions(M)
        pos_d = torch.from_numpy(pos).cuda()
        x = acc + bias[None, :].astype(np.float64)
        rope = dict(pos_d=pos_d, cs=cs, rope_positions=T_ROPE, hd=hd, rot_cols=rot_cols)
        runs = [("store", 0, None, {}, R.epi_store(acc)), ("store+bias", 0, bias_d, {}, R.epi_store(x)),
                ("residual", 1, None, dict(R_d=R_d), R.epi_residual(acc, Rr)),
                ("rope", 3, None, rope, R.epi_rope(acc, pos, cos, sin, hd, rot_cols)),
                ("rope+bias", 3, bias_d, rope, R.epi_rope(x, pos, cos, sin, hd, rot_cols))]
        for what, epi, b_d, kw, want in runs:
            tag = f"{what} N={N} hd={hd} M={M}"
            got = _bias_epi(A_d, B_d, M, N, K, epi, 6, b_d, **kw)
            assert np.isfinite(got).all(), (tag, "an element of C[:M, :N] was not written")
            if not np.array_equal(got, want):
                bad.append((tag, "float64 epilogue", _report(tag, got, want, None)))
            kwp = dict(kw, R_d=Rp_d) if epi == 1 else kw
            padded = _bias_epi(A_d, Bp_d, M, Np, K, epi, 4, biasp_d if b_d is not None else None, **kwp)
            if not np.array_equal(got, padded[:, :N]):
                bad.append((tag, "variant 4 on padded operands", float(np.abs(got - padded[:, :N]).max())))
    assert not bad, bad[:10]


def test_variant_6_routes_as_auto_everywhere_else():
    """N % 256 == 0: variant 4's bits. M < 128, and a gated epilogue at a ragged N: the generic kernel's bits. Random operands, so
    equal bits mean the same kernel's summation order. Variant 7 is still refused."""
    K, hd = 192, 64
    cs, _, _ = _table(hd)
    for M, N, epi, same_as in [(257, 1024, 0, 4), (257, 1024, 3, 4), (1, 1152, 3, 1), (127, 1152, 3, 1), (127, 896, 0, 1), (257, 320, 2, 1),
                               (257, 96, 0, 1)]:
        A, B, _ = _operands("random", M, N, K, M + N)
        A_d, B_d = _dev_bf16(A), _dev_bf16(B)
        bias_d = _dev_bf16(_bias("random", N, 2)) if epi in (0, 3) else None
        kw = dict(pos_d=torch.from_numpy(_positions(M)).cuda(), cs=cs, rope_positions=T_ROPE, hd=hd, rot_cols=N - 128) if epi == 3 else {}
        got = _bias_epi(A_d, B_d, M, N, K, epi, 6, bias_d, **kw)
        want = _bias_epi(A_d, B_d, M, N, K, epi, same_as, bias_d, **kw)
        assert np.isfinite(got).all() and np.array_equal(got, want), (M, N, epi, same_as)
    A, B, _ = _operands("random", 130, 320, K, 1)
    _bias_epi(_dev_bf16(A), _dev_bf16(B), 130, 320, K, 0, 7, None, want_rc=LR_EINVAL)
    from llamarec_amd._lib import lib

    _bias_epi(_dev_bf16(A), _dev_bf16(B), 130, 320, K, 0, 4, None, want_rc=LR_EUNSUPPORTED)   # forced 4 at a ragged width
    assert b"gemm variant 4 needs" in lib().lr_last_error()


# ---- head_dim-64 attention at Qwen2-0.5B's group of 7 -----------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_attention_hd64_at_gqa_group_7_within_bound(regime):
    nh, nkv, hd = 14, 2, 64
    lens = [1, 63, 64, 65, 129, 300]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    qkv = R.attention_data(regime, cu, nh, nkv, hd)
    ref, _, bound, _ = R.attention_ref64(qkv, cu, nh, nkv, hd)
    rc, got, _ = _attn(_dev_bf16(qkv), cu, int(cu[-1]), nh, nkv, hd, "plain", 5, False)
    assert rc == 0
    r = R.ratio(got, ref, bound)
    mut, _, _, _ = R.attention_ref64(qkv, cu, nh, nkv, hd, "gqa_mod")
    print(f"attention {regime} hd=64 nh=14 nkv=2 v5: err/bound {r:.3f}; reference mutant 'gqa_mod': {R.ratio(mut, ref, bound):.1f} x bound")
    assert R.ratio(mut, ref, bound) > 1.0
    assert r <= 1.0, r


# ---- the scoring path on the reference's goldens ----------------------------------------------------------------------------
_MODELS = {}


def _golden_model(golden_dir, name):
    """(archive, config, state, prompts, tolerance, ranker): one ranker per archive, its variants reset to the family default"""
    if name not in _MODELS:
        from llamarec_amd.llm import LlamaRanker
        from tests.gen_goldens_qwen2 import golden_tolerance

        z, cfg, sd, seqs = load_qwen2_golden(golden_dir, name)
        _MODELS[name] = (z, cfg, sd, seqs, golden_tolerance(z["logits_fp32"], z["logits_bf16"]), LlamaRanker.from_state_dict(sd, cfg))
    out = _MODELS[name]
    out[5].set_variants(out[5].default_gemm_variant, 0).set_last_layer_pruning(True)
    return out


def _fits_tile(cfg, hd):
    d, f = cfg["hidden_size"], cfg["intermediate_size"]
    qkv_w = (cfg["num_attention_heads"] + 2 * cfg["num_key_value_heads"]) * hd
    return all(n % 256 == 0 for n in (d, 2 * f, qkv_w)) and all(k % 64 == 0 for k in (d, f))


@pytest.mark.parametrize("name", QWEN2_GOLDENS)
@pytest.mark.parametrize("variants", ["default", (1, 1), (4, "mfma"), (0, 0)])
def test_qwen2_prefill_vs_reference_goldens(golden_dir, name, variants):
    """Last-token logits within the archive's own tolerance of the reference's fp32 and bf16 logits: the family default (GEMM
    variant 6), the generic kernels, auto, and GEMM variant 4 with the head size's MFMA attention forced where the shapes fit
    the tile (hd128_gqa; on hd64_ragged and hd16 forced 4 fails by name and the archive is scored with variant 6 instead)."""
    from llamarec_amd._lib import LlamaRecError

    z, cfg, sd, seqs, tol, model = _golden_model(golden_dir, name)
    assert model.family == "qwen2" and model.default_gemm_variant == 6 and "0.bqkv" in model._tensors
    if variants == "default":
        variants = None
    elif variants[1] == "mfma":
        attn = {64: 5, 128: 2}.get(model.hd, 1)
        assert _fits_tile(cfg, model.hd) == (name == "hd128_gqa")
        if not _fits_tile(cfg, model.hd):
            with pytest.raises(LlamaRecError, match="gemm variant 4"):
                model.set_variants(4, attn).last_logits(seqs)
            torch.cuda.synchronize()
            variants = (6, attn)
        else:
            variants = (4, attn)
    if variants is not None:
        model.set_variants(*variants)
    got = model.last_logits(seqs).cpu().numpy()
    assert got.shape == z["logits_bf16"].shape and np.array_equal(got, bf16_round(got))
    print(f"{name} {variants}: vs bf16 {np.abs(got - z['logits_bf16']).max():.4f}, vs fp32 {np.abs(got - z['logits_fp32']).max():.4f}, "
          f"tolerance {tol:.4f}")
    assert np.abs(got - z["logits_fp32"]).max() < tol
    assert np.abs(got - z["logits_bf16"]).max() < tol
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])


@pytest.mark.parametrize("name", QWEN2_GOLDENS)
def test_a_model_with_zeroed_biases_is_far_from_the_goldens(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs, tol, _ = _golden_model(golden_dir, name)
    zeroed = {k: (np.zeros_like(v) if k.endswith(".bias") else v) for k, v in sd.items()}
    got = LlamaRanker.from_state_dict(zeroed, cfg).last_logits(seqs).cpu().numpy()
    assert np.abs(got - z["logits_fp32"]).max() > 10 * tol


MODEL_TAILS = [1, 7, 40, 90, 130]
LABELS = list(range(40, 60))


@pytest.mark.parametrize("name", ["hd64_ragged", "hd128_gqa"])
def test_qwen2_modes_agree(golden_dir, name):
    """Scores with the shared 36-token prefix are bit-identical to the unshared call (pruned last layer on and off: the K | V
    and Q products of the pruned layer take their slices of the bias); pruning on and off, and latency mode (GEMM variant 5)
    against the default, agree within the golden tolerance, which also holds each against the reference's logits."""
    z, cfg, sd, seqs, tol, model = _golden_model(golden_dir, name)
    shared_seqs = _prefixed_prompts(36, MODEL_TAILS, cfg["vocab_size"], 36)
    assert max(len(s) for s in shared_seqs) <= cfg["max_position_embeddings"] and sum(MODEL_TAILS) + 36 >= 128
    for prune in (True, False):
        model.set_last_layer_pruning(prune)
        shared = model.prefill_verbalize(shared_seqs, LABELS, share_prefix=True)
        plain = model.prefill_verbalize(shared_seqs, LABELS, share_prefix=False)
        assert torch.isfinite(plain).all() and torch.equal(shared, plain), prune
    pruned = model.set_last_layer_pruning(True).last_logits(seqs).cpu().numpy()
    full = model.set_last_layer_pruning(False).last_logits(seqs).cpu().numpy()
    latency = model.set_last_layer_pruning(True).set_variants(5, 0).last_logits(seqs).cpu().numpy()
    print(f"{name}: pruned-full {np.abs(pruned - full).max():.4f}, latency-default {np.abs(latency - pruned).max():.4f}, tolerance {tol:.4f}")
    assert np.abs(pruned - full).max() < tol and np.abs(full - z["logits_bf16"]).max() < tol
    assert np.abs(latency - pruned).max() < tol
    assert np.abs(latency - z["logits_fp32"]).max() < tol and np.abs(latency - z["logits_bf16"]).max() < tol


# ---- lr_llama_set_qkv_bias ------------------------------------------------------------------------------------------------------
def test_set_qkv_bias_checks_its_array_and_null_restores_the_llama_scores(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd._lib import lib
    from llamarec_amd.llm import LlamaRanker

    L = lib()
    z, cfg, sd, seqs, tol, model = _golden_model(golden_dir, "hd64_ragged")
    nl = cfg["num_hidden_layers"]
    before = model.prefill_verbalize(seqs, LABELS)
    arr = (C.c_void_p * nl)(*[model._tensors[f"{i}.bqkv"].data_ptr() for i in range(nl)])
    arr[nl - 1] = None
    assert L.lr_llama_set_qkv_bias(model._h, arr) == LR_EINVAL and b"null bias" in L.lr_last_error()
    arr[nl - 1] = model._tensors[f"{nl - 1}.bqkv"].data_ptr() + 2
    assert L.lr_llama_set_qkv_bias(model._h, arr) == LR_EINVAL and b"aligned" in L.lr_last_error()
    assert torch.equal(model.prefill_verbalize(seqs, LABELS), before)                  # the handle kept its biases
    # folded norms and a LoRA engine are refused on a handle with a bias
    w = model._tensors["0.wqkv"]
    fold = (C.c_void_p * nl)(*([w.data_ptr()] * nl))
    assert L.lr_llama_set_folded_norms(model._h, fold, fold) == LR_EUNSUPPORTED and b"bias" in L.lr_last_error()
    assert L.lr_llama_set_folded_norms(model._h, None, None) == 0
    lc = A.LrLoraTrainConfig(r=8, alpha=32.0, dropout=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, seed=1)
    layers = (A.LrLlamaLayerWeightsT * nl)()
    wt = A.LrLlamaWeightsTDesc(layers=layers, lm_head_t=None)
    h = C.c_void_p()
    assert L.lr_llama_lora_create(model._h, C.byref(wt), C.byref(lc), None, 0, None, C.byref(h)) == LR_EUNSUPPORTED
    assert b"bias" in L.lr_last_error()
    with pytest.raises(NotImplementedError, match="bias"):
        model.set_fold_norms(True)
    # NULL: the scores of the same weights loaded as a Llama (no biases), kernel for kernel
    llama_cfg = {k: v for k, v in cfg.items() if k != "model_type"}
    llama_sd = {k: v for k, v in sd.items() if not k.endswith(".bias")}
    llama = LlamaRanker.from_state_dict(llama_sd, llama_cfg).set_variants(6, 0)
    want = llama.prefill_verbalize(seqs, LABELS)
    assert L.lr_llama_set_qkv_bias(model._h, None) == 0
    bare = model.prefill_verbalize(seqs, LABELS)
    assert torch.equal(bare, want) and not torch.equal(bare, before)
    assert L.lr_llama_set_folded_norms(model._h, None, None) == 0
    good = (C.c_void_p * nl)(*[model._tensors[f"{i}.bqkv"].data_ptr() for i in range(nl)])
    assert L.lr_llama_set_qkv_bias(model._h, good) == 0
    assert torch.equal(model.prefill_verbalize(seqs, LABELS), before)
    model._bqkv_arr = good


@pytest.mark.parametrize("load_in_4bit", [False, True])
def test_qwen2_from_pretrained_reads_the_biases(golden_dir, tmp_path, load_in_4bit):
    """A local checkpoint directory with Qwen2's bias tensors scores like from_state_dict, also behind the NF4 round trip, which
    leaves the biases alone (bitsandbytes quantises weights only): their bits are the same in both."""
    from safetensors.torch import save_file

    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_qwen2_golden(golden_dir, "hd64_ragged")
    hf = str(tmp_path / "qwen2")
    os.makedirs(hf)
    json.dump(dict(cfg, architectures=["Qwen2ForCausalLM"], torch_dtype="bfloat16"), open(os.path.join(hf, "config.json"), "w"))
    save_file({n: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for n, v in sd.items()},
              os.path.join(hf, "model.safetensors"), metadata={"format": "pt"})
    loaded = LlamaRanker.from_pretrained(hf, load_in_4bit=load_in_4bit)
    assert loaded.hd == 64 and loaded.family == "qwen2" and loaded.max_prompt_len is None
    label_ids = list(z["label_ids"])
    got = loaded.prefill_verbalize(seqs, label_ids)
    same = LlamaRanker.from_state_dict(sd, cfg, nf4=load_in_4bit)
    assert torch.isfinite(got).all() and torch.equal(got, same.prefill_verbalize(seqs, label_ids))
    plain = LlamaRanker.from_state_dict(sd, cfg)
    for i in range(cfg["num_hidden_layers"]):
        assert torch.equal(loaded._tensors[f"{i}.bqkv"], plain._tensors[f"{i}.bqkv"])
        assert torch.equal(loaded._tensors[f"{i}.wqkv"], plain._tensors[f"{i}.wqkv"]) == (not load_in_4bit)
    if load_in_4bit:   # the round trip moved the weights: not the unquantised scores
        assert not torch.equal(got, plain.prefill_verbalize(seqs, label_ids))


def test_train_ranker_synthetic_qwen2_eval_only(tmp_path):
    """`train_ranker.py --synthetic --llm qwen2 --eval_only` with default flags (NF4 on) scores the retrieved users through a
    tiny Qwen2 ranker (biases, ragged widths, 14 heads on 2 KV heads) and writes the reference's metric files."""
    import pickle

    import train_ranker
    import train_retriever

    lru_root = str(tmp_path / "experiments" / "lru" / "synthetic")
    train_retriever.main(["--dataset_code", "synthetic", "--synthetic", "--export_root", lru_root,
                          "--max_train_iterations", "30", "--val_iterations", "10"])
    r = pickle.load(open(os.path.join(lru_root, "retrieved.pkl"), "rb"))
    assert r["test_users"], "the synthetic retriever retrieved nobody"
    out = str(tmp_path / "experiments" / "qwen2" / "synthetic")
    metrics, overall = train_ranker.main(["--dataset_code", "synthetic", "--synthetic", "--llm", "qwen2", "--eval_only",
                                          "--llm_retrieved_path", lru_root, "--export_root", out, "--llm_max_history", "5"])
    assert "test_NDCG@10" in metrics and 0.0 <= metrics["test_NDCG@10"] <= 1.0
    assert os.path.exists(os.path.join(out, "subset_metrics.json")) and os.path.exists(os.path.join(out, "overall_metrics.json"))
