"""GPU: Llama-3.1 / 3.2 rankers -- the llama3-scaled rotary table, attention variant 5 (head_dim-64 MFMA flash attention),
and the whole scoring and LoRA paths on a scaled base against the reference's goldens and the torch restatement."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from llamarec_amd.synth import bf16_bits_to_f32, bf16_round, hash_uniform
from tests.test_gpu_llama import attention, attention_ref, dev_bf16, host_f32
from tests.test_llama3_host import LLAMA3_GOLDENS, load_llama3_golden

LENS = [1, 63, 64, 65, 128, 129, 300, 2, 256, 257, 600, 1125]
GOLDEN_SCALING = dict(kind=1, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_positions=64)


def _scaling(**kw):
    from llamarec_amd import _abi as A

    return A.LrRopeScaling(**kw)


def _rope_table(T, hd, theta, scaling, ex=True):
    """(fp32 table [T][hd/2][2], packed table uint32 [T][hd/2], return code) of lr_rope_table_ex / lr_rope_table."""
    from llamarec_amd._lib import lib, stream_ptr

    nbytes = lib().lr_rope_table_bytes(T, hd)
    assert nbytes == T * (hd // 2) * 12
    buf = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    if ex:
        rc = lib().lr_rope_table_ex(buf.data_ptr(), T, hd, theta, C.byref(scaling) if scaling is not None else None, stream_ptr())
    else:
        rc = lib().lr_rope_table(buf.data_ptr(), T, hd, theta, stream_ptr())
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    return raw[: T * hd].reshape(T, hd // 2, 2), raw[T * hd:].view(np.uint32).reshape(T, hd // 2), rc


def _inv_freq_fp32(hd, theta, s):
    """The rule of include/llamarec_mi355x.h in numpy fp32 (s = None: plain)."""
    f32 = np.float32
    inv = f32(1.0) / np.power(f32(theta), np.arange(0, hd, 2, dtype=np.float32) / f32(hd), dtype=np.float32)
    if s is None:
        return inv
    factor, low, high, orig = f32(s["factor"]), f32(s["low_freq_factor"]), f32(s["high_freq_factor"]), f32(s["original_max_positions"])
    wavelen = f32(2 * np.pi) / inv
    out = inv.copy()
    for j in range(len(inv)):
        if wavelen[j] > orig / low:
            out[j] = inv[j] / factor
        elif not wavelen[j] < orig / high:
            sm = (orig / wavelen[j] - low) / (high - low)
            out[j] = (f32(1) - sm) * inv[j] / factor + sm * inv[j]
    return out.astype(np.float32)


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_table_ex_llama3_against_the_formula(hd):
    T, theta = 512, 500000.0
    cs, cs16, rc = _rope_table(T, hd, theta, _scaling(**GOLDEN_SCALING))
    assert rc == 0 and np.isfinite(cs).all()
    inv = _inv_freq_fp32(hd, theta, GOLDEN_SCALING)
    plain_inv = _inv_freq_fp32(hd, theta, None)
    ratio = plain_inv / inv
    assert (ratio == 1).any() and np.isclose(ratio, 8).any() and ((ratio > 1.01) & (ratio < 7.99)).any()   # three branches
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)   # fp32 product, float64 trig
    assert np.abs(cs[..., 0] - np.cos(ang)).max() <= 2.0 ** -8
    assert np.abs(cs[..., 1] - np.sin(ang)).max() <= 2.0 ** -8
    # ... and it is not the plain table
    pang = (np.arange(T, dtype=np.float32)[:, None] * plain_inv[None, :]).astype(np.float64)
    assert np.abs(cs[..., 0] - np.cos(pang)).max() > 0.5
    # the packed table holds the fp32 table's bits (bf16-representable values)
    bits = cs.view(np.uint32)
    assert not (bits & 0xFFFF).any()
    assert np.array_equal(cs16, (bits[..., 0] >> 16) | (bits[..., 1] & 0xFFFF0000))


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_table_ex_without_scaling_is_lr_rope_table(hd):
    T, theta = 512, 10000.0
    want = _rope_table(T, hd, theta, None, ex=False)
    for s in (None, _scaling(kind=0)):
        got = _rope_table(T, hd, theta, s)
        assert got[2] == 0 and want[2] == 0
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # factor 1 is the plain table too, through the scaled kernel: every branch leaves inv as it is (up to the fp32
    # rounding of the interpolation) -- within one bf16 ulp everywhere
    one = _rope_table(T, hd, theta, _scaling(**dict(GOLDEN_SCALING, factor=1.0)))
    assert np.abs(one[0] - want[0]).max() <= 2.0 ** -8


def test_rope_scaling_words_are_validated(golden_dir):
    from llamarec_amd import _abi as A
    from llamarec_amd._lib import lib
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, "tiny_hd128")
    model = LlamaRanker.from_state_dict(sd, cfg)
    bad = [dict(GOLDEN_SCALING, kind=2), dict(GOLDEN_SCALING, kind=-1), dict(GOLDEN_SCALING, factor=0.5),
           dict(GOLDEN_SCALING, factor=float("nan")), dict(GOLDEN_SCALING, original_max_positions=0),
           dict(GOLDEN_SCALING, original_max_positions=-8), dict(GOLDEN_SCALING, low_freq_factor=0.0),
           dict(GOLDEN_SCALING, low_freq_factor=4.0), dict(GOLDEN_SCALING, low_freq_factor=5.0),
           dict(GOLDEN_SCALING, high_freq_factor=float("nan"))]
    for kw in bad:
        s = _scaling(**kw)
        assert _rope_table(8, 64, 1e4, s)[2] == -1, kw
        assert lib().lr_llama_set_rope_scaling(model._h, C.byref(s)) == -1, kw
    for i in range(3):
        for kind in (0, 1):
            s = _scaling(**dict(GOLDEN_SCALING, kind=kind))
            s.reserved[i] = 1
            assert _rope_table(8, 64, 1e4, s)[2] == -1
            assert lib().lr_llama_set_rope_scaling(model._h, C.byref(s)) == -1 and b"reserved" in lib().lr_last_error()
    # the refusals left the handle's words alone; NULL and kind 0 switch to plain RoPE, the words switch back
    long = np.nonzero(z["lens"] >= 20)[0]
    gap = float(z["bf16_gap"])
    scaled = model.last_logits(seqs).cpu().numpy()
    assert np.abs(scaled - z["logits_bf16"]).max() < 4 * gap
    for off in (None, C.byref(_scaling(kind=0))):
        assert lib().lr_llama_set_rope_scaling(model._h, off) == 0
        plain = model.last_logits(seqs).cpu().numpy()
        assert np.abs(plain - z["logits_fp32_plain_rope"]).max() < 4 * gap
        assert np.abs(plain - z["logits_fp32"])[long].max(axis=1).min() > 2 * gap
        assert lib().lr_llama_set_rope_scaling(model._h, C.byref(_scaling(**GOLDEN_SCALING))) == 0
        assert np.array_equal(model.last_logits(seqs).cpu().numpy(), scaled)


# ---- attention variant 5 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv", [(32, 8), (4, 4), (8, 1), (2, 2)])
def test_hd64_attention_vs_numpy(nh, nkv):
    cu = np.concatenate([[0], np.cumsum(LENS)])
    qkv = bf16_round(hash_uniform(nh * 100 + nkv, (cu[-1], (nh + 2 * nkv) * 64), 1.0))
    got = attention(qkv, cu, nh, nkv, 64, 5)
    ref = attention_ref(qkv, cu, nh, nkv, 64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    print(f"hd64 ({nh}, {nkv}): variant 5 max err {err.max():.5f}")
    assert err.max() < 1.5e-2, err.max()
    gen = attention(qkv, cu, nh, nkv, 64, 1)             # the generic kernel at the same rounding points
    assert np.abs(gen - ref).max() < 1.5e-2


def test_hd64_attention_refuses_other_head_dims_and_lse():
    from llamarec_amd._lib import lib, stream_ptr

    cu = np.array([0, 10], np.int32)
    cud = torch.from_numpy(cu).cuda()
    qkv = torch.zeros((10, 3 * 128), dtype=torch.int16, device="cuda")
    out = torch.zeros((10, 128), dtype=torch.int16, device="cuda")
    rc = lib().lr_attention_varlen(qkv.data_ptr(), out.data_ptr(), cud.data_ptr(), cu.ctypes.data, 1, 1, 1, 128, 5, stream_ptr())
    assert rc == -2 and b"head_dim 64" in lib().lr_last_error()
    lse = torch.zeros((10, 1), dtype=torch.float32, device="cuda")
    rc = lib().lr_attention_varlen_ws(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu.ctypes.data, 1, 1, 1, 64,
                                      5, None, 0, stream_ptr())
    assert rc == -1 and b"lse" in lib().lr_last_error()
    rc = lib().lr_attention_varlen_lse(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), cud.data_ptr(), cu.ctypes.data, 1, 1, 1, 64,
                                       5, stream_ptr())
    assert rc == -1 and b"lse" in lib().lr_last_error()
    torch.cuda.synchronize()


def test_hd64_attention_rows_are_batch_invariant():
    nh, nkv = 8, 2
    rng = np.random.default_rng(1)
    lens = [700, 129, 1125, 5]
    cu = np.concatenate([[0], np.cumsum(lens)])
    qkv = bf16_round(rng.standard_normal((cu[-1], (nh + 2 * nkv) * 64)).astype(np.float32))
    full = attention(qkv, cu, nh, nkv, 64, 5)
    for b in (0, 2, 3):
        alone = attention(qkv[cu[b]:cu[b + 1]], np.array([0, lens[b]]), nh, nkv, 64, 5)
        assert np.array_equal(alone, full[cu[b]:cu[b + 1]]), b


def test_hd64_online_softmax_with_forced_maximum_jumps():
    """test_hd256_online_softmax_with_forced_maximum_jumps (tests/test_gpu_gemma.py) at head_dim 64: keys far into a prompt
    copy the direction of chosen queries at large gains, so some rows' maximum jumps past the deferral threshold at chosen
    (off-diagonal, first, diagonal) blocks; a float64 reference with bf16 probabilities. The gains are twice that test's: a
    spiked score is gain |q|^2 / sqrt(hd) with |q|^2 ~ 0.09 hd, so at a quarter of the width twice the gain gives the same
    scores (with that test's gains only 6 rows jump here and its `jumps > 10` premise fails; with these, 23)."""
    nh = nkv = 2
    hd = 64
    lens = [700, 333]
    cu = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(3)
    n = int(cu[-1])
    qkv = (rng.standard_normal((n, 3 * nh * hd)) * 0.3).astype(np.float32)
    q = qkv[:, : nh * hd].reshape(n, nh, hd)
    k = qkv[:, nh * hd: 2 * nh * hd].reshape(n, nh, hd)
    spikes = [(200, [450, 460, 699], 9.0), (330, [600, 601], 25.0), (70, [500], 3.0), (5, [40, 300], 12.0),
              (640, [650, 690], 14.0), (700 + 100, [700 + 250, 700 + 332], 20.0)]
    for key, qs, gain in spikes:
        for h in range(nh):
            k[key, h] = 2.0 * gain * np.mean([q[j, h] for j in qs], axis=0)
    qkv = bf16_round(qkv)
    got = attention(qkv, cu, nh, nkv, hd, 5)
    qq = qkv[:, : nh * hd].reshape(n, nh, hd).astype(np.float64)
    kk = qkv[:, nh * hd: 2 * nh * hd].reshape(n, nh, hd).astype(np.float64)
    vv = qkv[:, 2 * nh * hd:].reshape(n, nh, hd).astype(np.float64)
    ref = np.zeros((n, nh * hd))
    jumps = 0
    for b in range(len(lens)):
        s, e = cu[b], cu[b + 1]
        T = e - s
        mask = np.tril(np.ones((T, T), bool))
        for h in range(nh):
            sc = np.where(mask, (qq[s:e, h] @ kk[s:e, h].T) / np.sqrt(hd), -np.inf)
            for blk in range(1, (T + 63) // 64):   # a later block's maximum past everything before it by > 2^8
                before = sc[:, : blk * 64].max(-1)
                here = sc[:, blk * 64: (blk + 1) * 64].max(-1)
                jumps += int((((here - before) * 1.4426950408889634) > 8.0).sum())
            p = np.exp(sc - sc.max(-1, keepdims=True))
            ref[s:e, h * hd:(h + 1) * hd] = (p @ vv[s:e, h]) / p.sum(-1, keepdims=True)
    assert jumps > 10
    assert np.isfinite(got).all()
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() < 2.0e-2 * max(1.0, scale), (np.abs(got - ref).max(), scale)


# ---- the scoring path on the reference's goldens -------------------------------------------------------------------------
@pytest.mark.parametrize("name", LLAMA3_GOLDENS)
@pytest.mark.parametrize("variants", [(0, 0), (1, 1), (4, "mfma"), (5, 0)])
def test_llama3_prefill_vs_reference_goldens(golden_dir, name, variants):
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, name)
    gap = float(z["bf16_gap"])
    model = LlamaRanker.from_state_dict(sd, cfg)
    assert model.family == "llama" and model.rope_scaling["factor"] == 8.0 and model.hd == cfg["head_dim"]
    if variants[1] == "mfma":
        variants = (4, 5 if cfg["head_dim"] == 64 else 2)
    model.set_variants(*variants)
    got = model.last_logits(seqs).cpu().numpy()
    assert got.shape == z["logits_bf16"].shape and np.array_equal(got, bf16_round(got))
    print(f"{name} {variants}: vs bf16 {np.abs(got - z['logits_bf16']).max():.4f}, vs fp32 {np.abs(got - z['logits_fp32']).max():.4f}, "
          f"bf16_gap {gap:.4f}")
    assert np.abs(got - z["logits_bf16"]).max() < 4 * gap
    assert np.abs(got - z["logits_fp32"]).max() < 4 * gap
    long = np.nonzero(z["lens"] >= 20)[0]
    assert np.abs(got - z["logits_fp32_plain_rope"])[long].max(axis=1).min() > 2 * gap
    scores = model.prefill_verbalize(seqs, z["label_ids"]).cpu().numpy()
    assert np.array_equal(scores, got[:, z["label_ids"]])


@pytest.mark.parametrize("name", LLAMA3_GOLDENS)
def test_llama3_last_layer_pruning_matches_full_last_layer(golden_dir, name):
    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, name)
    gap = float(z["bf16_gap"])
    model = LlamaRanker.from_state_dict(sd, cfg)
    pruned = model.last_logits(seqs).cpu().numpy()
    full = model.set_last_layer_pruning(False).last_logits(seqs).cpu().numpy()
    assert np.abs(pruned - full).max() < 4 * gap
    assert np.abs(full - z["logits_bf16"]).max() < 4 * gap


def test_full_width_llama32_fast_vs_generic_and_restatement():
    """Llama-3.2-1B layer shapes (32 x 64 GQA heads over 8 KV heads on 2048, tied head, llama3 scaling with factor 32 over
    8192 positions), 2 layers, vocab 32000, random weights, long prompts: the fast path (256-tile GEMMs with the hd-64 RoPE
    epilogue, attention variant 5, pruned last layer) against the generic kernels (1, 1), and both against the fp32 torch
    restatement on the GPU. The generic path's distance to the restatement is measured in the run; the fast path is allowed
    that plus the fast-vs-generic gap test_full_width_gemma_fast_vs_generic_and_restatement allows (5e-2 x scale).
    Measured on an MI355X: max |ref| 2.834; generic vs restatement 0.0419, fast vs restatement 0.0419, fast vs generic
    0.0312; the plain-RoPE restatement is 0.4056 away."""
    from llamarec_amd.llm import LLAMA32_1B, LlamaRanker
    from tests import llama3_ref as R

    cfg = dict(LLAMA32_1B, num_hidden_layers=2, vocab_size=32000)
    sd = R.random_llama_state(cfg, seed=7, device="cuda")
    assert "lm_head.weight" not in sd
    model = LlamaRanker.from_state_dict(sd, cfg)
    rng = np.random.default_rng(2)
    lens = [460, 1125, 700, 5]
    seqs = [np.concatenate([[1], rng.integers(3, 32000, size=n - 1)]).astype(np.int32) for n in lens]
    label_ids = list(range(100, 120))
    fast = model.prefill_verbalize(seqs, label_ids).cpu().numpy()
    gen = model.set_variants(1, 1).prefill_verbalize(seqs, label_ids).cpu().numpy()
    forced = model.set_variants(0, 5).prefill_verbalize(seqs, label_ids).cpu().numpy()
    model.set_variants(0, 0)
    ref = R.last_logits(sd, cfg, seqs, torch.float32, device="cuda")[:, label_ids]
    plain = R.last_logits(sd, cfg, seqs, torch.float32, device="cuda", scaled=False)[:, label_ids]
    scale = max(1.0, float(np.abs(ref).max()))
    gen_err = float(np.abs(gen - ref).max())
    print(f"llama-3.2-1b: max |ref| {np.abs(ref).max():.3f}, fast-ref {np.abs(fast - ref).max():.4f}, gen-ref {gen_err:.4f}, "
          f"fast-gen {np.abs(fast - gen).max():.4f}, plain-ref {np.abs(plain - ref).max():.4f}")
    assert np.isfinite(fast).all() and float(np.abs(fast).max()) > 0.05
    assert np.array_equal(forced, fast)                       # the prefill's auto is variant 5 at head_dim 64
    assert gen_err <= 1e-1 * scale
    assert np.abs(fast - gen).max() <= 5e-2 * scale
    assert np.abs(fast - ref).max() <= gen_err + 5e-2 * scale
    # a prompt's scores do not depend on the rest of the batch
    alone = model.prefill_verbalize([seqs[1]], label_ids).cpu().numpy()
    assert np.array_equal(alone[0], fast[1])


def test_workspace_does_not_grow_with_max_position_embeddings(golden_dir):
    """max_position_embeddings = 131072 (every Llama-3.1 / 3.2 config.json): the rotary table is built for the batch's longest
    prompt, so the prefill's and the LoRA pass's workspaces are sized from the tokens, not from the config's limit."""
    from llamarec_amd._lib import lib
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import LoraTrainEngine

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, "tiny_hd128")
    small = LlamaRanker.from_state_dict(sd, cfg)
    big = LlamaRanker.from_state_dict(sd, dict(cfg, max_position_embeddings=131072))
    n = int(z["lens"].sum())
    a, b = (lib().lr_llama_workspace_bytes(m._h, n, len(seqs)) for m in (small, big))
    assert a > 0 and b - a <= (n - 512) * 128 * 12 + 1024          # 12 bytes per table entry, n - 512 more rows at the most
    assert np.array_equal(big.last_logits(seqs).cpu().numpy(), small.last_logits(seqs).cpu().numpy())
    ea, eb = (LoraTrainEngine(m, dropout=0.0) for m in (small, big))
    wa, wb = (lib().lr_llama_lora_eval_workspace_bytes(e._h, n, len(seqs)) for e in (ea, eb))
    assert wa > 0 and wb - wa <= (n - 512) * 128 * 8 + 1024
    label_ids = list(z["label_ids"])
    assert torch.equal(eb.scores(seqs, label_ids), ea.scores(seqs, label_ids))


def test_lora_on_a_scaled_base_trains_against_scaled_rope(golden_dir):
    """A LoRA engine reaches the rope scaling through its base handle: at initialisation (B = 0) its no-dropout scores are
    the golden's, far from the plain-RoPE scores, and one loss_grad + apply step is finite."""
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.rank_train import IGNORE, LoraTrainEngine

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, "tiny_hd128")
    gap = float(z["bf16_gap"])
    label_ids = list(z["label_ids"])
    eng = LoraTrainEngine(LlamaRanker.from_state_dict(sd, cfg), dropout=0.0, seed=3)
    got = eng.scores(seqs, label_ids).cpu().numpy()
    print(f"lora scores vs golden bf16 {np.abs(got - z['scores_bf16']).max():.4f}, fp32 {np.abs(got - z['scores_fp32']).max():.4f}")
    assert np.abs(got - z["scores_bf16"]).max() < 4 * gap and np.abs(got - z["scores_fp32"]).max() < 4 * gap
    long = np.nonzero(z["lens"] >= 20)[0]
    plain = z["logits_fp32_plain_rope"][:, z["label_ids"]]
    assert np.abs(got - plain)[long].max(axis=1).min() > 2 * gap
    train = [s for s in seqs if len(s) >= 2]
    labels = [np.concatenate([np.full(len(s) - 1, IGNORE), [label_ids[i % 20]]]) for i, s in enumerate(train)]
    loss = float(eng.loss_and_grads(train, labels))
    assert eng.bad_targets == 0 and np.isfinite(loss) and 0.0 < loss < 20.0
    assert torch.isfinite(eng.grads).all() and float(eng.grads.abs().max()) > 0
    norm = float(eng.apply(1e-3, 1.0))
    assert np.isfinite(norm) and norm > 0 and torch.isfinite(eng.params).all()
    assert np.isfinite(eng.scores(seqs, label_ids).cpu().numpy()).all()


def test_llama3_from_pretrained_reads_rope_scaling(golden_dir, tmp_path):
    """A local checkpoint directory as transformers <= 4 writes it: config.json with rope_scaling = llama3 and a tied head
    (no lm_head.weight in the safetensors) scores like from_state_dict."""
    from safetensors.torch import save_file

    from llamarec_amd.llm import LlamaRanker

    z, cfg, sd, seqs = load_llama3_golden(golden_dir, "tiny_hd64_gqa")
    hf = str(tmp_path / "llama32")
    os.makedirs(hf)
    assert cfg["tie_word_embeddings"] and "lm_head.weight" not in sd and "rope_parameters" not in cfg
    json.dump(dict(cfg, architectures=["LlamaForCausalLM"], torch_dtype="bfloat16"), open(os.path.join(hf, "config.json"), "w"))
    save_file({n: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16) for n, v in sd.items()},
              os.path.join(hf, "model.safetensors"), metadata={"format": "pt"})
    loaded = LlamaRanker.from_pretrained(hf)
    assert loaded.hd == 64 and loaded.rope_scaling["original_max_position_embeddings"] == 64 and loaded.rope_theta == 500000.0
    label_ids = list(z["label_ids"])
    got = loaded.prefill_verbalize(seqs, label_ids)
    assert torch.equal(got, LlamaRanker.from_state_dict(sd, cfg).prefill_verbalize(seqs, label_ids))
    assert np.abs(got.cpu().numpy() - z["scores_bf16"]).max() < 4 * float(z["bf16_gap"])
