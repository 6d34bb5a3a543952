"""GPU: shared-prefix and last-row attention at head_dim 64 and 256 (llama_attn_hd64_prefix.hip, llama_attn_hd256_prefix.hip)
and at head_dim 128 (variant 2's modes, which had no stand-alone entry point), through lr_attention_varlen_prefix and
lr_attention_last_rows, and through the prefill of the committed head_dim-64 / -256 goldens.

The contract is bit identity: a row of the prefix layout ([P shared rows][rest of prompt 0]..[rest of prompt B-1]) carries the
bits the pinned kernel (variant 5 / 4 / 2 through lr_attention_varlen) writes for the same row of the same WHOLE prompt, and
the last-row kernel writes the bits of row T - 1. The prefix kernel is also held to the float64 bound of tests/stage2_ref.py."""
import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, f32_to_bf16_bits
from tests import stage2_ref as R

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
# (head_dim, variant, num_heads, num_kv_heads)
SHAPES = [(64, 5, 4, 2), (64, 5, 8, 1), (64, 5, 2, 2), (256, 4, 4, 1), (256, 4, 2, 2), (128, 2, 4, 2)]
PREFIXES = [1, 36, 63, 64, 65, 127, 128, 129, 191]   # every side of the 64-key block and the 128-row tile
TAILS = [1, 4, 70, 130, 61]
GUARD = 3          # rows behind `out` that must keep their bits
POISON = 0x7FC0    # bf16 NaN


def _bits(x):
    return torch.from_numpy(f32_to_bf16_bits(x).view(np.int16)).cuda()


def _lib():
    from llamarec_amd._lib import lib, stream_ptr

    return lib(), stream_ptr()


def _whole_prompts(regime, P, tails, nh, nkv, hd):
    """bf16-valued qkv of whole prompts (P prefix rows + tail each) whose first P rows repeat prompt 0's, and their starts."""
    cu = np.concatenate([[0], np.cumsum([P + t for t in tails])]).astype(np.int64)
    qkv = R.attention_data(regime, cu, nh, nkv, hd)
    for b in range(1, len(tails)):
        qkv[cu[b]:cu[b] + P] = qkv[:P]
    return qkv, cu


def _prefix_layout(qkv, cu, P):
    """Rows of the prefix layout, segment starts [S + 1], and for every layout row its row in the whole-prompt array."""
    B = len(cu) - 1
    if P == 0:
        return qkv, cu.astype(np.int32), np.arange(len(qkv))
    src = np.concatenate([np.arange(P)] + [np.arange(cu[b] + P, cu[b + 1]) for b in range(B)])
    seg = np.concatenate([[0, P], P + np.cumsum([cu[b + 1] - cu[b] - P for b in range(B)])]).astype(np.int32)
    return qkv[src], seg, src


def _full(qkv_d, cu, nh, nkv, hd, variant):
    """The pinned kernel on whole prompts: bf16 bits [n][nh * hd]."""
    L, st = _lib()
    cu32 = np.ascontiguousarray(cu, dtype=np.int32)
    out = torch.full((int(cu[-1]), nh * hd), POISON, dtype=torch.int16, device="cuda")
    cud = torch.from_numpy(cu32).cuda()
    rc = L.lr_attention_varlen(qkv_d.data_ptr(), out.data_ptr(), cud.data_ptr(), cu32.ctypes.data,
                               len(cu) - 1, nh, nkv, hd, variant, st)
    torch.cuda.synchronize()
    assert rc == 0, L.lr_last_error()
    return out.cpu().numpy()


def _prefix_call(rows_d, seg, P, nh, nkv, hd, variant, fill=POISON):
    L, st = _lib()
    n = int(seg[-1])
    out = torch.full((n + GUARD, nh * hd), fill, dtype=torch.int16, device="cuda")
    segd = torch.from_numpy(seg).cuda()
    rc = L.lr_attention_varlen_prefix(rows_d.data_ptr(), out.data_ptr(), segd.data_ptr(), seg.ctypes.data, len(seg) - 1, P, nh, nkv,
                                      hd, variant, st)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


_FULL_CACHE = {}


def _case(regime, P, shape):
    """(whole qkv, cu, pinned kernel's bits, float64 reference and bound), computed once per (regime, P, shape)."""
    key = (regime, P, shape)
    if key not in _FULL_CACHE:
        hd, variant, nh, nkv = shape
        qkv, cu = _whole_prompts(regime, P, TAILS, nh, nkv, hd)
        full = _full(_bits(qkv), cu, nh, nkv, hd, variant)
        ref, _, bound, _ = R.attention_ref64(qkv, cu, nh, nkv, hd)
        _FULL_CACHE[key] = (qkv, cu, full, ref, bound)
    return _FULL_CACHE[key]


@pytest.mark.parametrize("regime", ["flat", "last_block"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "hd%d_v%d_%dx%d" % s)
def test_prefix_kernel_is_bit_identical_to_the_whole_prompt_and_within_bound(shape, regime):
    hd, variant, nh, nkv = shape
    for P in PREFIXES:
        qkv, cu, full, ref, bound = _case(regime, P, shape)
        rows, seg, src = _prefix_layout(qkv, cu, P)
        assert int(seg[-1]) <= 460
        for v in (variant, 0):
            rc, got = _prefix_call(_bits(rows), seg, P, nh, nkv, hd, v)
            assert rc == 0, (P, v, _lib()[0].lr_last_error())
            n = int(seg[-1])
            assert (got[n:].view(np.uint16) == POISON).all(), (P, v, "guard rows written")
            # segment 0 == prompt rows < P, segments >= 1 == the whole prompts' rows at positions >= P
            diff = np.flatnonzero((got[:n] != full[src]).any(axis=1))
            assert diff.size == 0, (P, v, "rows differ from the pinned kernel", diff[:8], np.searchsorted(seg, diff[:8], "right") - 1)
            r = R.ratio(bf16_bits_to_f32(got[:n].view(np.uint16)), ref[src], bound[src])
            print(f"prefix attention {regime} hd={hd} v{v} nh={nh} nkv={nkv} P={P}: err/bound {r:.3f}")
            assert r <= 1.0, (P, v, r)


LAST_T = [1, 2, 63, 64, 65, 128, 129, 200]


@pytest.mark.parametrize("P", [0, 36, 64, 129])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "hd%d_v%d_%dx%d" % s)
def test_last_row_kernel_equals_row_T_minus_1_of_the_full_kernel(shape, P):
    """One batch of prompts with LAST_T own rows each behind P shared ones (P = 0: T = LAST_T exactly)."""
    hd, variant, nh, nkv = shape
    L, st = _lib()
    qkv, cu = _whole_prompts("flat", P, LAST_T, nh, nkv, hd)
    full = _full(_bits(qkv), cu, nh, nkv, hd, variant)
    rows, seg, _ = _prefix_layout(qkv, cu, P)
    B = len(LAST_T)
    kv = np.ascontiguousarray(rows[:, nh * hd:])
    q_last = np.ascontiguousarray(qkv[cu[1:] - 1, :nh * hd])
    kv_d, q_d, segd = _bits(kv), _bits(q_last), torch.from_numpy(seg).cuda()
    for v in (variant, 0):
        out = torch.full((B + GUARD, nh * hd), POISON, dtype=torch.int16, device="cuda")
        rc = L.lr_attention_last_rows(kv_d.data_ptr(), q_d.data_ptr(), out.data_ptr(), segd.data_ptr(), seg.ctypes.data, len(seg) - 1,
                                      P, nh, nkv, hd, v, st)
        torch.cuda.synchronize()
        assert rc == 0, L.lr_last_error()
        got = out.cpu().numpy()
        assert (got[B:].view(np.uint16) == POISON).all(), "rows past the prompts written"
        bad = np.flatnonzero((got[:B] != full[cu[1:] - 1]).any(axis=1))
        assert bad.size == 0, (v, "prompts whose last row differs", bad, [LAST_T[i] for i in bad])


def test_refusals_leave_outputs_untouched():
    L, st = _lib()
    nh, nkv = 4, 2

    def both(seg, P, hd, variant, want):
        seg = np.asarray(seg, dtype=np.int32)
        n = max(int(seg.max()), 1)
        rows = torch.zeros((n, (nh + 2 * nkv) * hd), dtype=torch.int16, device="cuda")
        rc, out = _prefix_call(rows, seg, P, nh, nkv, hd, variant, fill=0x1234)
        assert rc == want, (seg, P, hd, variant, rc, L.lr_last_error())
        assert (out == 0x1234).all()
        S = len(seg) - 1
        q = torch.zeros((S, nh * hd), dtype=torch.int16, device="cuda")
        o = torch.full((S, nh * hd), 0x1234, dtype=torch.int16, device="cuda")
        segd = torch.from_numpy(seg).cuda()
        rc = L.lr_attention_last_rows(rows.data_ptr(), q.data_ptr(), o.data_ptr(), segd.data_ptr(), seg.ctypes.data, S, P, nh, nkv,
                                      hd, variant, st)
        torch.cuda.synchronize()
        assert rc == want, (seg, P, hd, variant, rc, L.lr_last_error())
        assert (o.cpu().numpy() == 0x1234).all()

    for hd, v in ((64, 5), (256, 4), (128, 2)):
        both([0, 35, 70, 90], 36, hd, v, LR_EINVAL)        # segment 0 != prefix_len
        both([0, 37, 70, 90], 36, hd, v, LR_EINVAL)
        both([0, 36, 36, 90], 36, hd, v, LR_EINVAL)        # an empty segment
        both([0, 36, 90, 80], 36, hd, v, LR_EINVAL)        # decreasing starts
        both([1, 37, 90], 36, hd, v, LR_EINVAL)            # starts[0] != 0
        both([0, 36], 36, hd, v, LR_EINVAL)                # a prefix and no prompt
        both([0, 36, 90], -1, hd, v, LR_EINVAL)
        both([0, 36, 90], 36, hd, 1, LR_EUNSUPPORTED)      # the generic kernel reads no prefix
    both([0, 36, 90], 36, 128, 5, LR_EUNSUPPORTED)         # variant 5 at head_dim 128
    both([0, 36, 90], 36, 64, 4, LR_EUNSUPPORTED)          # variant 4 at head_dim 64
    both([0, 36, 90], 36, 256, 5, LR_EUNSUPPORTED)
    both([0, 36, 90], 36, 32, 0, LR_EUNSUPPORTED)          # no MFMA kernel at this head_dim
    # num_heads % num_kv_heads
    seg = np.array([0, 36, 90], dtype=np.int32)
    rows = torch.zeros((90, 5 * 64), dtype=torch.int16, device="cuda")
    out = torch.full((90, 3 * 64), 0x1234, dtype=torch.int16, device="cuda")
    segd = torch.from_numpy(seg).cuda()
    rc = L.lr_attention_varlen_prefix(rows.data_ptr(), out.data_ptr(), segd.data_ptr(), seg.ctypes.data, 2, 36, 3, 2, 64, 5, st)
    torch.cuda.synchronize()
    assert rc == LR_EINVAL and (out.cpu().numpy() == 0x1234).all()


# ---------------------------------------------------------------------------------------------------------------------
# model level, on the committed goldens
# ---------------------------------------------------------------------------------------------------------------------
def _prefixed_prompts(P, tails, vocab, seed):
    rng = np.random.default_rng(seed)
    prefix = np.concatenate([[1], rng.integers(3, vocab, size=P - 1)]) if P > 1 else np.array([1])
    return [np.concatenate([prefix, rng.integers(3, vocab, size=n)]).astype(np.int32) for n in tails]


# (golden, attention variant of its head_dim)
GOLDENS = [("llama3_tiny_hd64_gqa", 5), ("gemma_tiny_hd256_mqa", 4), ("gemma_tiny_hd256_wide", 4)]
_MODELS = {}


def _model(golden_dir, name):
    """(ranker, config) of a golden's weights, with room for the longest test prompt; built once per golden."""
    if name not in _MODELS:
        from llamarec_amd.llm import LlamaRanker
        from tests.test_gemma_host import load_gemma_golden
        from tests.test_llama3_host import load_llama3_golden

        fam, rest = name.split("_", 1)
        z, cfg, sd, seqs = (load_llama3_golden if fam == "llama3" else load_gemma_golden)(golden_dir, rest)
        assert cfg["max_position_embeddings"] >= 130 + 90, cfg["max_position_embeddings"]
        _MODELS[name] = (LlamaRanker.from_state_dict(sd, cfg), cfg)
    model, cfg = _MODELS[name]
    model.set_variants(0, 0).set_last_layer_pruning(True)
    return model, cfg


def _gemm_rows(L):
    """[(epilogue, N, K, rows)] of every GEMM launch of the profiled region (rows = work / (2 N K), N and K from the tag)."""
    recs = []
    for kind in (0, 1):
        n = L.lr_profile_records(kind, None, None, None, 0)
        if n <= 0:
            continue
        ms, work, tag = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
        assert L.lr_profile_records(kind, ms.ctypes.data, work.ctypes.data, tag.ctypes.data, n) == n
        for w, t in zip(work, tag):
            epi, N, K = int(t >> 56), int((t >> 28) & ((1 << 28) - 1)), int(t & ((1 << 28) - 1))
            recs.append((epi, N, K, int(round(w / (2.0 * N * K)))))
    return recs


MODEL_TAILS = [1, 7, 40, 90]
LABELS = list(range(40, 60))


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_shared_prefix_prefill_is_bit_identical_at_hd64_and_hd256(golden_dir, name, variant):
    from llamarec_amd.llm import common_prefix_len, pack_prompts

    model, cfg = _model(golden_dir, name)
    lab = torch.as_tensor(np.asarray(LABELS, dtype=np.int32)).cuda()
    for P in (5, 36, 64, 70, 130):
        seqs = _prefixed_prompts(P, MODEL_TAILS, cfg["vocab_size"], P)
        ids, cu = pack_prompts(seqs)
        assert common_prefix_len(ids, cu) >= P
        for prune in (True, False):
            for v in (0, variant):
                model.set_variants(0, v).set_last_layer_pruning(prune)
                shared = model.prefill_verbalize(seqs, LABELS, share_prefix=True)
                plain = model.prefill_verbalize(seqs, LABELS, share_prefix=False)
                assert torch.isfinite(plain).all() and torch.equal(shared, plain), (P, prune, v)
                part = model.prefill_verbalize_packed(torch.from_numpy(ids).cuda(), torch.from_numpy(cu).cuda(), cu, lab,
                                                      prefix_len=P - 3)
                assert torch.equal(part, plain), (P, prune, v)


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_shared_prefix_and_last_row_mode_are_executed_at_hd64_and_hd256(golden_dir, name, variant):
    """The profile of one shared call: the first layer's qkv product runs on n - (B - 1) P rows, and the pruned last layer
    runs a K | V product (N = 2 nkv hd) over all rows and a Q product (N = nh hd) over the B last rows."""
    from llamarec_amd._lib import lib

    L = lib()
    model, cfg = _model(golden_dir, name)
    P, B = 36, len(MODEL_TAILS)
    seqs = _prefixed_prompts(P, MODEL_TAILS, cfg["vocab_size"], 7)
    n_in = sum(len(s) for s in seqs)
    n = n_in - (B - 1) * P
    d, nh, nkv, hd = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    q_w, kv_w = nh * hd, 2 * nkv * hd
    for v in (0, variant):
        model.set_variants(0, v)
        model.prefill_verbalize(seqs, LABELS, share_prefix=True)   # warm (workspace allocation outside the profiled call)
        assert L.lr_profile_start(4096) == 0
        model.prefill_verbalize(seqs, LABELS, share_prefix=True)
        torch.cuda.synchronize()
        assert L.lr_profile_stop() == 0
        recs = _gemm_rows(L)
        print(name, v, recs)
        rope = sorted((N, rows) for epi, N, K, rows in recs if epi == 3 and K == d)   # the qkv products (rotary epilogue)
        want = sorted([(q_w + kv_w, n)] * (cfg["num_hidden_layers"] - 1) + [(kv_w, n), (q_w, B)])
        assert rope == want, (rope, want, n_in)
        assert n_in not in [r[3] for r in recs], recs


@pytest.mark.parametrize("name,variant", GOLDENS[:2])
def test_shared_prefix_promise_is_verified_on_the_device_at_hd64_and_hd256(golden_dir, name, variant):
    from llamarec_amd.llm import pack_prompts

    model, cfg = _model(golden_dir, name)
    V = cfg["vocab_size"]
    seqs = _prefixed_prompts(8, [5, 9, 30], V, 0)
    lab = torch.arange(40, 60, dtype=torch.int32).cuda()
    ids, cu = pack_prompts(seqs)

    def run(i, p):
        return model.prefill_verbalize_packed(torch.from_numpy(i).cuda(), torch.from_numpy(cu).cuda(), cu, lab, prefix_len=p)

    good = run(ids, 8)
    assert torch.isfinite(good).all()
    lying = ids.copy()
    lying[cu[2] + 5] = (lying[cu[2] + 5] + 1) % V or 3          # prompt 2 no longer shares token 5
    assert torch.isnan(run(lying, 8)).all()
    assert torch.isfinite(run(lying, 5)).all()
    assert torch.equal(run(ids, 8), good)                         # the flag is per call


@pytest.mark.parametrize("which", ["llama32_1b", "gemma_2b"])
def test_full_width_one_layer_shared_pruned_equals_plain_pruned(which):
    from llamarec_amd.llm import GEMMA_2B, LLAMA32_1B, LlamaRanker

    if which == "gemma_2b":
        from tests import gemma_ref as G

        cfg = dict(GEMMA_2B, num_hidden_layers=1, vocab_size=32000)
        sd = G.random_gemma_state(cfg, seed=7, device="cuda")
    else:
        from tests import llama3_ref as G

        cfg = dict(LLAMA32_1B, num_hidden_layers=1, vocab_size=32000)
        sd = G.random_llama_state(cfg, seed=7, device="cuda")
    model = LlamaRanker.from_state_dict(sd, cfg)
    rng = np.random.default_rng(3)
    prefix = np.concatenate([[2], rng.integers(3, 32000, size=35)])
    seqs = [np.concatenate([prefix, rng.integers(3, 32000, size=n - 36)]).astype(np.int32) for n in (460, 700, 1125, 37 + 5)]
    labels = list(range(100, 120))
    shared = model.prefill_verbalize(seqs, labels, share_prefix=True)
    plain = model.prefill_verbalize(seqs, labels, share_prefix=False)
    assert torch.isfinite(plain).all() and torch.equal(shared, plain)
    full = model.set_last_layer_pruning(False).prefill_verbalize(seqs, labels, share_prefix=True)
    full_plain = model.prefill_verbalize(seqs, labels, share_prefix=False)
    assert torch.equal(full, full_plain)
    gap = (shared - full).abs().max().item()
    print(f"{which}: pruned vs unpruned {gap:.4f}")
    assert gap < 2e-2
