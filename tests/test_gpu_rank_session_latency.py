"""GPU: ranker sessions in the row-invariant latency mode, gemm variant 7 (DESIGN 16 "Latency mode"). Under it
lr_llama_extend_verbalize runs every n-row product split over K, with the split fixed by the weight's shape, and must carry the
BITS of lr_llama_prefill_verbalize of the whole prompt under variant 7; where the QKV product splits, its reduce pass writes
K | V straight into the slot rows, and LR_EXTEND_SEPARATE_CACHE_WRITE=1 (tests and benches only) keeps the two-launch form as
the bitwise yardstick. Models, prompts and helpers are those of tests/test_gpu_rank_session.py.

The tiny models have hidden size 256, i.e. 4 K tiles: LR_GEMM_SPLITK_MIN_TILES=1 makes all four products split there (4, 4, 4
and 8 runs; test 1 asserts it through lr_gemm_splitk_plan), layer 0 through the q | K | V product and the pruned last layer
through the K | V-only one."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_rank_session import LABELS, LR_EINVAL, LR_EUNSUPPORTED, MAX_TOKENS, _bits, _model, _raw_extend

pytestmark = pytest.mark.gpu

CACHED = [63, 64, 65, 127, 128, 129]   # one below, at and one above the 64-key block and the 128-row query tile
NEW = [1, 64, 65, 130]                 # 127 / 128 / 129 + 130: a whole prompt of 257 .. 259 rows, past one row tile


@pytest.fixture
def split_everything(monkeypatch):
    monkeypatch.setenv("LR_GEMM_SPLITK_MIN_TILES", "1")   # monkeypatch puts the environment back
    yield


def _whole7(model, seq):
    """fp32 bits of the whole-prompt call's scores; the caller has set the variant."""
    return _bits(model.prefill_verbalize([np.asarray(seq, dtype=np.int32)], LABELS))[0]


def _splits(variant, M, N, K):
    from llamarec_amd._lib import lib

    s, r = C.c_int32(0), C.c_int32(0)
    assert lib().lr_gemm_splitk_plan(variant, M, N, K, 64 << 20, C.byref(s), C.byref(r)) == 0
    return s.value


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit identity with the whole prompt under variant 7
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_hd128", "hd128_mqa"])
def test_split_prompt_scores_equal_whole_prompt_bits_under_variant_7(golden_dir, split_everything, name):
    model, ids, _ = _model(golden_dir, name)
    c = model.config
    d, f, q_w = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"] * model.hd
    kv_w = 2 * c["num_key_value_heads"] * model.hd
    for M in (1, 130, 259):   # every product of the call splits, the same way at every row count
        assert [_splits(7, M, N, K) for N, K in ((q_w + kv_w, d), (kv_w, d), (d, q_w), (2 * f, d), (d, f))] == [4, 4, 4, 4, 8]
    bad = []
    try:
        model.set_variants(7, 0)
        whole = {T: _whole7(model, ids[:T]) for T in sorted({c_ + q for c_ in CACHED for q in NEW})}
        cache = model.new_prompt_cache(1, MAX_TOKENS)
        for c_ in CACHED:
            model.extend_verbalize(cache, [0], [ids[:c_]], LABELS, keep=[c_], cached_len=[0])
            for q in NEW:   # keep = 0: the new rows are scratch, the slot still holds exactly the first c_ tokens
                got = _bits(model.extend_verbalize(cache, [0], [ids[c_:c_ + q]], LABELS, keep=[0]))[0]
                if not np.array_equal(got, whole[c_ + q]):
                    bad.append((c_, q))
    finally:
        model.set_variants(0, 0)
    assert not bad, f"{name}: (cached_len, new) pairs whose scores differ from the variant-7 whole prompt's: {bad}"


# ---------------------------------------------------------------------------------------------------------------------
# 2. Llama-2-7b's widths, no override: the split the online path really runs, and the fused cache write against the copy
# ---------------------------------------------------------------------------------------------------------------------
def test_full_width_layer_carries_the_variant_7_bits_and_the_copy_kernels_slot_bytes(monkeypatch):
    """One layer at Llama-2-7b's widths (tests/test_gpu_llama.py::test_full_width_batch_invariance's model). T = 300 extended
    as 140 and then 160. The tolerance against the default mode is the one that test gives latency mode."""
    from llamarec_amd.llm import LLAMA2_7B, LlamaRanker

    monkeypatch.delenv("LR_GEMM_SPLITK_MIN_TILES", raising=False)
    monkeypatch.delenv("LR_EXTEND_SEPARATE_CACHE_WRITE", raising=False)
    cfg = dict(LLAMA2_7B, num_hidden_layers=1)
    model = LlamaRanker.random_init(cfg, seed=7)
    seq = np.concatenate([[1], np.random.default_rng(0).integers(3, 32000, size=299)]).astype(np.int32)
    labels = list(range(319, 339))
    kv_w = 2 * cfg["num_key_value_heads"] * model.hd
    rows = 300 * kv_w * 2   # bytes of layer 0's rows 0 .. 299 at the head of a slot

    def two_calls(cache, slot):
        model.extend_verbalize(cache, [slot], [seq[:140]], labels)
        return model.extend_verbalize(cache, [slot], [seq[140:]], labels)

    try:
        for prune in (True, False):   # the K | V-only product of the pruned layer, then the q | K | V product
            default = model.set_variants(0, 0).set_last_layer_pruning(prune).prefill_verbalize([seq], labels)
            model.set_variants(7, 0)
            whole = model.prefill_verbalize([seq], labels)
            cache = model.new_prompt_cache(2, 320)
            cache.table.fill_(0x5A)
            fused = two_calls(cache, 0)
            monkeypatch.setenv("LR_EXTEND_SEPARATE_CACHE_WRITE", "1")
            copied = two_calls(cache, 1)
            monkeypatch.delenv("LR_EXTEND_SEPARATE_CACHE_WRITE")
            diff, bound = float((whole - default).abs().max()), 5e-2 * max(1.0, float(default.abs().max()))
            print(f"prune={prune}: variant 7 vs default mode, max score diff {diff:.3e} (bound {bound:.3e})")
            assert torch.isfinite(whole).all() and np.array_equal(_bits(fused), _bits(whole)), prune
            assert np.array_equal(_bits(copied), _bits(whole)), prune
            assert diff < bound
            assert torch.equal(cache.table[0, :rows], cache.table[1, :rows]), prune
            assert not (cache.table[0, :rows].view(torch.int16).view(300, kv_w) == 0x5A5A).all(dim=1).any(), "a row was not written"
            assert (cache.table[:, rows:] == 0x5A).all(), "bytes behind row 299 were written"
    finally:
        model.set_variants(0, 0).set_last_layer_pruning(True)


# ---------------------------------------------------------------------------------------------------------------------
# 3. three users in one call: 135 + 131 + 7 = 273 new rows, a row-tile boundary inside the second prompt
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_hd128", "hd128_mqa"])
def test_three_prompts_in_one_call_under_variant_7(golden_dir, split_everything, name):
    model, ids, _ = _model(golden_dir, name)
    rng = np.random.default_rng(5)
    vocab = model.config["vocab_size"]
    prompts = [np.concatenate([[1], rng.integers(3, vocab, size=n - 1)]).astype(np.int32) for n in (200, 131, 77)]
    cached = [65, 0, 70]
    slots = [2, 0, 1]
    assert [len(p) - c for p, c in zip(prompts, cached)] == [135, 131, 7]
    try:
        model.set_variants(7, 0)
        cache = model.new_prompt_cache(4, MAX_TOKENS)
        cache.table.fill_(0x5A)
        for b in (0, 2):
            model.extend_verbalize(cache, [slots[b]], [prompts[b][:cached[b]]], LABELS)
        unused = cache.table[3].clone()
        got = _bits(model.extend_verbalize(cache, slots, [p[c:] for p, c in zip(prompts, cached)], LABELS))
        whole = [_whole7(model, p) for p in prompts]
    finally:
        model.set_variants(0, 0)
    for b in range(3):
        assert np.array_equal(got[b], whole[b]), b
        assert cache.ids[slots[b]] == prompts[b].tolist()
    assert torch.equal(cache.table[3], unused) and (unused == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. a chain, keep and rollback
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_keep_and_rollback_under_variant_7(golden_dir, split_everything):
    model, ids, _ = _model(golden_dir, "tiny_hd128")
    other = np.random.default_rng(23).integers(3, model.config["vocab_size"], size=90).astype(np.int32)
    try:
        model.set_variants(7, 0)
        cache = model.new_prompt_cache(2, MAX_TOKENS)
        for cut in ((0, 100), (100, 129), (129, 259)):
            chained = model.extend_verbalize(cache, [1], [ids[cut[0]:cut[1]]], LABELS)
        once = model.extend_verbalize(cache, [0], [ids], LABELS)
        assert np.array_equal(_bits(chained)[0], _bits(once)[0])
        assert np.array_equal(_bits(chained)[0], _whole7(model, ids))
        cache = model.new_prompt_cache(1, MAX_TOKENS)
        model.extend_verbalize(cache, [0], [ids[:70]], LABELS)
        model.extend_verbalize(cache, [0], [ids[70:200]], LABELS, keep=[60])      # rows 130 .. 199 are scratch afterwards
        assert cache.ids[0] == ids[:130].tolist()
        got = _bits(model.extend_verbalize(cache, [0], [other], LABELS))[0]      # from cached_len = 70 + 60, other tokens
        assert np.array_equal(got, _whole7(model, np.concatenate([ids[:130], other])))
        got = _bits(model.extend_verbalize(cache, [0], [other[:33]], LABELS, cached_len=[97]))[0]   # rolled back below the kept
        assert np.array_equal(got, _whole7(model, np.concatenate([ids[:97], other[:33]])))
        assert cache.ids[0] == np.concatenate([ids[:97], other[:33]]).tolist()
    finally:
        model.set_variants(0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. up to one row tile variant 7 is variant 5, 6. a variant-5 handle keeps the default-mode bits in the extend call
# ---------------------------------------------------------------------------------------------------------------------
def test_variant_7_is_variant_5_up_to_256_tokens(golden_dir, split_everything):
    model, ids, _ = _model(golden_dir, "tiny_hd128")
    try:
        for T in (1, 129, 256):
            seven = _whole7(model.set_variants(7, 0), ids[:T])
            five = _whole7(model.set_variants(5, 0), ids[:T])
            assert np.array_equal(seven, five), T
        three = [ids[:100], ids[7:90], ids[40:113]]   # 256 rows in one batch
        seven = _bits(model.set_variants(7, 0).prefill_verbalize(three, LABELS))
        assert np.array_equal(seven, _bits(model.set_variants(5, 0).prefill_verbalize(three, LABELS)))
        for b in range(3):   # and under 7 a prompt's bits do not depend on the batch
            assert np.array_equal(seven[b], _whole7(model.set_variants(7, 0), three[b])), b
    finally:
        model.set_variants(0, 0)


def test_variant_5_handle_still_extends_with_the_default_mode_bits(golden_dir, split_everything):
    """A guard: the split of variant 5 depends on the row count, so its handle runs the default-mode products in the call."""
    model, ids, _ = _model(golden_dir, "tiny_hd128")
    whole = _whole7(model.set_variants(0, 0), ids[:259])
    try:
        model.set_variants(5, 0)
        cache = model.new_prompt_cache(1, MAX_TOKENS)
        model.extend_verbalize(cache, [0], [ids[:129]], LABELS)
        got = _bits(model.extend_verbalize(cache, [0], [ids[129:259]], LABELS))[0]
    finally:
        model.set_variants(0, 0)
    assert np.array_equal(got, whole)


# ---------------------------------------------------------------------------------------------------------------------
# 7. RankerSession.rank against rank_candidates, both under variant 7
# ---------------------------------------------------------------------------------------------------------------------
def test_ranker_session_matches_rank_candidates_under_variant_7(split_everything):
    from llamarec_amd import data as D
    from llamarec_amd import inference as I
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.synth import synth_llama_state
    from llamarec_amd.verb import ManualVerbalizer
    from tests.fake_tokenizer import FakeTokenizer

    ds = D.synthetic_dataset(num_users=5, num_items=400, seed=3)
    tok = FakeTokenizer()
    cfg = dict(vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
               num_key_value_heads=2, max_position_embeddings=2048, rms_norm_eps=1e-5, rope_theta=10000.0)
    ranker = LlamaRanker.from_state_dict(synth_llama_state(cfg, 11), cfg).set_variants(7, 0)
    verb = ManualVerbalizer(tokenizer=tok, classes=list(range(20)), label_words={i: chr(65 + i) for i in range(20)})
    items = ds["train"][1]
    history, more = list(items[-8:-1]), list(items[-8:])
    pool = [int(i) for i in range(30, 50)]
    pool2 = [int(i) for i in range(120, 140)]
    try:
        session = I.RankerSession(ranker, tok, verb, max_tokens=2048)
        sent = []
        for query, cands in ((history, pool), (more, pool), (more, pool2)):
            prompt = I.generate_prompt(query, cands, ds["meta"])
            assert session.rank(prompt, cands, top_k=10) == I.rank_candidates(ranker, tok, prompt, cands, verb, top_k=10)
            sent.append((session.last_sent, len(tok(prompt)["input_ids"])))
    finally:
        ranker.set_variants(0, 0)
    assert sent[0][0] == sent[0][1] and 0 < sent[1][0] < sent[1][1] and 0 < sent[2][0] < sent[2][1], sent


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals are what they were
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_under_variant_7_leave_scores_and_table_untouched(golden_dir, split_everything):
    from llamarec_amd._lib import lib

    model, ids, _ = _model(golden_dir, "tiny_hd128")
    cache = model.new_prompt_cache(3, MAX_TOKENS)
    cache.table.fill_(0x3C)
    table0 = cache.table.clone()
    out = torch.full((2, len(LABELS)), -123.0, device="cuda")
    out0 = out.clone()
    a, b = ids[:5], ids[5:12]
    c = model.config
    width = (c["num_attention_heads"] + 2 * c["num_key_value_heads"]) * model.hd
    biases = [torch.zeros(width, dtype=torch.bfloat16, device="cuda") for _ in range(c["num_hidden_layers"])]
    arr = (C.c_void_p * len(biases))(*[t.data_ptr() for t in biases])
    try:
        model.set_variants(7, 0)
        rc, msg = _raw_extend(model, cache.table, 3, [1, 1], [0, 0], [a, b], [5, 7], out)
        assert rc == LR_EINVAL and "same slot" in msg, (rc, msg)
        assert torch.equal(out, out0) and torch.equal(cache.table, table0)
        assert lib().lr_llama_set_qkv_bias(model._h, arr) == 0
        try:
            rc, msg = _raw_extend(model, cache.table, 3, [0, 1], [0, 0], [a, b], [5, 7], out)
        finally:
            assert lib().lr_llama_set_qkv_bias(model._h, None) == 0
        assert rc == LR_EUNSUPPORTED and "bias" in msg, (rc, msg)
        assert torch.equal(out, out0) and torch.equal(cache.table, table0)
        rc, msg = _raw_extend(model, cache.table, 3, [0, 1], [0, 0], [a, b], [5, 7], out)   # the same arguments, accepted, write
        assert rc == 0, msg
        assert not torch.equal(out, out0) and not torch.equal(cache.table, table0) and torch.equal(cache.table[2], table0[2])
    finally:
        model.set_variants(0, 0)
