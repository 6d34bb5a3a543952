"""GPU: ranker sessions -- lr_llama_extend_verbalize, lr_attention_varlen_cached, LlamaRanker.extend_verbalize and
inference.RankerSession. A user's cache slot holds the rotated keys and the values of a prompt prefix; a call
prefills only the new tokens. The scores must carry the BITS of lr_llama_prefill_verbalize on the whole prompt.

Models: the tiny goldens' configs and weight seeds (llama_tiny_hd128: head_dim 128, the MFMA attention route; llama_tiny_gqa:
4 query heads on 2 KV heads at head_dim 32 and llama_tiny_hd16: the generic route), with max_position_embeddings raised from
256 to 512 -- the weights do not depend on it and the boundary cases below reach 259 tokens -- and "hd128_mqa", the hd128
config with ONE KV head, so that GQA also runs end to end on the MFMA kernel.

The stand-alone attention is compared with a float64 reference of this file within the bound of tests/stage2_ref.py's
module docstring (same rounding points: fp32 scores, bf16 P, fp32 sums, bf16 output):
    |got - ref| <= 2^-8 |ref| + (2^-8 + T 2^-24 + 2 eps) S,   S = sum_j p_j |v_j| / l,   T = the row's key count,
    eps = 2^-24 scale hd |q_i| max_j |k_j| + 2^-22 max_j |s_j| + 2^-21,
every term computed from the data."""
import json
import os

import numpy as np
import pytest
import torch

from llamarec_amd.synth import bf16_bits_to_f32, f32_to_bf16_bits, hash_uniform, synth_llama_state

pytestmark = pytest.mark.gpu

LR_EINVAL, LR_EUNSUPPORTED = -1, -2
LABELS = [17, 3, 319, 5, 200, 42, 7, 99, 100, 101, 150, 151, 152, 153, 154, 155, 156, 157, 158, 159]
CACHED = [1, 63, 64, 65, 127, 128, 129]   # one below, at and one above the 64-key block and the 128-row query tile
NEW = [1, 2, 63, 64, 65, 130]
MAX_TOKENS = 260
_MODELS = {}


def _model(golden_dir, name):
    """(LlamaRanker, 259 prompt ids, {T: whole-prompt scores of ids[:T]}), built once per name."""
    from llamarec_amd.llm import LlamaRanker

    if name not in _MODELS:
        z = np.load(os.path.join(golden_dir, "llama_tiny_hd128.npz" if name == "hd128_mqa" else f"llama_{name}.npz"))
        cfg = dict(json.loads(str(z["config"])), max_position_embeddings=512)
        if name == "hd128_mqa":
            cfg["num_key_value_heads"] = 1
        model = LlamaRanker.from_state_dict(synth_llama_state(cfg, int(z["weight_seed"])), cfg)
        ids = np.random.default_rng(11).integers(3, cfg["vocab_size"], size=259).astype(np.int32)
        ids[0] = 1
        _MODELS[name] = (model, ids, {})
    return _MODELS[name]


def _whole(entry, seq=None, T=None):
    """fp32 bits (as int32) of the whole-prompt call's scores; cached by length for the entry's own ids."""
    model, ids, memo = entry
    if seq is None:
        if T not in memo:
            memo[T] = model.prefill_verbalize([ids[:T]], LABELS)[0].cpu().numpy().view(np.int32)
        return memo[T]
    return model.prefill_verbalize([np.asarray(seq, dtype=np.int32)], LABELS)[0].cpu().numpy().view(np.int32)


def _bits(scores):
    return scores.cpu().numpy().view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit identity with the whole prompt
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_hd128", "hd128_mqa", "tiny_gqa", "tiny_hd16"])
def test_split_prompt_scores_equal_whole_prompt_bits(golden_dir, name):
    entry = _model(golden_dir, name)
    model, ids, _ = entry
    cache = model.new_prompt_cache(1, MAX_TOKENS)
    bad = []
    for q in NEW:   # c = 0: an empty slot is the plain call
        got = _bits(model.extend_verbalize(cache, [0], [ids[:q]], LABELS, keep=[0], cached_len=[0]))[0]
        if not np.array_equal(got, _whole(entry, T=q)):
            bad.append((0, q))
    for c in CACHED:
        model.extend_verbalize(cache, [0], [ids[:c]], LABELS, keep=[c], cached_len=[0])
        assert cache.ids[0] == ids[:c].tolist()
        for q in NEW:
            # keep = 0: the new rows are scratch, the slot still holds exactly the first c tokens for the next q
            got = _bits(model.extend_verbalize(cache, [0], [ids[c:c + q]], LABELS, keep=[0]))[0]
            if not np.array_equal(got, _whole(entry, T=c + q)):
                bad.append((c, q))
    assert not bad, f"{name}: (cached_len, new) pairs whose scores differ from the whole prompt's: {bad}"


# ---------------------------------------------------------------------------------------------------------------------
# 2. one call with three users
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_hd128", "hd128_mqa", "tiny_hd16"])
def test_three_prompts_in_one_call(golden_dir, name):
    entry = _model(golden_dir, name)
    model, ids, _ = entry
    rng = np.random.default_rng(5)
    vocab = model.config["vocab_size"]
    prompts = [np.concatenate([[1], rng.integers(3, vocab, size=n - 1)]).astype(np.int32) for n in (200, 131, 77)]
    cached = [65, 0, 70]
    slots = [2, 0, 1]
    cache = model.new_prompt_cache(4, MAX_TOKENS)
    cache.table.fill_(0x5A)
    for b in (0, 2):
        model.extend_verbalize(cache, [slots[b]], [prompts[b][:cached[b]]], LABELS)
    unused = cache.table[3].clone()
    got = _bits(model.extend_verbalize(cache, slots, [p[c:] for p, c in zip(prompts, cached)], LABELS))
    for b in range(3):
        assert np.array_equal(got[b], _whole(entry, seq=prompts[b])), b
        assert cache.ids[slots[b]] == prompts[b].tolist()
    assert torch.equal(cache.table[3], unused)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a chain, 4. keep and rollback
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_hd128", "tiny_gqa"])
def test_chain_of_three_extensions(golden_dir, name):
    entry = _model(golden_dir, name)
    model, ids, _ = entry
    cache = model.new_prompt_cache(2, MAX_TOKENS)
    for cut in ((0, 100), (100, 129), (129, 259)):
        chained = model.extend_verbalize(cache, [1], [ids[cut[0]:cut[1]]], LABELS)
    once = model.extend_verbalize(cache, [0], [ids], LABELS)
    assert np.array_equal(_bits(chained)[0], _bits(once)[0])
    assert np.array_equal(_bits(chained)[0], _whole(entry, T=259))


@pytest.mark.parametrize("name", ["tiny_hd128", "tiny_hd16"])
def test_keep_and_rollback(golden_dir, name):
    entry = _model(golden_dir, name)
    model, ids, _ = entry
    other = np.random.default_rng(23).integers(3, model.config["vocab_size"], size=90).astype(np.int32)
    cache = model.new_prompt_cache(1, MAX_TOKENS)
    model.extend_verbalize(cache, [0], [ids[:70]], LABELS)
    model.extend_verbalize(cache, [0], [ids[70:200]], LABELS, keep=[60])      # rows 130 .. 199 are scratch afterwards
    assert cache.ids[0] == ids[:130].tolist()
    got = _bits(model.extend_verbalize(cache, [0], [other], LABELS))[0]      # from cached_len = 70 + 60, other tokens
    assert np.array_equal(got, _whole(entry, seq=np.concatenate([ids[:130], other])))
    # roll back below what was kept and extend again
    got = _bits(model.extend_verbalize(cache, [0], [other[:33]], LABELS, cached_len=[97]))[0]
    assert np.array_equal(got, _whole(entry, seq=np.concatenate([ids[:97], other[:33]])))
    assert cache.ids[0] == np.concatenate([ids[:97], other[:33]]).tolist()
    with pytest.raises(ValueError):
        model.extend_verbalize(cache, [0], [other[:3]], LABELS, cached_len=[131])   # more than the slot holds


@pytest.mark.parametrize("name,gemm,prune", [("tiny_hd128", 1, True), ("tiny_hd128", 4, True), ("tiny_hd128", 6, True),
                                             ("tiny_hd128", 0, False), ("tiny_hd128", 1, False), ("tiny_hd16", 0, False)])
def test_identity_holds_on_the_other_routes_of_the_call(golden_dir, name, gemm, prune):
    """The call mirrors the whole-prompt path's routing: the generic GEMMs (no one-row last layer), GEMM variants 4 and 6, and
    a last layer that is not pruned (every new row attended, the last rows gathered)."""
    model, ids, _ = _model(golden_dir, name)
    try:
        model.set_variants(gemm, 0).set_last_layer_pruning(prune)
        whole = _bits(model.prefill_verbalize([ids[:195]], LABELS))[0]
        cache = model.new_prompt_cache(1, MAX_TOKENS)
        model.extend_verbalize(cache, [0], [ids[:65]], LABELS)
        got = _bits(model.extend_verbalize(cache, [0], [ids[65:195]], LABELS))[0]
    finally:
        model.set_variants(0, 0).set_last_layer_pruning(True)
    assert np.array_equal(got, whole)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the MFMA and the generic kernel agree
# ---------------------------------------------------------------------------------------------------------------------
def test_mfma_and_generic_routes_agree(golden_dir):
    """The bound is the one tests/test_gpu_llama.py puts between the MFMA and the generic kernels' scores
    (test_full_width_batch_invariance): 5e-2 * max(1, max |score|)."""
    model, ids, _ = _model(golden_dir, "tiny_hd128")
    res = []
    try:
        for variant in (0, 1):
            model.set_variants(0, variant)
            cache = model.new_prompt_cache(1, MAX_TOKENS)
            model.extend_verbalize(cache, [0], [ids[:129]], LABELS)
            res.append(model.extend_verbalize(cache, [0], [ids[129:259]], LABELS))
    finally:
        model.set_variants(0, 0)
    diff = float((res[0] - res[1]).abs().max())
    bound = 5e-2 * max(1.0, float(res[0].abs().max()))
    print(f"MFMA vs generic cached attention: max score diff {diff:.3e} (bound {bound:.3e})")
    assert torch.isfinite(res[0]).all() and torch.isfinite(res[1]).all()
    assert diff < bound


# ---------------------------------------------------------------------------------------------------------------------
# 6. lr_attention_varlen_cached alone against float64
# ---------------------------------------------------------------------------------------------------------------------
def _cached_attention_ref64(qkv, cached_len, nh, nkv, hd, offset_bug=False):
    """Rows cached_len .. T - 1 of the float64 causal attention over the whole prompt qkv [T][(nh + 2 nkv) hd]: row i of the
    new part is a softmax over cached_len + i + 1 keys. Returns (out, bound), [T - cached_len][nh hd] each. offset_bug: the
    mutant that forgets the cached rows' offset (row i sees keys 0 .. i)."""
    x = np.asarray(qkv, dtype=np.float64)
    T = x.shape[0]
    q = x[:, : nh * hd].reshape(T, nh, hd)
    k = x[:, nh * hd: (nh + nkv) * hd].reshape(T, nkv, hd)
    v = x[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    scale = 1.0 / np.sqrt(hd)
    rows = np.arange(cached_len, T)
    seen = rows - cached_len if offset_bug else rows
    keep = np.arange(T)[None, :] <= seen[:, None]
    out = np.zeros((T - cached_len, nh * hd))
    bound = np.zeros_like(out)
    for h in range(nh):
        g = h // (nh // nkv)
        sc = np.where(keep, (q[rows, h] @ k[:, g].T) * scale, -np.inf)
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        l = p.sum(axis=1, keepdims=True)
        o = (p @ v[:, g]) / l
        S = (p @ np.abs(v[:, g])) / l
        kn = np.linalg.norm(k[:, g], axis=1)
        kmax = np.where(keep, kn[None, :], 0.0).max(axis=1)
        smax = np.where(keep, np.abs(sc), 0.0).max(axis=1)
        eps = 2.0 ** -24 * scale * hd * np.linalg.norm(q[rows, h], axis=1) * kmax + 2.0 ** -22 * smax + 2.0 ** -21
        cols = slice(h * hd, (h + 1) * hd)
        out[:, cols] = o
        bound[:, cols] = 2.0 ** -8 * np.abs(o) + (2.0 ** -8 + (seen + 1)[:, None] * 2.0 ** -24 + 2 * eps[:, None]) * S
    return out, bound


# (cached_len, new rows): every boundary length of test 1 on one side or the other, and an empty slot
SEGMENTS = [(1, 130), (63, 2), (64, 64), (65, 63), (127, 65), (128, 1), (129, 130), (0, 65)]
SEG_SLOTS = [7, 2, 9, 0, 4, 5, 1, 8]   # of 10: slots 3 and 6 stay unused


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 1)])
def test_cached_attention_within_float64_bound(nh, nkv, variant):
    from llamarec_amd._lib import lib, stream_ptr

    hd, num_slots, max_tokens, num_layers, layer = 128, 10, 261, 2, 1
    kv_w, q_w = 2 * nkv * hd, nh * hd
    L = lib()
    slot_bytes = L.lr_llama_kv_cache_slot_bytes(num_layers, nkv, hd, max_tokens)
    assert slot_bytes >= num_layers * max_tokens * kv_w * 2 and slot_bytes % 256 == 0
    # a table of finite, recognisable bf16 garbage (7.0): a key read past a prompt's end would move the result
    table = np.full((num_slots, slot_bytes // 2), 0x40E0, np.uint16)
    prompts, refs, new_rows = [], [], []
    for s, (c, qn) in enumerate(SEGMENTS):
        x = hash_uniform(400 + 10 * s + nkv, (c + qn, q_w + kv_w), 1.0)
        x = bf16_bits_to_f32(f32_to_bf16_bits(x))
        prompts.append(x)
        refs.append(_cached_attention_ref64(x, c, nh, nkv, hd))
        new_rows.append(x[c:])
        lay = table[SEG_SLOTS[s]][layer * max_tokens * kv_w: (layer + 1) * max_tokens * kv_w].reshape(max_tokens, kv_w)
        lay[:c] = f32_to_bf16_bits(x[:c, q_w:])
    before = table.copy()
    cu = np.concatenate([[0], np.cumsum([qn for _, qn in SEGMENTS])]).astype(np.int32)
    cl = np.array([c for c, _ in SEGMENTS], np.int32)
    sl = np.array(SEG_SLOTS, np.int32)
    n = int(cu[-1])
    qkv_d = torch.from_numpy(f32_to_bf16_bits(np.concatenate(new_rows)).view(np.int16)).cuda()
    table_d = torch.from_numpy(table.view(np.int16)).cuda()
    out_d = torch.full((n, q_w), 0x7FC0, dtype=torch.int16, device="cuda")
    cu_d, cl_d, sl_d = (torch.from_numpy(a).cuda() for a in (cu, cl, sl))
    rc = L.lr_attention_varlen_cached(qkv_d.data_ptr(), out_d.data_ptr(), table_d.data_ptr(), num_slots, max_tokens, num_layers,
                                      layer, sl_d.data_ptr(), sl.ctypes.data, cl_d.data_ptr(), cl.ctypes.data, cu_d.data_ptr(),
                                      cu.ctypes.data, len(SEGMENTS), nh, nkv, hd, variant, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.lr_last_error()
    got = bf16_bits_to_f32(out_d.cpu().numpy().view(np.uint16)).astype(np.float64)
    worst = 0.0
    for s, (c, qn) in enumerate(SEGMENTS):
        ref, bound = refs[s]
        g = got[cu[s]: cu[s + 1]]
        assert np.isfinite(g).all(), (s, c, qn)
        worst = max(worst, float((np.abs(g - ref) / bound).max()))
    mut, _ = _cached_attention_ref64(prompts[0], SEGMENTS[0][0], nh, nkv, hd, offset_bug=True)
    mutant = float((np.abs(mut - refs[0][0]) / refs[0][1]).max())
    print(f"cached attention nh={nh} nkv={nkv} variant {variant}: err/bound {worst:.3f}; offset mutant {mutant:.1f} x bound")
    assert worst <= 1.0
    assert mutant > 1.0
    # the table: the call's own rows hold its K | V, every other byte is what it was
    after = table_d.cpu().numpy().view(np.uint16)
    want = before.copy()
    for s, (c, qn) in enumerate(SEGMENTS):
        lay = want[SEG_SLOTS[s]][layer * max_tokens * kv_w: (layer + 1) * max_tokens * kv_w].reshape(max_tokens, kv_w)
        lay[c: c + qn] = f32_to_bf16_bits(prompts[s][c:, q_w:])
    assert np.array_equal(after, want)


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals, all before any launch
# ---------------------------------------------------------------------------------------------------------------------
def _raw_extend(model, table, num_slots, slots, cached_len, seqs, keep, out, max_tokens=MAX_TOKENS, table_ptr=None):
    from llamarec_amd._lib import lib, stream_ptr

    B = len(slots)
    sl, cl, kp = (np.asarray(a, np.int32) for a in (slots, cached_len, keep))
    cu = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    ids = np.concatenate([np.asarray(s, np.int32) for s in seqs] + [np.zeros(1, np.int32)])
    sl_d, cl_d, cu_d, ids_d = (torch.from_numpy(a).cuda() for a in (sl, cl, cu, ids))
    lab = torch.tensor(LABELS, dtype=torch.int32, device="cuda")
    L = lib()
    need = L.lr_llama_extend_workspace_bytes(model._h, max(int(cu[-1]), 1), B, max_tokens)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.lr_llama_extend_verbalize(model._h, table.data_ptr() if table_ptr is None else table_ptr, num_slots, max_tokens,
                                     sl_d.data_ptr(), sl.ctypes.data, cl_d.data_ptr(), cl.ctypes.data, ids_d.data_ptr(),
                                     cu_d.data_ptr(), cu.ctypes.data, kp.ctypes.data, B, lab.data_ptr(), len(LABELS),
                                     out.data_ptr(), ws.data_ptr(), need, stream_ptr())
    torch.cuda.synchronize()
    return rc, L.lr_last_error().decode()


def test_refusals_leave_scores_and_table_untouched(golden_dir):
    from llamarec_amd._lib import lib

    model, ids, _ = _model(golden_dir, "tiny_hd128")
    cache = model.new_prompt_cache(3, MAX_TOKENS)
    cache.table.fill_(0x3C)
    table0 = cache.table.clone()
    out = torch.full((2, len(LABELS)), -123.0, device="cuda")
    out0 = out.clone()
    a, b = ids[:5], ids[5:12]
    cases = {
        "duplicate slot": dict(slots=[1, 1], cached_len=[0, 0], seqs=[a, b], keep=[5, 7]),
        "slot out of range": dict(slots=[0, 3], cached_len=[0, 0], seqs=[a, b], keep=[5, 7]),
        "negative slot": dict(slots=[-1, 2], cached_len=[0, 0], seqs=[a, b], keep=[5, 7]),
        "overflow of max_tokens": dict(slots=[0, 1], cached_len=[0, MAX_TOKENS - 6], seqs=[a, b], keep=[5, 7]),
        "keep > q_len": dict(slots=[0, 1], cached_len=[0, 0], seqs=[a, b], keep=[6, 7]),
        "negative keep": dict(slots=[0, 1], cached_len=[0, 0], seqs=[a, b], keep=[5, -1]),
        "empty new part": dict(slots=[0, 1], cached_len=[4, 0], seqs=[a[:0], b], keep=[0, 7]),
        "negative cached_len": dict(slots=[0, 1], cached_len=[-1, 0], seqs=[a, b], keep=[5, 7]),
        "misaligned table": dict(slots=[0, 1], cached_len=[0, 0], seqs=[a, b], keep=[5, 7], table_ptr=cache.table.data_ptr() + 2),
        "null table": dict(slots=[0, 1], cached_len=[0, 0], seqs=[a, b], keep=[5, 7], table_ptr=0),
    }
    for what, kw in cases.items():
        rc, msg = _raw_extend(model, cache.table, 3, out=out, **kw)
        assert rc == LR_EINVAL and msg, (what, rc, msg)
        assert torch.equal(out, out0) and torch.equal(cache.table, table0), what
    # beyond max_positions (512 here) although the slot would hold it
    big = model.new_prompt_cache(1, 600)
    rc, msg = _raw_extend(model, big.table, 1, [0], [510], [a], [5], out, max_tokens=600)
    assert rc == LR_EINVAL and "max_positions" in msg
    # a handle with q/k/v biases has no cached form
    c = model.config
    Lyr, width = c["num_hidden_layers"], (c["num_attention_heads"] + 2 * c["num_key_value_heads"]) * model.hd
    biases = [torch.zeros(width, dtype=torch.bfloat16, device="cuda") for _ in range(Lyr)]
    import ctypes
    arr = (ctypes.c_void_p * Lyr)(*[t.data_ptr() for t in biases])
    assert lib().lr_llama_set_qkv_bias(model._h, arr) == 0
    try:
        rc, msg = _raw_extend(model, cache.table, 3, [0, 1], [0, 0], [a, b], [5, 7], out)
    finally:
        assert lib().lr_llama_set_qkv_bias(model._h, None) == 0
    assert rc == LR_EUNSUPPORTED and "bias" in msg
    assert torch.equal(out, out0) and torch.equal(cache.table, table0)
    # and the same arguments, accepted, do write
    rc, msg = _raw_extend(model, cache.table, 3, [0, 1], [0, 0], [a, b], [5, 7], out)
    assert rc == 0, msg
    assert not torch.equal(out, out0) and not torch.equal(cache.table, table0) and torch.equal(cache.table[2], table0[2])


# ---------------------------------------------------------------------------------------------------------------------
# 8. RankerSession.rank against rank_candidates
# ---------------------------------------------------------------------------------------------------------------------
def test_ranker_session_matches_rank_candidates():
    from llamarec_amd import data as D
    from llamarec_amd import inference as I
    from llamarec_amd.llm import LlamaRanker
    from llamarec_amd.verb import ManualVerbalizer
    from tests.fake_tokenizer import FakeTokenizer

    ds = D.synthetic_dataset(num_users=5, num_items=400, seed=3)
    tok = FakeTokenizer()
    cfg = dict(vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
               num_key_value_heads=2, max_position_embeddings=2048, rms_norm_eps=1e-5, rope_theta=10000.0)
    ranker = LlamaRanker.from_state_dict(synth_llama_state(cfg, 11), cfg)
    verb = ManualVerbalizer(tokenizer=tok, classes=list(range(20)), label_words={i: chr(65 + i) for i in range(20)})
    items = ds["train"][1]
    history, more = list(items[-8:-1]), list(items[-8:])
    pool = [int(i) for i in range(30, 50)]
    pool2 = [int(i) for i in range(120, 140)]
    session = I.RankerSession(ranker, tok, verb, max_tokens=2048)
    sent = []
    for query, cands in ((history, pool), (more, pool), (more, pool2)):
        prompt = I.generate_prompt(query, cands, ds["meta"])
        n_ids = len(tok(prompt)["input_ids"])
        assert session.rank(prompt, cands, top_k=10) == I.rank_candidates(ranker, tok, prompt, cands, verb, top_k=10)
        sent.append((session.last_sent, n_ids))
    print(f"tokens sent / prompt tokens per call: {sent}")
    assert sent[0][0] == sent[0][1]
    assert 0 < sent[1][0] < sent[1][1] and 0 < sent[2][0] < sent[2][1]
    assert session.sent_tokens == sum(s for s, _ in sent)
    short = I.RankerSession(ranker, tok, verb, max_tokens=16)
    with pytest.raises(ValueError):
        short.rank(I.generate_prompt(history, pool, ds["meta"]), pool)
