"""GPU parity for LRURec user states: a state that was reset and then advanced by any chunking of a history, in any batch,
through any slot, gives the bits of the CPU oracle on the whole history (last hidden state, top-K ids and scores).
Every expected value comes from oracle.lru_oracle -- the reference, not the product."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_lru import _big_case

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _history(ids):
    """What a state has seen of these rows: the ids >= 1, left padded to the same width. The contract speaks of such
    histories. For a left-padded row this is the row itself; the one golden row that is not (L50, row 4, ends in a pad
    id: the encoder embeds a pad at the LAST position as a token, the state skips it) is compared on its live ids."""
    return _concat_live(ids, ids[:, :0])


@pytest.fixture(scope="module")
def env(golden_dir):
    from llamarec_amd.lru import LRURec
    from oracle import lru_oracle as O

    z = np.load(os.path.join(golden_dir, "lru_v300.npz"))
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    return z, sd, LRURec.from_state_dict(sd), O.LruOracle(sd), O


@pytest.fixture(scope="module")
def pool(env):
    """64 left-padded histories of 1..12 ids over the golden model's catalog and their oracle states: after the first 5
    columns (`q5`, zeros where a user has not started) and after all 12 (`q`). Shared, never changed."""
    _, _, _, orc, _ = env
    rng = np.random.default_rng(7)
    U, L = 64, 12
    ids = np.zeros((U, L), np.int64)
    for u in range(U):
        n = int(rng.integers(1, L + 1)) if u else L   # user 0 has a full row
        ids[u, L - n:] = rng.integers(1, 301, size=n)
    q = orc.encode_last(ids)
    q5 = orc.encode_last(ids[:, :5])
    q5[~(ids[:, :5] > 0).any(1)] = 0.0   # a never-advanced row answers zeros
    q.setflags(write=False), q5.setflags(write=False)
    return ids, q5, q


def _concat_live(a, b):
    """Row-wise concatenation of two left-padded id matrices as ONE left-padded history (the pads of b are skipped)."""
    out = np.zeros((a.shape[0], a.shape[1] + b.shape[1]), np.int64)
    for u in range(a.shape[0]):
        live = np.concatenate([a[u][a[u] > 0], b[u][b[u] > 0]])
        out[u, out.shape[1] - len(live):] = live
    return out


def _check_started(q, ids_so_far, orc):
    """q rows of the users that have consumed an id equal the oracle on the prefix; the others are still zero."""
    started = (ids_so_far > 0).any(1)
    want = orc.encode_last(_history(ids_so_far))
    assert np.array_equal(_bits(q[started]), _bits(want[started]))
    assert not q[~started].any()
    return started


@pytest.mark.parametrize("case", ["L7", "L50", "L64", "L200"])
def test_column_by_column(env, case):
    """One column of the id matrix per call: users whose prefix is still all pad exercise the skip rule."""
    z, _, model, orc, _ = env
    ids = z[f"ids/{case}"]
    B, L = ids.shape
    checks = set(range(1, L + 1)) if L <= 64 else set(np.linspace(1, L, 14).round().astype(int).tolist())
    assert {1, L} <= checks and len(checks) >= min(12, L)
    st = model.new_user_states(B)
    dev = torch.from_numpy(ids).to(model.device)
    prev, prev_t = None, 0
    for t in range(1, L + 1):
        q = model.advance(st, dev[:, t - 1:t])
        if t not in checks:
            continue
        q = _np(q)
        _check_started(q, ids[:, :t], orc)
        if prev is not None:   # the comparison is not vacuous: whoever consumed an id since the last check moved
            moved = (ids[:, prev_t:t] > 0).any(1)
            assert moved.any()
            assert all(not np.array_equal(prev[u], q[u]) for u in np.nonzero(moved)[0])
        prev, prev_t = q, t
    assert prev_t == L


@pytest.mark.parametrize("case", ["L7", "L50", "L64", "L200"])
def test_chunks(env, case):
    """Chunks of 1, 15, 16, 17 columns and the rest."""
    z, _, model, orc, _ = env
    ids = z[f"ids/{case}"]
    B, L = ids.shape
    st = model.new_user_states(B)
    t, prev = 0, None
    for n in (1, 15, 16, 17, L):
        n = min(n, L - t)
        if n == 0:
            break
        q = _np(model.advance(st, ids[:, t:t + n]))
        t += n
        _check_started(q, ids[:, :t], orc)
        if prev is not None:   # whoever consumed an id in this chunk moved
            moved = np.nonzero((ids[:, t - n:t] > 0).any(1))[0]
            assert len(moved) and all(not np.array_equal(prev[u], q[u]) for u in moved)
        prev = q
    assert t == L


@pytest.mark.parametrize("nb", [1, 3])
def test_block_counts(nb):
    from llamarec_amd.lru import LRURec
    from oracle import lru_oracle as O

    sd, ids = _big_case(500, 20, 30, seed=nb, nb=nb)
    model, orc = LRURec.from_state_dict(sd), O.LruOracle(sd)
    want = orc.encode_last(ids)
    st = model.new_user_states(20)
    assert st.table.shape[1] == nb * 1024 + 512
    assert np.array_equal(_bits(_np(model.advance(st, ids))), _bits(want))          # the whole history in one call
    st2 = model.new_user_states(20)
    for t in range(30):
        q = model.advance(st2, ids[:, t:t + 1])
    assert np.array_equal(_bits(_np(q)), _bits(want))                               # one id per call
    assert torch.equal(st.table, st2.table)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 37])
def test_batch_shapes_and_independence(env, pool, B):
    """A user's row bytes and q are the same in a batch, through permuted slots, and alone."""
    _, _, model, _, _ = env
    ids, q5, q12 = pool
    st = model.new_user_states(B)
    assert np.array_equal(_bits(_np(model.advance(st, ids[:B, :5]))), _bits(q5[:B]))
    assert np.array_equal(_bits(_np(model.advance(st, ids[:B, 5:]))), _bits(q12[:B]))
    rows = st.numpy()

    perm = np.random.default_rng(B).permutation(40)[:B].astype(np.int32)
    sp = model.new_user_states(40)
    model.advance(sp, ids[:B, :5], slots=perm)
    qp = _np(model.advance(sp, ids[:B, 5:], slots=perm))
    assert np.array_equal(_bits(qp), _bits(q12[:B]))
    assert np.array_equal(sp.numpy()[perm], rows)
    untouched = np.setdiff1d(np.arange(40), perm)
    assert not sp.numpy()[untouched].any()

    for u in sorted({0, B // 2, B - 1}):
        s1 = model.new_user_states(1)
        model.advance(s1, ids[u:u + 1, :5])
        q1 = _np(model.advance(s1, ids[u:u + 1, 5:]))
        assert np.array_equal(_bits(q1[0]), _bits(q12[u]))
        assert np.array_equal(s1.numpy()[0], rows[u])


def test_slots_interleaved_zero_rows_and_reset(env, pool):
    from llamarec_amd.lru import UserStates

    _, _, model, orc, _ = env
    ids, q5, q12 = pool
    a = np.array([3, 10, 17, 40, 63], np.int32)          # users 0..4
    b = np.array([0, 5, 11, 41, 62, 20], np.int32)       # users 5..10
    ua, ub = np.arange(5), np.arange(5, 11)
    table = torch.full((64, lib_row_bytes(model)), 0xAB, dtype=torch.uint8, device=model.device)
    st = UserStates(table)
    table[torch.from_numpy(a).long().to(model.device)] = 0   # a zero-filled row ...
    model.reset_user_states(st, b)                           # ... behaves as a reset one
    before = st.numpy()
    assert not before[a].any() and not before[b].any()

    model.advance(st, ids[ua, :5], slots=a)
    model.advance(st, ids[ub, :5], slots=b)
    qa = _np(model.advance(st, ids[ua, 5:], slots=a))
    qb = _np(model.advance(st, ids[ub, 5:], slots=b))
    assert np.array_equal(_bits(qa), _bits(q12[ua]))
    assert np.array_equal(_bits(qb), _bits(q12[ub]))
    after = st.numpy()
    untouched = np.setdiff1d(np.arange(64), np.concatenate([a, b]))
    assert np.array_equal(after[untouched], before[untouched]) and (after[untouched] == 0xAB).all()

    # reset a subset: their next advance is a fresh user's; the others go on with their history
    model.reset_user_states(st, a[:2])
    assert not st.numpy()[a[:2]].any() and np.array_equal(st.numpy()[a[2:]], after[a[2:]])
    nxt = ids[20:25]
    q = _np(model.advance(st, nxt, slots=a))
    want_fresh = orc.encode_last(nxt[:2])
    want_cont = orc.encode_last(_concat_live(ids[ua[2:]], nxt[2:]))
    assert np.array_equal(_bits(q[:2]), _bits(want_fresh))
    assert np.array_equal(_bits(q[2:]), _bits(want_cont))
    assert np.array_equal(st.numpy()[b], after[b])


def lib_row_bytes(model):
    from llamarec_amd._lib import lib

    return int(lib().lr_lru_user_state_row_bytes(model.num_blocks))


def test_slot_guard(env, pool):
    """Slots outside [0, num_slots) are skipped. The allocation has 8 rows and the call is told of 4, so a missing guard
    shows as a failed comparison, never as a write outside the allocation."""
    from llamarec_amd.lru import UserStates

    _, _, model, _, _ = env
    ids, _, q12 = pool
    table = torch.zeros((8, lib_row_bytes(model)), dtype=torch.uint8, device=model.device)
    table[4:] = 0xCD
    st = UserStates(table[:4])
    assert st.num_slots == 4 and st.table.data_ptr() == table.data_ptr()
    slots = np.array([0, -1, 2, 5, 3], np.int32)
    q = _np(model.advance(st, ids[:5], slots=slots))
    ok = np.array([0, 2, 4])
    assert np.array_equal(_bits(q[ok]), _bits(q12[ok]))
    assert not q[[1, 3]].any()
    full = table.cpu().numpy()
    assert (full[4:] == 0xCD).all()
    assert not full[1].any()                       # slot 1 was never named
    ref = model.new_user_states(4)
    model.advance(ref, ids[ok], slots=np.array([0, 2, 3], np.int32))
    assert np.array_equal(full[:4], ref.numpy())   # the other users are unaffected
    idx, _ = model.retrieve_topk_from_states(st, 5, slots=slots)   # the same guard in the query-only call
    want, _ = model.retrieve_topk_from_states(ref, 5, slots=np.array([0, 2, 3], np.int32))
    assert torch.equal(idx[torch.from_numpy(ok).to(idx.device)], want)
    assert np.array_equal(table.cpu().numpy(), full)


def test_persistence(env, pool):
    """Table -> host -> a new table: the continuation equals the uninterrupted run, rows and q."""
    _, _, model, _, _ = env
    ids, q5, q12 = pool
    st = model.new_user_states(37)
    assert np.array_equal(_bits(_np(model.advance(st, ids[:37, :5]))), _bits(q5[:37]))
    saved = st.numpy().copy()
    st2 = model.load_user_states(saved)
    assert st2.table.data_ptr() != st.table.data_ptr()
    q_a = _np(model.advance(st, ids[:37, 5:]))
    q_b = _np(model.advance(st2, ids[:37, 5:]))
    assert np.array_equal(_bits(q_a), _bits(q12[:37])) and np.array_equal(_bits(q_b), _bits(q12[:37]))
    assert np.array_equal(st.numpy(), st2.numpy())
    assert not np.array_equal(saved, st.numpy())
    # a user with no id in the call keeps its state and answers its stored q
    q_c = _np(model.advance(st2, np.zeros((37, 3), np.int64)))
    assert np.array_equal(_bits(q_c), _bits(q12[:37])) and np.array_equal(st.numpy(), st2.numpy())


def _topk_case(model, orc, O, sd, ids, K, excl):
    """Whole history but the last column by `advance`, the last column in the retrieving call, then a query-only call."""
    B, L = ids.shape
    st = model.new_user_states(B)
    model.advance(st, ids[:, :-1])
    ex = ids if excl else None
    idx, sc = model.retrieve_topk_from_states(st, K, new_ids=ids[:, -1:], exclude=ex)
    idx, sc = _np(idx), _np(sc)
    oi, os_ = orc.retrieve_topk(_history(ids), K, excl)
    started = (ids > 0).any(1)
    if not started.all():   # no history: q = 0, so a score is the item's bias (and the pad id is masked with the history)
        s = np.repeat(np.asarray(sd["model.bias"], np.float32)[None], int((~started).sum()), axis=0)
        if excl:
            s[:, 0] = -1e9
        oi[~started], os_[~started] = O.topk(s, K)
    assert np.array_equal(idx, oi)
    assert np.array_equal(_bits(sc), _bits(os_))
    idx2, sc2 = model.retrieve_topk_from_states(st, K, exclude=ex)   # query only: Ln = 0
    assert np.array_equal(_np(idx2), idx) and np.array_equal(_bits(_np(sc2)), _bits(sc))


@pytest.mark.parametrize("case,K,excl", [("L50", 20, True), ("L50", 50, True), ("L200", 50, True), ("L50", 1, True),
                                         ("L7", 20, False)])
def test_topk_from_states(env, case, K, excl):
    z, sd, model, orc, O = env
    _topk_case(model, orc, O, sd, z[f"ids/{case}"], K, excl)


@pytest.mark.parametrize("V,B,L,K", [(33, 9, 50, 50), (12086, 300, 50, 50)])
def test_topk_from_states_larger_shapes(V, B, L, K):
    """A catalog smaller than K + history (masked -1e9 entries surface, ties by id) and one many-chunk case."""
    from llamarec_amd.lru import LRURec
    from oracle import lru_oracle as O

    sd, ids = _big_case(V, B, L, seed=V + B)
    _topk_case(LRURec.from_state_dict(sd), O.LruOracle(sd), O, sd, ids, K, True)


def test_retriever_session(env):
    from llamarec_amd.inference import RetrieverSession, retrieve_candidates

    _, _, model, orc, _ = env
    items = np.random.default_rng(3).integers(1, 301, size=5)
    s = RetrieverSession(model)
    s.append(items[:1])
    first = s.candidates(20)
    s.append(items[1:4])
    s.append(int(items[4]))
    got = s.candidates(20)
    assert s.query == items.tolist()
    assert got == retrieve_candidates(model, items, 20)
    assert got == orc.retrieve_topk(items.reshape(1, -1), 20, False)[0][0].tolist()
    assert first == orc.retrieve_topk(items[:1].reshape(1, -1), 20, False)[0][0].tolist() and first != got
