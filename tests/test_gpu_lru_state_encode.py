"""GPU parity for LRURec user states seeded from whole histories by the encoder pass (`LRURec.encode_states`,
`retrieve_topk(..., states=)`, `RetrieverSession(model, history=)`): the q returned, the table bytes left behind and
everything later computed from them. Every expected q / top-K comes from oracle.lru_oracle on the concatenated history;
expected table bytes come from reset + `advance` of the same ids, which tests/test_gpu_lru_state.py holds to the oracle.
All comparisons are on bits."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_lru import _big_case
from tests.test_gpu_lru_state import _bits, _concat_live

pytestmark = pytest.mark.gpu

GOLDEN = ["L7", "L50", "L64", "L200"]   # live lengths 7/7/2/5, 10/1/0/50/48/3/25/50, 64/33/32/1, 200/100/129/17
SEAMS = [15, 1, 16, 32, 63, 1, 64, 65, 3, 3, 3, 3, 3, 3, 130]
# lr_lru_workspace_bytes(golden model, users, K, L) as the commit BEFORE the seeding calls returns it (computed once there,
# pinned here): the existing workspace layout must not move
PARENT_WS_4096_50_200 = 432325888
PARENT_WS_1_1_7 = 1049088
EINVAL, EWORKSPACE = -1, -4


def _np(t):
    return t.cpu().numpy()


def _apart(ids):
    """Rows that end in a pad id but have live ids: outside the states' contract (the encoder embeds the last pad as a
    token, a state skips it), their table row is written as the reset state. The all-pad row ends in a pad too, but the
    reset row it gets IS what reset + advance of its (no) live ids leaves, so it follows the general rule."""
    return (ids[:, -1] <= 0) & (ids > 0).any(1)


def _cut(ids):
    """What the encoder processes of each row (em_live_kernel): the ids behind the last id <= 0 among the first L-1."""
    out = ids.copy()
    for u in range(ids.shape[0]):
        pads = np.nonzero(ids[u, :-1] <= 0)[0]
        if len(pads):
            out[u, :pads[-1] + 1] = 0
    return out


def _seen(ids):
    """The history a seeded state stands for: the cut ids, nothing for the rows treated apart."""
    h = _cut(ids)
    h[ids[:, -1] <= 0] = 0
    return h


def _advance_table(model, ids, num_slots=None, slots=None):
    """The table reset + advance of what the state stands for leaves, on the host."""
    st = model.new_user_states(num_slots or ids.shape[0])
    model.advance(st, _seen(ids), slots=slots)
    return st.numpy()


def _draw_new(rng, B, n, V=300):
    """[B, n] new ids in 1..V, a different count (1..n) per user, left padded; user 0 gets all n."""
    new = np.zeros((B, n), np.int64)
    for u in range(B):
        k = n if u == 0 else int(rng.integers(1, n + 1))
        new[u, n - k:] = rng.integers(1, V + 1, size=k)
    return new


def _continue_and_check(model, orc, st, hist, rng, counts=(1, 16, 17), V=300, slots=None):
    for n in counts:
        new = _draw_new(rng, hist.shape[0], n, V)
        q = _np(model.advance(st, new, slots=slots))
        hist = _concat_live(hist, new)
        assert np.array_equal(_bits(q), _bits(orc.encode_last(hist))), n
    return hist


@pytest.fixture(scope="module")
def env(golden_dir):
    from llamarec_amd.lru import LRURec
    from oracle import lru_oracle as O

    z = np.load(os.path.join(golden_dir, "lru_v300.npz"))
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    return z, sd, LRURec.from_state_dict(sd), O.LruOracle(sd), O


@pytest.fixture(scope="module")
def seams():
    """One batch at L = 130 whose live lengths put users' last rows at tile rows 15 / 31 / 63, a user at row 0 of a tile,
    a user through the carry, six users inside one wave's segment, and segment cuts at rows 16 / 32 / 48."""
    rng = np.random.default_rng(130)
    ids = np.zeros((len(SEAMS), 130), np.int64)
    for u, n in enumerate(SEAMS):
        ids[u, 130 - n:] = rng.integers(1, 301, size=n)
    ids.setflags(write=False)
    return ids


# ---- 1. golden cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN)
def test_golden_cases(env, case):
    z, _, model, orc, _ = env
    ids = z[f"ids/{case}"]
    B = ids.shape[0]
    apart = _apart(ids)
    assert int(apart.sum()) == (1 if case == "L50" else 0)
    if case == "L50":
        assert apart[4]
    st = model.new_user_states(B)
    q = _np(model.encode_states(st, ids))
    assert np.array_equal(_bits(q), _bits(_np(model.encode_last(ids))))
    assert np.array_equal(_bits(q), _bits(orc.encode_last(ids)))      # the apart row's out_q is the encoder's too
    rows = st.numpy()
    assert not rows[apart].any()
    live = (ids > 0).any(1) & ~apart
    assert all(rows[u].any() for u in np.nonzero(live)[0])
    _continue_and_check(model, orc, st, _seen(ids), np.random.default_rng(1))


# ---- 2. bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN)
def test_bytes_golden(env, case):
    z, _, model, _, _ = env
    ids = z[f"ids/{case}"]
    st = model.new_user_states(ids.shape[0])
    model.encode_states(st, ids)
    got, want = st.numpy(), _advance_table(model, ids)
    assert not got[_apart(ids)].any()
    _assert_same_rows(got, want, model.num_blocks)


def _assert_same_rows(got, want, nb):
    """Byte equality, with the first differing (user, block, re/im, channel) or field in the message."""
    if np.array_equal(got, want):
        return
    u, o = [int(v[0]) for v in np.nonzero(got != want)]
    f = o // 4
    where = (f"block {f // 256} {'re' if f % 256 < 128 else 'im'} channel {f % 128}" if f < nb * 256 else
             f"q[{f - nb * 256}]" if f < nb * 256 + 64 else "live" if f == nb * 256 + 64 else "padding")
    raise AssertionError(f"user {u}: {where} (byte {o}) differs; {int((got != want).any(1).sum())} rows differ")


def test_bytes_pool(env):
    """tests/test_gpu_lru_state.py's pool shape: 64 users of 1..12 ids."""
    _, _, model, _, _ = env
    rng = np.random.default_rng(7)
    ids = np.zeros((64, 12), np.int64)
    for u in range(64):
        n = int(rng.integers(1, 13)) if u else 12
        ids[u, 12 - n:] = rng.integers(1, 301, size=n)
    st = model.new_user_states(64)
    model.encode_states(st, ids)
    _assert_same_rows(st.numpy(), _advance_table(model, ids), model.num_blocks)


# ---- 3. tile seams -------------------------------------------------------------------------------------------------------
def test_tile_seams_both_kernels(env, seams):
    _, _, model, orc, _ = env
    ids = np.array(seams)
    want_q, want_rows = orc.encode_last(ids), _advance_table(model, ids)
    tables = []
    try:
        for pipe in (True, False):
            model.set_encoder_pipeline(pipe)
            st = model.new_user_states(len(SEAMS))
            q = _np(model.encode_states(st, ids))
            assert np.array_equal(_bits(q), _bits(want_q)), pipe
            _assert_same_rows(st.numpy(), want_rows, model.num_blocks)
            tables.append(st.numpy())
            _continue_and_check(model, orc, st, ids, np.random.default_rng(2), counts=(1, 17))
    finally:
        model.set_encoder_pipeline(True)
    assert np.array_equal(tables[0], tables[1])


# ---- 4. block counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3])
def test_block_counts(nb):
    from llamarec_amd._lib import lib
    from llamarec_amd.lru import LRURec
    from oracle import lru_oracle as O

    sd, ids = _big_case(500, 20, 30, seed=nb, nb=nb)
    model, orc = LRURec.from_state_dict(sd), O.LruOracle(sd)
    base = lib().lr_lru_workspace_bytes(model._h, 20, 1, 30)
    assert lib().lr_lru_user_state_encode_workspace_bytes(model._h, 20, 1, 30) == base + (nb - 1) * 20 * 1024
    for pipe in (True, False):
        model.set_encoder_pipeline(pipe)
        st = model.new_user_states(20)
        assert st.table.shape[1] == nb * 1024 + 512
        q = _np(model.encode_states(st, ids))
        assert np.array_equal(_bits(q), _bits(orc.encode_last(ids)))
        _assert_same_rows(st.numpy(), _advance_table(model, ids), nb)
        _continue_and_check(model, orc, st, ids, np.random.default_rng(nb), counts=(1, 5), V=500)
    model.set_encoder_pipeline(True)


# ---- 5. cut and overwrite ------------------------------------------------------------------------------------------------
def test_cut_and_overwrite(env):
    _, _, model, orc, _ = env
    rng = np.random.default_rng(5)
    ids = rng.integers(1, 301, size=(6, 40)).astype(np.int64)
    ids[0, 17] = 0            # a pad in the middle cuts: the state is that of ids[0, 18:]
    ids[1, :9] = 0            # plain left padding
    ids[2, 3] = ids[2, 30] = 0   # two pads: the last one cuts
    ids[3, 38] = 0            # one live id behind the cut
    ids[4, 11] = -7           # a negative id cuts like a pad
    st = model.new_user_states(6)
    q = _np(model.encode_states(st, ids))
    assert np.array_equal(_bits(q), _bits(orc.encode_last(ids)))
    behind = _cut(ids)
    assert (behind[0, :18] == 0).all() and (behind[0, 18:] > 0).all() and (behind[3] > 0).sum() == 1
    assert np.array_equal(_bits(q), _bits(orc.encode_last(behind)))   # the encoder's cut is the oracle's
    _assert_same_rows(st.numpy(), _advance_table(model, ids), model.num_blocks)
    hist = _continue_and_check(model, orc, st, behind, rng, counts=(1, 3))

    # seed the advanced rows again with other histories: no trace of the first
    other = rng.integers(1, 301, size=(6, 23)).astype(np.int64)
    other[5, :22] = 0
    assert not np.array_equal(st.numpy(), _advance_table(model, other))
    q2 = _np(model.encode_states(st, other))
    assert np.array_equal(_bits(q2), _bits(orc.encode_last(other)))
    fresh = model.new_user_states(6)
    model.encode_states(fresh, other)
    assert np.array_equal(st.numpy(), fresh.numpy())
    _assert_same_rows(st.numpy(), _advance_table(model, other), model.num_blocks)
    assert hist.shape[1] == 44


# ---- 6. slots ------------------------------------------------------------------------------------------------------------
def test_slots_and_guard(env):
    """The allocation has 48 rows and the call is told of 40, so a missing guard shows as a failed comparison, never as a
    write outside the allocation."""
    from llamarec_amd.lru import UserStates

    z, _, model, orc, _ = env
    rng = np.random.default_rng(6)
    B, L, n_slots = 12, 20, 40
    ids = np.zeros((B, L), np.int64)
    for u in range(B):
        n = int(rng.integers(1, L + 1))
        ids[u, L - n:] = rng.integers(1, 301, size=n)
    slots = rng.permutation(n_slots)[:B].astype(np.int32)
    slots[3], slots[8] = -1, n_slots
    ok = np.array([u for u in range(B) if u not in (3, 8)])
    table = torch.full((48, model.new_user_states(1).table.shape[1]), 0xAB, dtype=torch.uint8, device=model.device)
    st = UserStates(table[:n_slots])
    q = _np(model.encode_states(st, ids, slots=slots))
    assert np.array_equal(_bits(q), _bits(orc.encode_last(ids)))          # out-of-range users' rows included
    full = table.cpu().numpy()
    untouched = np.setdiff1d(np.arange(48), slots[ok])
    assert (full[untouched] == 0xAB).all()
    ref = _advance_table(model, ids[ok], num_slots=n_slots, slots=slots[ok])
    pay = model.num_blocks * 1024 + 256 + 4
    assert np.array_equal(full[slots[ok], :pay], ref[slots[ok], :pay])
    assert (full[slots[ok], pay:] == 0xAB).all()                          # padding bytes are left alone
    new = _draw_new(rng, B, 2)
    q2 = _np(model.advance(st, new, slots=slots))
    assert np.array_equal(_bits(q2[ok]), _bits(orc.encode_last(_concat_live(ids, new))[ok]))
    assert not q2[[3, 8]].any()


# ---- 7. chunking ---------------------------------------------------------------------------------------------------------
def test_chunking(env):
    _, _, model, orc, _ = env
    L = 200
    cu = (1 << 21) // L                 # users per encoder chunk at this L
    B = cu + 15
    rng = np.random.default_rng(70)
    live = np.zeros((B, 3), np.int64)
    n = rng.integers(1, 4, size=B)
    for k in (1, 2, 3):
        rows = np.nonzero(n == k)[0]
        live[rows[:, None], np.arange(3 - k, 3)[None]] = rng.integers(1, 301, size=(len(rows), k))
    ids = np.zeros((B, L), np.int64)
    ids[:, L - 3:] = live
    st = model.new_user_states(B)
    q = _np(model.encode_states(st, torch.from_numpy(ids)))
    assert np.array_equal(_bits(q), _bits(orc.encode_last(live)))
    new = rng.integers(1, 301, size=(B, 1)).astype(np.int64)
    q2 = _np(model.advance(st, new))
    sel = np.union1d(np.arange(B - 64, B), np.arange(cu - 32, min(B, cu + 32)))
    assert (sel < cu).sum() >= 32 and (sel >= cu).sum() == 15
    assert np.array_equal(_bits(q2[sel]), _bits(orc.encode_last(np.concatenate([live, new], axis=1)[sel])))


# ---- 8. seeded top-K -----------------------------------------------------------------------------------------------------
def _seeded_topk_case(model, orc, ids, K, excl, V, rng):
    B = ids.shape[0]
    st = model.new_user_states(B)
    idx, sc = model.retrieve_topk(ids, K, excl, states=st)
    idx0, sc0 = model.retrieve_topk(ids, K, excl)
    oi, os_ = orc.retrieve_topk(ids, K, excl)
    assert torch.equal(idx, idx0) and np.array_equal(_bits(_np(sc)), _bits(_np(sc0)))
    assert np.array_equal(_np(idx), oi) and np.array_equal(_bits(_np(sc)), _bits(os_))
    _assert_same_rows(st.numpy(), _advance_table(model, ids), model.num_blocks)
    new = rng.integers(1, V + 1, size=(B, 1)).astype(np.int64)
    hist = _concat_live(_seen(ids), new)
    idx2, sc2 = model.retrieve_topk_from_states(st, K, new_ids=new, exclude=hist)
    oi2, os2 = orc.retrieve_topk(hist, K, True)
    assert np.array_equal(_np(idx2), oi2) and np.array_equal(_bits(_np(sc2)), _bits(os2))


@pytest.mark.parametrize("K", [1, 50])
@pytest.mark.parametrize("excl", [False, True])
@pytest.mark.parametrize("case", GOLDEN)
def test_seeded_topk_golden(env, case, K, excl):
    z, _, model, orc, _ = env
    _seeded_topk_case(model, orc, z[f"ids/{case}"], K, excl, 300, np.random.default_rng(K))


@pytest.mark.parametrize("K", [1, 50])
@pytest.mark.parametrize("excl", [False, True])
def test_seeded_topk_small_catalog(K, excl):
    """tests/test_gpu_lru._big_case's smallest shape: a catalog smaller than K + history."""
    from llamarec_amd.lru import LRURec
    from oracle import lru_oracle as O

    sd, ids = _big_case(33, 9, 50, seed=42)
    _seeded_topk_case(LRURec.from_state_dict(sd), O.LruOracle(sd), ids, K, excl, 33, np.random.default_rng(K))


# ---- 9. existing calls unchanged -----------------------------------------------------------------------------------------
def test_existing_calls_unchanged(env):
    from llamarec_amd._lib import lib

    z, _, model, orc, _ = env
    assert lib().lr_lru_workspace_bytes(model._h, 4096, 50, 200) == PARENT_WS_4096_50_200
    assert lib().lr_lru_workspace_bytes(model._h, 1, 1, 7) == PARENT_WS_1_1_7
    ids = z["ids/L64"]
    st = model.new_user_states(ids.shape[0])
    model.retrieve_topk(ids, 50, True, states=st)      # a seeding call on the handle and workspace the next calls reuse
    model.encode_states(st, ids)
    assert np.array_equal(_bits(_np(model.encode_last(ids))), _bits(orc.encode_last(ids)))
    idx, sc = model.retrieve_topk(ids, 50, True)
    oi, os_ = orc.retrieve_topk(ids, 50, True)
    assert np.array_equal(_np(idx), oi) and np.array_equal(_bits(_np(sc)), _bits(os_))


# ---- 10. argument checks -------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing(env):
    from llamarec_amd._lib import lib, stream_ptr

    z, _, model, _, _ = env
    l = lib()
    ids = torch.from_numpy(z["ids/L7"]).to(model.device)
    B, L = ids.shape
    st = model.new_user_states(B)
    st.table.fill_(0x5C)
    need = l.lr_lru_user_state_encode_workspace_bytes(model._h, B, 50, L)
    assert need >= l.lr_lru_user_state_encode_workspace_bytes(model._h, B, 1, L) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=model.device)
    q = torch.zeros((B, 64), device=model.device)
    idx = torch.zeros((B, 50), dtype=torch.int32, device=model.device)
    T, I, W, Q, X = st.table.data_ptr(), ids.data_ptr(), ws.data_ptr(), q.data_ptr(), idx.data_ptr()
    need1 = l.lr_lru_user_state_encode_workspace_bytes(model._h, B, 1, L)

    def enc(states=T, ids_=I, B_=B, L_=L, ws_=W, nbytes=need1, slots=None):
        return l.lr_lru_user_state_encode(model._h, states, B, slots, ids_, B_, L_, Q, ws_, nbytes, stream_ptr())

    def top(states=T, ids_=I, B_=B, L_=L, K=50, out=X, ws_=W, nbytes=need):
        return l.lr_lru_retrieve_topk_seed_user_state(model._h, states, B, None, ids_, B_, L_, K, 1, out, None, ws_, nbytes,
                                                      stream_ptr())

    with torch.cuda.device(model.device):
        for call in (enc, top):
            for kw, code in ((dict(states=None), EINVAL), (dict(ids_=None), EINVAL), (dict(L_=0), EINVAL),
                             (dict(B_=-1), EINVAL), (dict(ws_=None), EWORKSPACE),
                             (dict(nbytes=(need1 if call is enc else need) - 1), EWORKSPACE)):
                assert call(**kw) == code, (call.__name__, kw)
                assert len(l.lr_last_error()) > 0
        for K in (0, 65):
            assert top(K=K) == EINVAL and b"K=" in l.lr_last_error()
        assert top(out=None) == EINVAL and len(l.lr_last_error()) > 0
        assert enc(B_=0) == 0 and top(B_=0) == 0        # B = 0 is LR_OK and launches nothing
        torch.cuda.synchronize()
        assert (st.numpy() == 0x5C).all() and not _np(q).any() and not _np(idx).any()
        assert enc() == 0 and top() == 0                # the same arguments, unbroken, do run
        torch.cuda.synchronize()
    assert not (st.numpy()[:, :2048 + 260] == 0x5C).all(1).any()


# ---- 11. RetrieverSession(model, history=) -------------------------------------------------------------------------------
def test_retriever_session_with_history(env):
    from llamarec_amd.inference import RetrieverSession, retrieve_candidates

    _, _, model, orc, _ = env
    h = np.random.default_rng(11).integers(1, 301, size=70).tolist()
    s = RetrieverSession(model, history=h)
    assert s.query == h
    got = s.candidates(20)
    assert got == retrieve_candidates(model, h, 20)
    assert got == orc.retrieve_topk(np.asarray(h).reshape(1, -1), 20, False)[0][0].tolist()
    s.append(123)
    assert s.query == h + [123]
    got2 = s.candidates(20)
    assert got2 == retrieve_candidates(model, h + [123], 20) and got2 != got
    empty = RetrieverSession(model)                     # unchanged without a history
    assert empty.query == [] and empty.append([5]).candidates(3) == retrieve_candidates(model, [5], 3)
