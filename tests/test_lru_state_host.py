"""CPU: the host side of the LRURec user-state entry points -- the row size, and every argument check, which runs before
anything touches a device (no GPU is needed: a bad call never gets that far)."""
import ctypes as C

import numpy as np
import pytest
import torch

EINVAL = -1


@pytest.fixture(scope="module")
def l():
    from llamarec_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def fake():
    """Non-null stand-ins for a handle, a table and the other buffers: zeroed host memory no valid call is made with."""
    buf = C.create_string_buffer(1 << 16)
    return C.addressof(buf), buf


def _failed(l, rc, code=EINVAL):
    msg = l.lr_last_error()
    return rc == code and len(msg) > 0


def test_row_bytes(l):
    for nb in (1, 2, 3, 4):
        raw = nb * 1024 + 256 + 4
        assert l.lr_lru_user_state_row_bytes(nb) == (raw + 255) // 256 * 256 == nb * 1024 + 512
    assert l.lr_lru_user_state_row_bytes(0) == 0
    assert l.lr_lru_user_state_row_bytes(5) == 0


def test_reset_checks(l, fake):
    p, _ = fake
    assert _failed(l, l.lr_lru_user_state_reset(None, p, 4, None, 0, None)) and b"null" in l.lr_last_error()
    assert _failed(l, l.lr_lru_user_state_reset(p, None, 4, None, 0, None)) and b"null" in l.lr_last_error()
    assert _failed(l, l.lr_lru_user_state_reset(p, p, 0, None, 0, None)) and b"num_slots" in l.lr_last_error()
    assert _failed(l, l.lr_lru_user_state_reset(p, p, 4, p, -1, None)) and b"B=-1" in l.lr_last_error()
    assert l.lr_lru_user_state_reset(p, p, 4, p, 0, None) == 0   # B = 0: nothing to do, nothing launched


def test_advance_checks(l, fake):
    p, _ = fake
    adv = l.lr_lru_user_state_advance
    assert _failed(l, adv(None, p, 4, None, p, 2, 1, p, None)) and b"null" in l.lr_last_error()
    assert _failed(l, adv(p, None, 4, None, p, 2, 1, p, None)) and b"null" in l.lr_last_error()
    assert _failed(l, adv(p, p, 0, None, p, 2, 1, p, None)) and b"num_slots" in l.lr_last_error()
    assert _failed(l, adv(p, p, -3, None, p, 2, 1, p, None)) and b"num_slots" in l.lr_last_error()
    assert _failed(l, adv(p, p, 4, None, p, -1, 1, p, None)) and b"B=-1" in l.lr_last_error()
    assert _failed(l, adv(p, p, 4, None, p, 2, -1, p, None)) and b"Ln=-1" in l.lr_last_error()
    assert _failed(l, adv(p, p, 4, None, None, 2, 3, p, None)) and b"new_ids" in l.lr_last_error()
    assert adv(p, p, 4, None, p, 0, 1, p, None) == 0   # B = 0 is LR_OK and launches nothing


def test_retrieve_checks(l, fake):
    p, _ = fake
    ret = l.lr_lru_retrieve_topk_user_state

    def call(h=p, states=p, num_slots=4, new_ids=p, B=2, Ln=1, excl=p, Lx=3, K=10, out_idx=p, ws=p, ws_bytes=1 << 16):
        return ret(h, states, num_slots, None, new_ids, B, Ln, excl, Lx, K, out_idx, None, ws, ws_bytes, None)

    assert _failed(l, call(h=None)) and b"null" in l.lr_last_error()
    assert _failed(l, call(states=None)) and b"null" in l.lr_last_error()
    assert _failed(l, call(num_slots=0)) and b"num_slots" in l.lr_last_error()
    assert _failed(l, call(B=-2)) and b"B=-2" in l.lr_last_error()
    assert _failed(l, call(Ln=-1)) and b"Ln=-1" in l.lr_last_error()
    assert _failed(l, call(new_ids=None, Ln=2)) and b"new_ids" in l.lr_last_error()
    assert _failed(l, call(Lx=-1)) and b"Lx=-1" in l.lr_last_error()
    assert _failed(l, call(excl=None, Lx=2)) and b"exclude_ids" in l.lr_last_error()
    for K in (0, -1, 65):
        assert _failed(l, call(K=K)) and b"K=" in l.lr_last_error()
    assert _failed(l, call(out_idx=None)) and b"null" in l.lr_last_error()
    assert _failed(l, call(ws=None)) and b"null" in l.lr_last_error()
    assert call(B=0) == 0


def test_python_wrappers_reject_bad_arguments():
    from llamarec_amd.lru import LRURec, UserStates

    model = LRURec.__new__(LRURec)   # no device: the checks below come before any call into the library
    model.device, model.num_blocks = torch.device("cpu"), 2
    st = UserStates(torch.zeros((4, 2560), dtype=torch.uint8))
    assert st.num_slots == 4 and st.numpy().shape == (4, 2560)
    with pytest.raises(ValueError):
        model.advance(st, np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        model.advance(st, np.zeros((2, 2, 2), np.int64))
    for k in (0, 65):
        with pytest.raises(ValueError):
            model.retrieve_topk_from_states(st, k)
    with pytest.raises(ValueError):
        model.retrieve_topk_from_states(st, 5, new_ids=np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        model.retrieve_topk_from_states(st, 5, exclude=np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        model.advance(st, np.ones((2, 1), np.int64), slots=np.array([[0, 1]]))
    with pytest.raises(ValueError):
        model.advance(st, np.ones((5, 1), np.int64))   # more users than slots
    with pytest.raises(ValueError):
        model.new_user_states(0)
    with pytest.raises(ValueError):
        model.load_user_states(np.zeros((4, 100), np.uint8))
