"""CPU: the host side of the user-state seeding calls (lr_lru_user_state_encode_workspace_bytes, lr_lru_user_state_encode,
lr_lru_retrieve_topk_seed_user_state): header, ctypes prototypes and the built library agree on them, and the checks that
need no device."""
import ctypes
import inspect
import os
import re

NAMES = ("lr_lru_user_state_encode_workspace_bytes", "lr_lru_user_state_encode", "lr_lru_retrieve_topk_seed_user_state")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declarations():
    text = open(os.path.join(REPO, "include", "llamarec_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(lr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_prototypes_and_library_agree():
    from llamarec_amd import _lib

    decl = _declarations()
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in decl, f"{name} is not declared in include/llamarec_mi355x.h"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
        assert hasattr(l, name), f"{name} is not exported by the library"
        n_args = len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"])
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert _lib.PROTOTYPES[NAMES[0]][0] is ctypes.c_size_t
    assert _lib.PROTOTYPES[NAMES[1]][0] is ctypes.c_int and _lib.PROTOTYPES[NAMES[2]][0] is ctypes.c_int


def test_workspace_bytes_of_a_null_handle_is_zero_with_an_error_text():
    from llamarec_amd import _lib

    l = _lib.lib()
    assert l.lr_lru_user_state_encode_workspace_bytes(None, 4096, 50, 200) == 0
    assert b"lr_lru_user_state_encode_workspace_bytes" in l.lr_last_error()


def test_argument_checks_come_before_the_device():
    from llamarec_amd import _lib

    l = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    enc, top = l.lr_lru_user_state_encode, l.lr_lru_retrieve_topk_seed_user_state
    assert enc(None, p, 4, None, p, 2, 5, p, p, 1 << 12, None) == -1 and b"null" in l.lr_last_error()
    assert enc(p, None, 4, None, p, 2, 5, p, p, 1 << 12, None) == -1 and b"null" in l.lr_last_error()
    assert enc(p, p, 0, None, p, 2, 5, p, p, 1 << 12, None) == -1 and b"num_slots" in l.lr_last_error()
    assert enc(p, p, 4, None, p, -2, 5, p, p, 1 << 12, None) == -1 and b"B=-2" in l.lr_last_error()
    assert enc(p, p, 4, None, p, 2, 0, p, p, 1 << 12, None) == -1 and b"L=0" in l.lr_last_error()
    assert enc(p, p, 4, None, None, 2, 5, p, p, 1 << 12, None) == -1 and b"ids" in l.lr_last_error()
    assert enc(p, p, 4, None, p, 0, 5, p, p, 1 << 12, None) == 0
    assert top(p, p, 4, None, p, 2, 5, 0, 1, p, None, p, 1 << 12, None) == -1 and b"K=0" in l.lr_last_error()
    assert top(p, p, 4, None, p, 2, 5, 65, 1, p, None, p, 1 << 12, None) == -1 and b"K=65" in l.lr_last_error()
    assert top(p, p, 4, None, p, 2, 5, 10, 1, None, None, p, 1 << 12, None) == -1 and b"out_idx" in l.lr_last_error()
    assert top(p, p, 4, None, None, 2, 5, 10, 1, p, None, p, 1 << 12, None) == -1 and b"ids" in l.lr_last_error()
    assert top(p, p, 4, None, p, 0, 5, 10, 1, p, None, p, 1 << 12, None) == 0


def test_retrieve_topk_keeps_its_three_argument_call():
    from llamarec_amd.lru import LRURec

    sig = inspect.signature(LRURec.retrieve_topk)
    names = list(sig.parameters)
    assert names[:4] == ["self", "x", "k", "exclude_history"]
    sig.bind(object(), [[1, 2]], 5, False)                 # the call every existing caller makes
    sig.bind(object(), [[1, 2]], 5)
    assert sig.parameters["exclude_history"].default is True
    assert sig.parameters["states"].default is None and sig.parameters["slots"].default is None
    assert "x" in inspect.signature(LRURec.encode_states).parameters
    from llamarec_amd.inference import RetrieverSession

    assert inspect.signature(RetrieverSession.__init__).parameters["history"].default is None
