"""CPU: the host side of ranker sessions -- inference.RankerSession's common-prefix, rollback and keep
bookkeeping against a model object that records what it is sent, the new symbols' prototypes, and the slot size."""
import numpy as np
import pytest

from llamarec_amd import inference as I
from llamarec_amd.llm import PromptCache


class RecordingModel:
    """new_prompt_cache / extend_verbalize of LlamaRanker without a device: records every call and keeps cache.ids as
    the real one does (ids[:cached_len] + the kept new ids)."""

    def __init__(self):
        self.calls = []

    def new_prompt_cache(self, num_slots, max_tokens):
        return PromptCache(None, num_slots, max_tokens)

    def extend_verbalize(self, cache, slots, new_ids_list, label_token_ids, keep=None, cached_len=None):
        assert len(slots) == len(new_ids_list) == len(keep) == len(cached_len) == 1
        s, new, c, k = slots[0], list(new_ids_list[0]), cached_len[0], keep[0]
        assert 0 <= c <= len(cache.ids[s]) and 0 <= k <= len(new) and len(new) >= 1 and c + len(new) <= cache.max_tokens
        self.calls.append(dict(slot=s, cached_len=c, new=new, keep=k, prompt=cache.ids[s][:c] + new,
                               labels=list(label_token_ids)))
        cache.ids[s] = cache.ids[s][:c] + new[:k]
        return np.zeros((1, len(label_token_ids)), np.float32)


def test_session_sends_only_what_the_slot_does_not_share():
    m = RecordingModel()
    s = I.RankerSession(m, tokenizer=None, verbalizer=None, max_tokens=32)
    head, pool_a, pool_b = [1, 5, 6, 7, 8], [20, 21, 22, 9], [30, 31, 9]
    labels = [100, 101]
    # first prompt: everything is sent, everything is kept
    s.extend(head + pool_a, labels)
    assert m.calls[-1]["cached_len"] == 0 and m.calls[-1]["new"] == head + pool_a and m.calls[-1]["keep"] == 9
    assert (s.last_sent, s.sent_tokens) == (9, 9) and s.cache.ids[0] == head + pool_a
    # one more history item in front of the same pool: the shared head stays, the rest is rolled back and sent
    s.extend(head + [11] + pool_a, labels)
    assert m.calls[-1]["cached_len"] == 5 and m.calls[-1]["new"] == [11] + pool_a
    assert m.calls[-1]["prompt"] == head + [11] + pool_a
    assert (s.last_sent, s.sent_tokens) == (5, 14)
    # the same history with another pool
    s.extend(head + [11] + pool_b, labels)
    assert m.calls[-1]["cached_len"] == 6 and m.calls[-1]["new"] == pool_b and s.cache.ids[0] == head + [11] + pool_b
    # the same prompt again: the last token is always prefilled (its row gives the scores)
    s.extend(head + [11] + pool_b, labels)
    assert m.calls[-1]["cached_len"] == 8 and m.calls[-1]["new"] == [9] and s.last_sent == 1
    # a prompt that is a strict prefix of what the slot holds: rollback, one token sent
    s.extend(head, labels)
    assert m.calls[-1]["cached_len"] == 4 and m.calls[-1]["new"] == [8] and s.cache.ids[0] == head
    # nothing in common
    s.extend([2, 3], labels)
    assert m.calls[-1]["cached_len"] == 0 and s.cache.ids[0] == [2, 3]
    assert all(c["labels"] == labels and c["slot"] == 0 for c in m.calls)
    assert s.sent_tokens == sum(len(c["new"]) for c in m.calls)


def test_session_refuses_prompts_it_cannot_hold():
    m = RecordingModel()
    s = I.RankerSession(m, tokenizer=None, verbalizer=None, max_tokens=4)
    with pytest.raises(ValueError):
        s.extend([1, 2, 3, 4, 5], [7])
    with pytest.raises(ValueError):
        s.extend([], [7])
    assert not m.calls and s.sent_tokens == 0
    s.extend([1, 2, 3, 4], [7])
    assert m.calls[-1]["new"] == [1, 2, 3, 4]


def test_session_matches_on_token_ids_through_the_tokenizer():
    """rank() tokenises as rank_candidates does; a tokenizer that merges text across the junction of history and pool
    only shortens the reuse."""
    class Tok:
        def __call__(self, prompt, **kw):
            assert kw == dict(truncation=False, padding=False, return_tensors=None)
            return {"input_ids": [int(w) for w in prompt.split()]}

    m = RecordingModel()
    s = I.RankerSession(m, Tok(), verbalizer=None, max_tokens=16)
    s.extend(Tok()("1 2 3 4 5", truncation=False, padding=False, return_tensors=None)["input_ids"], [7])
    s.extend(Tok()("1 2 3 45", truncation=False, padding=False, return_tensors=None)["input_ids"], [7])   # "4 5" merged into one id
    assert m.calls[-1]["cached_len"] == 3 and m.calls[-1]["new"] == [45]


def test_new_symbols_have_prototypes():
    from llamarec_amd import _lib

    for name in ("lr_llama_kv_cache_slot_bytes", "lr_llama_extend_workspace_bytes", "lr_llama_extend_verbalize",
                 "lr_attention_varlen_cached"):
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["lr_llama_extend_verbalize"][1]) == 19
    assert len(_lib.PROTOTYPES["lr_attention_varlen_cached"][1]) == 19


def test_slot_bytes_is_pure_cpu_and_monotone():
    from llamarec_amd import _lib

    L = _lib.lib()
    prev = 0
    for t in (1, 2, 63, 64, 65, 460, 2048, 4096):
        b = L.lr_llama_kv_cache_slot_bytes(32, 32, 128, t)
        assert b >= 32 * t * 2 * 32 * 128 * 2 and b % 256 == 0 and b - 32 * t * 2 * 32 * 128 * 2 < 256
        assert b > prev
        prev = b
    assert L.lr_llama_kv_cache_slot_bytes(2, 1, 16, 3) == 512   # 2 * 3 * 32 * 2 = 384 bytes, padded
    for bad in ((0, 1, 16, 8), (2, 0, 16, 8), (2, 1, 6, 8), (2, 1, 512, 8), (2, 1, 16, 0)):
        assert L.lr_llama_kv_cache_slot_bytes(*bad) == 0
    # the device entry points check their arguments before anything touches a GPU
    rc = L.lr_attention_varlen_cached(None, None, None, 1, 8, 1, 0, None, None, None, None, None, None, 1, 2, 2, 16, 0, None)
    assert rc == -1 and b"null pointer" in L.lr_last_error()
    rc = L.lr_llama_extend_verbalize(None, None, 1, 8, None, None, None, None, None, None, None, None, 1, None, 1, None, None, 0,
                                     None)
    assert rc == -1 and b"null pointer" in L.lr_last_error()
