"""Online single-user path -- mirror of the reference's demo/inference.py:46-109 (second caller of
the same boundary): retrieve_candidates (no left padding, no history mask,
top_k 20..50), generate_prompt (titles NOT truncated), rank_candidates (verbalizer scores at the
last token -> top-k candidates). The Streamlit UI around it is out of scope.
"""
from __future__ import annotations

import numpy as np
import torch

from . import metrics as M
from . import prompt as P


def retrieve_candidates(model, query, top_k: int = 20):
    """demo/inference.py:46-53: `model(seqs)[:, -1, :]` then torch.topk -- here the fused retrieve
    without history exclusion (the demo does not mask the history)."""
    seqs = np.asarray(query, dtype=np.int64).reshape(1, -1)
    idx, _ = model.retrieve_topk(seqs, top_k, exclude_history=False)
    return idx[0].tolist()


class RetrieverSession:
    """One user's retriever state carried across interactions: `append` the items as they arrive, `candidates` whenever
    a list is wanted. Returns what `retrieve_candidates(model, whole_query, top_k)` returns for everything appended so
    far, without re-encoding it (LRURec.advance: one recurrence step per new item). A `history` the user already has is
    encoded once, in one call that also leaves the state (LRURec.encode_states), and `query` starts as that list."""

    def __init__(self, model, history=None):
        self.model = model
        self.states = model.new_user_states(1)
        self.query = []
        if history is not None:
            items = np.asarray(history, dtype=np.int64).reshape(-1)
            if items.size:
                model.encode_states(self.states, items.reshape(1, -1))
                self.query = items.tolist()

    def append(self, item_ids):
        """Add one item id or a sequence of them to the end of the user's history."""
        items = np.asarray(item_ids, dtype=np.int64).reshape(-1)
        if items.size:
            self.model.advance(self.states, items.reshape(1, -1))
            self.query.extend(items.tolist())
        return self

    def candidates(self, top_k: int = 20):
        idx, _ = self.model.retrieve_topk_from_states(self.states, top_k)
        return idx[0].tolist()


def generate_prompt(query, candidates, dataset_map, instruction=P.DEFAULT_SYSTEM_TEMPLATE,
                    input_template=P.DEFAULT_INPUT_TEMPLATE, prompter=None):
    """demo/inference.py:79-109 (titles verbatim, alpaca_short layout)."""
    q_t = " \n ".join("(" + str(i + 1) + ") " + dataset_map[item] for i, item in enumerate(query))
    c_t = " \n ".join("(" + chr(ord("A") + i) + ") " + dataset_map[item] for i, item in enumerate(candidates))
    return (prompter or P.Prompter()).generate_prompt(instruction, input_template.format(q_t, c_t))


def rank_candidates(model, tokenizer, prompt, candidates, verbalizer, top_k: int = 10):
    """demo/inference.py:56-76: tokenise, one forward, verbalizer scores at the last position,
    top-k of the candidates (here: ordered by score desc, ties -> earlier candidate)."""
    ids = tokenizer(prompt, truncation=False, padding=False, return_tensors=None)["input_ids"]
    scores = model.prefill_verbalize([np.asarray(ids, dtype=np.int32)], verbalizer.label_token_ids[: len(candidates)])
    order = M.rank_classes(scores)[0].tolist()
    return [candidates[i] for i in order[:top_k]]


class RankerSession:
    """One user's prompt K / V cache carried across rankings, the stage-2 counterpart of RetrieverSession: `rank` returns
    what `rank_candidates(model, tokenizer, prompt, candidates, verbalizer, top_k)` returns, but prefills only the tokens
    behind the longest prefix the prompt shares with the previous one (LlamaRanker.extend_verbalize). The numbered history
    of generate_prompt is not truncated, so after one more item, or with another candidate pool, that prefix reaches to the
    end of the old history.

    Matching is on token ids, never on text: whatever the tokenizer does where history and pool meet, a mismatch only
    shortens the reuse. Every new token is kept in the slot (keep = all of them) and the NEXT call's comparison decides how
    much of it is reused; whatever lies behind the common prefix is dropped by lowering the host length, which costs
    nothing. `sent_tokens` counts the tokens prefilled so far, `last_sent` those of the last call.

    For online use set the model to the row-invariant latency mode first, `model.set_variants(7, 0)`: the calls then split K
    as the latency-mode whole prompt does and return `rank_candidates`' scores under that mode bit for bit. In the default
    mode (and under gemm variant 5, which runs the default-mode products here) a short new part leaves most of the card idle."""

    def __init__(self, model, tokenizer, verbalizer, max_tokens=2048):
        self.model, self.tokenizer, self.verbalizer = model, tokenizer, verbalizer
        self.max_tokens = int(max_tokens)
        self.cache = model.new_prompt_cache(1, self.max_tokens)
        self.sent_tokens = 0
        self.last_sent = 0

    def extend(self, ids, label_token_ids):
        """Scores (fp32 [1, C]) of the prompt `ids` at its last token, reusing what the slot shares with it."""
        ids = [int(t) for t in ids]
        if not ids:
            raise ValueError("RankerSession: an empty prompt")
        if len(ids) > self.max_tokens:
            raise ValueError(f"RankerSession: a prompt of {len(ids)} tokens exceeds max_tokens {self.max_tokens}")
        held = self.cache.ids[0]
        c = 0
        while c < len(held) and c < len(ids) - 1 and held[c] == ids[c]:   # the last token is always prefilled: its row scores
            c += 1
        new = ids[c:]
        scores = self.model.extend_verbalize(self.cache, [0], [new], label_token_ids, keep=[len(new)], cached_len=[c])
        self.last_sent = len(new)
        self.sent_tokens += len(new)
        return scores

    def rank(self, prompt, candidates, top_k: int = 10):
        ids = self.tokenizer(prompt, truncation=False, padding=False, return_tensors=None)["input_ids"]
        scores = self.extend(ids, self.verbalizer.label_token_ids[: len(candidates)])
        order = M.rank_classes(scores)[0].tolist()
        return [candidates[i] for i in order[:top_k]]
