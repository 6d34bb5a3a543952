"""Deterministic synthetic weights and workloads (no datasets or checkpoints exist offline).

Everything here is integer-hash based or uses numpy.random.default_rng with the seeds fixed in
BASELINE.md section 3, so the same inputs are rebuilt bit-for-bit on any machine.
"""
from __future__ import annotations

import numpy as np

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xBF58476D1CE4E5B9)
_M3 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed: int, n: int, offset: int = 0) -> np.ndarray:
    """n 64-bit hashes of the counters offset..offset+n-1 under `seed` (splitmix64 finaliser)."""
    with np.errstate(over="ignore"):
        z = (np.arange(offset + 1, offset + n + 1, dtype=np.uint64) * _M1) + np.uint64(seed) * _M3
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        z = z ^ (z >> np.uint64(31))
    return z


def hash_uniform(seed: int, shape, std: float = 0.02) -> np.ndarray:
    """float32 array, uniform with standard deviation `std` (exactly reproducible: only
    integer hashing and power-of-two scaling followed by one float32 multiply)."""
    n = int(np.prod(shape))
    u = (splitmix64(seed, n) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return (u * np.float32(std * np.sqrt(3.0))).reshape(shape)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even float32 -> bfloat16 bit patterns (uint16). NaNs stay NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    out = ((u + r) >> np.uint32(16)).astype(np.uint16)
    nan = np.isnan(x)
    if nan.any():
        out = np.where(nan, np.uint16(0x7FC0), out)
    return out


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bfloat16 (returned as float32)."""
    return bf16_bits_to_f32(f32_to_bf16_bits(x))


def llama_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF LlamaForCausalLM parameter names and shapes for a config dict (no biases)."""
    d, f, v = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = d // nh
    out = [("model.embed_tokens.weight", (v, d))]
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        out += [
            (p + "self_attn.q_proj.weight", (nh * hd, d)),
            (p + "self_attn.k_proj.weight", (nkv * hd, d)),
            (p + "self_attn.v_proj.weight", (nkv * hd, d)),
            (p + "self_attn.o_proj.weight", (d, nh * hd)),
            (p + "mlp.gate_proj.weight", (f, d)),
            (p + "mlp.up_proj.weight", (f, d)),
            (p + "mlp.down_proj.weight", (d, f)),
            (p + "input_layernorm.weight", (d,)),
            (p + "post_attention_layernorm.weight", (d,)),
        ]
    out += [("model.norm.weight", (d,)), ("lm_head.weight", (v, d))]
    return out


def synth_llama_state(cfg: dict, seed: int, std: float = 0.02, norm_jitter: float = 0.1) -> dict:
    """name -> float32 array. Matrices ~ U(std); norm weights = 1 + U(norm_jitter).
    Values are bf16-representable so that fp32 and bf16 runs use identical weights."""
    sd = {}
    for i, (name, shape) in enumerate(llama_param_shapes(cfg)):
        if len(shape) == 1:
            w = np.float32(1.0) + hash_uniform(seed * 1000 + i, shape, norm_jitter)
        else:
            w = hash_uniform(seed * 1000 + i, shape, std)
        sd[name] = bf16_round(w)
    return sd


def gemma_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF GemmaForCausalLM parameter names and shapes: Llama's, with head_dim from the config (gemma-7b: 16 x 256 heads
    on a 3072-wide residual) and no lm_head (tied to the embedding)."""
    d, f, v = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or d // nh
    out = [("model.embed_tokens.weight", (v, d))]
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        out += [
            (p + "self_attn.q_proj.weight", (nh * hd, d)),
            (p + "self_attn.k_proj.weight", (nkv * hd, d)),
            (p + "self_attn.v_proj.weight", (nkv * hd, d)),
            (p + "self_attn.o_proj.weight", (d, nh * hd)),
            (p + "mlp.gate_proj.weight", (f, d)),
            (p + "mlp.up_proj.weight", (f, d)),
            (p + "mlp.down_proj.weight", (d, f)),
            (p + "input_layernorm.weight", (d,)),
            (p + "post_attention_layernorm.weight", (d,)),
        ]
    out += [("model.norm.weight", (d,))]
    return out


def gemma2_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF Gemma2ForCausalLM parameter names and shapes: Gemma's, plus the two norms per layer of the sandwich
    (pre_feedforward_layernorm in front of the MLP, post_feedforward_layernorm on its output; post_attention_layernorm is
    on the attention output here), in the order of HF's module tree per layer. No lm_head (tied)."""
    d = cfg["hidden_size"]
    out = []
    for name, shape in gemma_param_shapes(cfg):
        out.append((name, shape))
        if name.endswith("post_attention_layernorm.weight"):
            p = name[: -len("post_attention_layernorm.weight")]
            out += [(p + "pre_feedforward_layernorm.weight", (d,)), (p + "post_feedforward_layernorm.weight", (d,))]
    return out


def synth_gemma2_state(cfg: dict, seed: int, std: float = 0.02, norm_std: float = 0.3) -> dict:
    """As synth_gemma_state for a Gemma-2 config (four norms per layer). bf16 values."""
    sd = {}
    for i, (name, shape) in enumerate(gemma2_param_shapes(cfg)):
        sd[name] = bf16_round(hash_uniform(seed * 1000 + i, shape, norm_std if len(shape) == 1 else std))
    return sd


def gemma3_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF Gemma3ForCausalLM (text) parameter names and shapes: Gemma-2's, with q_norm.weight and k_norm.weight [head_dim] behind
    o_proj (HF's module order). No lm_head (tied)."""
    hd = cfg["head_dim"]
    out = []
    for name, shape in gemma2_param_shapes(cfg):
        out.append((name, shape))
        if name.endswith("o_proj.weight"):
            p = name[: -len("o_proj.weight")]
            out += [(p + "q_norm.weight", (hd,)), (p + "k_norm.weight", (hd,))]
    return out


# a tiny Gemma-3 (train_ranker.py --synthetic --llm gemma3): 7 layers, so both layer kinds occur and the last one is sliding;
# MQA at head_dim 256 on a hidden size that misses the 256-column GEMM tile; a window far below the synthetic prompts' length
GEMMA3_TINY = dict(model_type="gemma3_text", vocab_size=1000, hidden_size=320, intermediate_size=512, num_hidden_layers=7,
                   num_attention_heads=2, num_key_value_heads=1, head_dim=256, max_position_embeddings=4096, rms_norm_eps=1e-6,
                   rope_theta=1000000.0, rope_local_base_freq=10000.0, rope_scaling=None, sliding_window=64,
                   sliding_window_pattern=6, query_pre_attn_scalar=256, hidden_activation="gelu_pytorch_tanh",
                   attn_logit_softcapping=None, final_logit_softcapping=None, attention_bias=False)


def synth_gemma3_state(cfg: dict, seed: int, std: float = 0.02, norm_std: float = 0.3, qk_norm_spread: float = 0.75,
                       qk_norm_mean=0.0, attn_out_mean: float = 0.0, mlp_out_mean: float = 0.0) -> dict:
    """As synth_gemma2_state for a Gemma-3 config: matrices ~ U(std), the hidden-size norm weights ~ U(norm_std) around 0 (Gemma
    scales by 1 + w), the q / k norm weights qk_norm_mean + U(qk_norm_spread) -- wide enough that a model normed with w in place
    of 1 + w is clearly another model; the q / k norm fixes the scale of the scores whatever q_proj / k_proj hold, so
    qk_norm_mean (one number, or one per layer) is what makes the attention peaked (scores ~ (1 + w)^2). attn_out_mean / mlp_out_mean: the means of the two
    out-norms of the sandwich, which weigh the attention branch against the MLP branch in the residual stream. bf16 values."""
    sd = {}
    for i, (name, shape) in enumerate(gemma3_param_shapes(cfg)):
        if name.endswith(("q_norm.weight", "k_norm.weight")):
            layer = int(name.split(".")[2])
            mean = qk_norm_mean[layer] if isinstance(qk_norm_mean, (list, tuple)) else qk_norm_mean
            w = np.float32(mean) + hash_uniform(seed * 1000 + i, shape, qk_norm_spread)
        elif name.endswith(("post_attention_layernorm.weight", "post_feedforward_layernorm.weight")):
            mean = attn_out_mean if "post_attention" in name else mlp_out_mean
            w = np.float32(mean) + hash_uniform(seed * 1000 + i, shape, norm_std)
        else:
            w = hash_uniform(seed * 1000 + i, shape, norm_std if len(shape) == 1 else std)
        sd[name] = bf16_round(w)
    return sd


def phi3_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF Phi3ForCausalLM parameter names and shapes: Llama's with the q | k | v Linears fused into self_attn.qkv_proj and
    gate | up into mlp.gate_up_proj (no biases, untied lm_head)."""
    d, f, v = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or d // nh
    out = [("model.embed_tokens.weight", (v, d))]
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}."
        out += [
            (p + "self_attn.qkv_proj.weight", ((nh + 2 * nkv) * hd, d)),
            (p + "self_attn.o_proj.weight", (d, nh * hd)),
            (p + "mlp.gate_up_proj.weight", (2 * f, d)),
            (p + "mlp.down_proj.weight", (d, f)),
            (p + "input_layernorm.weight", (d,)),
            (p + "post_attention_layernorm.weight", (d,)),
        ]
    out += [("model.norm.weight", (d,)), ("lm_head.weight", (v, d))]
    return out


# a tiny Phi-3 at head_dim 96 (train_ranker.py --synthetic --llm phi3; tests/gen_goldens_phi3.py's hd96_mha with another vocab)
PHI3_TINY = dict(model_type="phi3", vocab_size=1000, hidden_size=768, intermediate_size=1024, num_hidden_layers=2,
                 num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=4096,
                 original_max_position_embeddings=4096, rms_norm_eps=1e-5, rope_theta=10000.0, rope_scaling=None,
                 hidden_act="silu", sliding_window=2047, tie_word_embeddings=False)


def synth_phi3_state(cfg: dict, seed: int, std: float = 0.02, norm_jitter: float = 0.1) -> dict:
    """As synth_llama_state under Phi-3's fused names. bf16 values."""
    sd = {}
    for i, (name, shape) in enumerate(phi3_param_shapes(cfg)):
        if len(shape) == 1:
            w = np.float32(1.0) + hash_uniform(seed * 1000 + i, shape, norm_jitter)
        else:
            w = hash_uniform(seed * 1000 + i, shape, std)
        sd[name] = bf16_round(w)
    return sd


def qwen2_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF Qwen2ForCausalLM parameter names and shapes: Llama's with a bias behind each of q_proj, k_proj and v_proj (in HF's
    module order: weight, then bias), and no lm_head.weight when the embeddings are tied."""
    out = []
    for name, shape in llama_param_shapes(cfg):
        if name == "lm_head.weight" and cfg.get("tie_word_embeddings"):
            continue
        out.append((name, shape))
        if name.endswith(("q_proj.weight", "k_proj.weight", "v_proj.weight")):
            out.append((name[: -len("weight")] + "bias", (shape[0],)))
    return out


# a tiny Qwen2 at Qwen2-0.5B's widths (train_ranker.py --synthetic --llm qwen2; tests/gen_goldens_qwen2.py's hd64_ragged with
# another vocab): hidden 896 and qkv 1152 miss the 256-column GEMM tile, 14 query heads share 2 KV heads, tied head
QWEN2_TINY = dict(model_type="qwen2", vocab_size=1000, hidden_size=896, intermediate_size=1280, num_hidden_layers=2,
                  num_attention_heads=14, num_key_value_heads=2, max_position_embeddings=4096, rms_norm_eps=1e-6,
                  rope_theta=1000000.0, hidden_act="silu", use_sliding_window=False, sliding_window=4096, max_window_layers=2,
                  tie_word_embeddings=True)


def synth_qwen2_state(cfg: dict, seed: int, std: float = 0.02, bias_std: float = 0.5, norm_jitter: float = 0.1,
                      v_bias_std: float | None = None) -> dict:
    """As synth_llama_state under Qwen2's names: matrices ~ U(std), q/k/v biases ~ U(bias_std) (the published checkpoints'
    q and k biases reach several units), norm weights 1 + U(norm_jitter). v_bias_std: another width for v_proj's bias (the
    checkpoints' are small; a v bias far wider than v itself makes every position's value the same vector, and the attention
    weights -- all that the q and k biases act on -- then hardly reach the logits). bf16 values."""
    sd = {}
    for i, (name, shape) in enumerate(qwen2_param_shapes(cfg)):
        if name.endswith(".bias"):
            w = hash_uniform(seed * 1000 + i, shape, v_bias_std if v_bias_std is not None and "v_proj" in name else bias_std)
        elif len(shape) == 1:
            w = np.float32(1.0) + hash_uniform(seed * 1000 + i, shape, norm_jitter)
        else:
            w = hash_uniform(seed * 1000 + i, shape, std)
        sd[name] = bf16_round(w)
    return sd


def qwen3_param_shapes(cfg: dict) -> list[tuple[str, tuple]]:
    """HF Qwen3ForCausalLM parameter names and shapes: Llama's at the config's head_dim (q_proj [nh hd][hidden], o_proj
    [hidden][nh hd]) with q_norm.weight and k_norm.weight [head_dim] behind o_proj (HF's module order), and no lm_head.weight
    when the embeddings are tied."""
    hd = cfg["head_dim"]
    out = []
    for name, shape in gemma_param_shapes(cfg):   # Llama's names with head_dim from the config, no lm_head
        out.append((name, shape))
        if name.endswith("o_proj.weight"):
            p = name[: -len("o_proj.weight")]
            out += [(p + "q_norm.weight", (hd,)), (p + "k_norm.weight", (hd,))]
    if not cfg.get("tie_word_embeddings"):
        out.append(("lm_head.weight", (cfg["vocab_size"], cfg["hidden_size"])))
    return out


# a tiny Qwen3 (train_ranker.py --synthetic --llm qwen3; tests/gen_goldens_qwen3.py's hd128_gqa with another vocab): 4 query
# heads of head_dim 128 on 2 KV heads over a hidden size of 256 (nh * hd != hidden), tied head
QWEN3_TINY = dict(model_type="qwen3", vocab_size=1000, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                  num_attention_heads=4, num_key_value_heads=2, head_dim=128, max_position_embeddings=4096, rms_norm_eps=1e-6,
                  rope_theta=1000000.0, rope_scaling=None, hidden_act="silu", attention_bias=False, use_sliding_window=False,
                  sliding_window=None, max_window_layers=2, tie_word_embeddings=True)


def synth_qwen3_state(cfg: dict, seed: int, std: float = 0.02, norm_jitter: float = 0.1, qk_norm_spread: float = 0.75) -> dict:
    """As synth_llama_state under Qwen3's names: matrices ~ U(std), the hidden-size norm weights 1 + U(norm_jitter), the q / k
    norm weights 1 + U(qk_norm_spread) -- mean 1 and wide enough (uniform of standard deviation 0.75) that a model with ones in their place
    is clearly another model (tests/gen_goldens_qwen3.py checks by how much). bf16 values."""
    sd = {}
    for i, (name, shape) in enumerate(qwen3_param_shapes(cfg)):
        if name.endswith(("q_norm.weight", "k_norm.weight")):
            w = np.float32(1.0) + hash_uniform(seed * 1000 + i, shape, qk_norm_spread)
        elif len(shape) == 1:
            w = np.float32(1.0) + hash_uniform(seed * 1000 + i, shape, norm_jitter)
        else:
            w = hash_uniform(seed * 1000 + i, shape, std)
        sd[name] = bf16_round(w)
    return sd


def synth_gemma_state(cfg: dict, seed: int, std: float = 0.02, norm_std: float = 0.3) -> dict:
    """name -> float32 array for a Gemma config. Matrices ~ U(std); norm weights ~ U(norm_std) around 0 -- Gemma scales by
    (1 + w), so non-zero w exercises that form (w = 0 would make it indistinguishable from Llama's w = 1). bf16 values."""
    sd = {}
    for i, (name, shape) in enumerate(gemma_param_shapes(cfg)):
        sd[name] = bf16_round(hash_uniform(seed * 1000 + i, shape, norm_std if len(shape) == 1 else std))
    return sd


# ---------------------------------------------------------------------------------------------
# Synthetic workloads of BASELINE.json's configs (BASELINE.md section 3 / SURVEY.md 8(d)).
# V items, U users, L = bert_max_len, title-length range of the prompt model, rerank batch
# (config.py:98), cfg_idx = position in BASELINE.json "configs" (seeds 42 + cfg_idx).
# ---------------------------------------------------------------------------------------------
WORKLOADS = {
    "ml-100k": dict(V=3650, U=610, L=200, title=(3, 10), rerank_batch=32, cfg_idx=1),
    "beauty": dict(V=12086, U=22332, L=50, title=(10, 32), rerank_batch=16, cfg_idx=2),
    "games": dict(V=7676, U=15264, L=50, title=(6, 24), rerank_batch=16, cfg_idx=3),
    "synth-1m": dict(V=1_000_000, U=1_000_000, L=200, title=(10, 32), rerank_batch=16, cfg_idx=4),
}
LLM_MAX_TEXT_LEN = 1536   # config.py:236
LLM_MAX_HISTORY = 20      # config.py:237
NUM_CANDIDATES = 20       # llm_negative_sample_size + 1 (config.py:238-241)


def history_lengths(name: str, n_users: int, rng) -> np.ndarray:
    w = WORKLOADS[name]
    L = w["L"]
    if name == "ml-100k":
        n = np.clip(np.rint(rng.lognormal(4.4, 1.0, size=n_users)), 3, 200)
    elif name == "beauty":
        n = np.minimum(L, 3 + rng.geometric(0.2, size=n_users))
    elif name == "games":
        n = np.minimum(L, 3 + rng.geometric(0.17, size=n_users))
    else:
        n = rng.integers(20, 201, size=n_users)
    return np.minimum(n, L).astype(np.int64)


def synth_users(name: str, n_users: int | None = None, first_user: int = 0, seed_offset: int = 0):
    """Left-padded int64 histories [U, L], labels [U] (not in the history), history lengths, and
    prompt lengths T_u. Users are generated independently from (seed, user index) blocks so that a
    data-parallel rank can build exactly its own contiguous shard."""
    w = WORKLOADS[name]
    V, L = w["V"], w["L"]
    U = w["U"] if n_users is None else n_users
    rng = np.random.default_rng([42 + w["cfg_idx"] + seed_offset, first_user])
    n = history_lengths(name, U, rng)
    ids = np.zeros((U, L), np.int64)
    labels = np.zeros(U, np.int64)
    for u in range(U):
        # n_u + 1 distinct items: history + label
        pick = rng.choice(V, size=int(n[u]) + 1, replace=False) + 1 if V < 50_000 else \
            np.unique(rng.integers(1, V + 1, size=int(n[u]) + 8))[: int(n[u]) + 1]
        if len(pick) < n[u] + 1:  # pragma: no cover (astronomically unlikely for V >= 50k)
            pick = rng.choice(V, size=int(n[u]) + 1, replace=False) + 1
        pick = rng.permutation(pick)
        ids[u, L - n[u]:] = pick[: n[u]]
        labels[u] = pick[n[u]]
    lo, hi = w["title"]
    hist = np.minimum(n, LLM_MAX_HISTORY)
    T = np.empty(U, np.int64)
    for u in range(U):
        t = rng.integers(lo, hi + 1, size=int(hist[u]) + NUM_CANDIDATES)
        T[u] = min(LLM_MAX_TEXT_LEN, 48 + int((4 + t).sum()))
    return ids, labels, n, T


# Every prompt opens with the same template text (dataloader/utils.py:24-40, templates/alpaca_short.json:3,
# config.py:247-249): BOS + "### Instruction:\n<system sentence>\n\n### Input:\nUser history:" -- with the Llama-2
# sentencepiece vocabulary 1 + 5 + 20 + 2 + 4 + 3 = 35 tokens, then "(1)" of the first history item; the other
# template tokens of SURVEY.md 8(d)'s 48 ("; \n Candidate pool:", "\n\n### Response:\n") sit at user-dependent
# positions. Prompts clamped by the 1536-token LEFT truncation (config.py:236) lose that prefix.
TEMPLATE_PREFIX_TOKENS = 36


def synth_prompt_tokens(T: np.ndarray, seed: int, vocab: int = 32000, shared_prefix: bool = True):
    """Packed int32 prompt ids for prompt lengths T: BOS (=1) then uniform ids in [3, vocab). With shared_prefix the
    first TEMPLATE_PREFIX_TOKENS ids of every prompt shorter than LLM_MAX_TEXT_LEN are the same fixed template ids
    (the ids of a truncated prompt stay random: its head was cut off)."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, dtype=np.int64)
    cu = np.zeros(len(T) + 1, np.int32)
    cu[1:] = np.cumsum(T)
    ids = rng.integers(3, vocab, size=int(cu[-1]), dtype=np.int32)
    ids[cu[:-1]] = 1
    if shared_prefix:
        template = np.random.default_rng(20240807).integers(3, vocab, size=TEMPLATE_PREFIX_TOKENS, dtype=np.int32)
        template[0] = 1
        for b in range(len(T)):
            if T[b] < LLM_MAX_TEXT_LEN:
                n = min(TEMPLATE_PREFIX_TOKENS, int(T[b]))
                ids[cu[b]: cu[b] + n] = template[:n]
    return ids, cu


# ---- a deterministic stand-in tokenizer for --synthetic runs and tests (no Llama tokenizer files exist offline) ----
# Exposes exactly the calls the reference makes on its tokenizer (dataloader/llm.py:21-27,67-69,
# trainer/verb.py:494): tokenize, convert_tokens_to_string, __call__(truncation, max_length),
# encode(add_special_tokens=False), plus the attributes set at dataloader/llm.py:122-126.
import zlib


class FakeTokenizer:
    bos_token_id = 1
    eos_token_id = 2
    unk_token_id = 0
    pad_token = "<unk>"
    unk_token = "<unk>"
    padding_side = "left"
    truncation_side = "left"
    vocab_size = 1000

    def __init__(self):
        self.seen_texts = []

    def tokenize(self, text):
        return [t for t in text.split(" ") if t != ""]

    def convert_tokens_to_string(self, tokens):
        return " ".join(tokens)

    def _id(self, tok):
        return 3 + zlib.crc32(tok.encode("utf-8")) % (self.vocab_size - 3)

    def encode(self, text, add_special_tokens=True):
        ids = [self._id(t) for t in self.tokenize(text)]
        return ([self.bos_token_id] + ids) if add_special_tokens else ids

    def __call__(self, text, truncation=False, max_length=None, padding=False, return_tensors=None):
        self.seen_texts.append(text)
        ids = self.encode(text, add_special_tokens=True)
        if truncation and max_length is not None and len(ids) > max_length:
            ids = ids[-max_length:] if self.truncation_side == "left" else ids[:max_length]
        return {"input_ids": ids, "attention_mask": [1] * len(ids)}
