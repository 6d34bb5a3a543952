"""Llama-2 ranker -- host-side mirror of the reference's patched `LlamaForCausalLM` for the
SCORING path, backed by the HIP prefill kernels (no torch compute in the forward, no fallback).

Reference interface being replaced (paths into the reference tree):
  LlamaForCausalLM.forward(input_ids[B,T], attention_mask[B,T], labels=...) ->
      CausalLMOutputWithPast(loss=tensor(-1.0), logits=fp32[B,vocab])   model/llm.py:35-145
  ManualVerbalizer.process_logits(logits) -> fp32[B,20]                 trainer/verb.py:546-586
  weights: bf16 compute over NF4-quantised base + LoRA(--lora_target_modules)   train_ranker.py:49-79;
           here bf16 weights with the adapter merged at load (W + (alpha/r) B A) into each Linear it targets.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi as A
from ._lib import check, lib, stream_ptr

LLAMA2_7B = dict(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32,
                 num_attention_heads=32, num_key_value_heads=32, max_position_embeddings=4096,
                 rms_norm_eps=1e-5, rope_theta=10000.0)
# meta-llama/Llama-3.2-1B, Llama-3.2-3B and Llama-3.1-8B (config.json of the checkpoints): GQA, llama3 RoPE scaling
LLAMA3_ROPE_SCALING = dict(rope_type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                           original_max_position_embeddings=8192)
LLAMA32_1B = dict(model_type="llama", vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16,
                  num_attention_heads=32, num_key_value_heads=8, head_dim=64, max_position_embeddings=131072,
                  rms_norm_eps=1e-5, rope_theta=500000.0, tie_word_embeddings=True, rope_scaling=dict(LLAMA3_ROPE_SCALING))
LLAMA32_3B = dict(LLAMA32_1B, hidden_size=3072, num_hidden_layers=28, num_attention_heads=24, head_dim=128)
LLAMA31_8B = dict(LLAMA32_1B, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
                  head_dim=128, tie_word_embeddings=False, rope_scaling=dict(LLAMA3_ROPE_SCALING, factor=8.0))
# google/gemma-2b and google/gemma-7b (config.json of the checkpoints; the reference's --llm gemma loads gemma-2b)
GEMMA_2B = dict(model_type="gemma", vocab_size=256000, hidden_size=2048, intermediate_size=16384, num_hidden_layers=18,
                num_attention_heads=8, num_key_value_heads=1, head_dim=256, max_position_embeddings=8192,
                rms_norm_eps=1e-6, rope_theta=10000.0, hidden_activation="gelu_pytorch_tanh")
GEMMA_7B = dict(GEMMA_2B, hidden_size=3072, intermediate_size=24576, num_hidden_layers=28, num_attention_heads=16,
                num_key_value_heads=16)
# google/gemma-2-2b and google/gemma-2-9b (config.json of the checkpoints; the reference's --llm gemma2 loads gemma-2-9b).
# query_pre_attn_scalar is 256 = head_dim for both (144 for gemma-2-27b, whose head_dim is 128).
GEMMA2_2B = dict(model_type="gemma2", vocab_size=256000, hidden_size=2304, intermediate_size=9216, num_hidden_layers=26,
                 num_attention_heads=8, num_key_value_heads=4, head_dim=256, max_position_embeddings=8192,
                 rms_norm_eps=1e-6, rope_theta=10000.0, hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=256,
                 attn_logit_softcapping=50.0, final_logit_softcapping=30.0, sliding_window=4096)
GEMMA2_9B = dict(GEMMA2_2B, hidden_size=3584, intermediate_size=14336, num_hidden_layers=42, num_attention_heads=16,
                 num_key_value_heads=8)
# google/gemma-3-1b-pt (config.json of the checkpoint; model_type "gemma3_text"): five of every six layers attend to a window of
# 512 tokens and rotate with base 10 000, every sixth is global with base 1 000 000; q/k norms, sandwich norms, no caps. The
# larger text models (4b and up, window 1 024) add rope_scaling linear with factor 8 on the global layers.
GEMMA3_1B = dict(model_type="gemma3_text", vocab_size=262144, hidden_size=1152, intermediate_size=6912, num_hidden_layers=26,
                 num_attention_heads=4, num_key_value_heads=1, head_dim=256, max_position_embeddings=32768, rms_norm_eps=1e-6,
                 rope_theta=1000000.0, rope_local_base_freq=10000.0, rope_scaling=None, sliding_window=512,
                 sliding_window_pattern=6, query_pre_attn_scalar=256, hidden_activation="gelu_pytorch_tanh",
                 attn_logit_softcapping=None, final_logit_softcapping=None, attention_bias=False)
# microsoft/Phi-3-mini-4k-instruct and Phi-3-medium-4k-instruct (config.json of the checkpoints; the reference's --llm phi3).
# Llama's arithmetic with fused qkv_proj / gate_up_proj Linears; mini's head_dim is 3072 / 32 = 96.
PHI3_MINI = dict(model_type="phi3", vocab_size=32064, hidden_size=3072, intermediate_size=8192, num_hidden_layers=32,
                 num_attention_heads=32, num_key_value_heads=32, max_position_embeddings=4096,
                 original_max_position_embeddings=4096, rms_norm_eps=1e-5, rope_theta=10000.0, rope_scaling=None,
                 hidden_act="silu", sliding_window=2047, tie_word_embeddings=False)
PHI3_MEDIUM = dict(PHI3_MINI, hidden_size=5120, intermediate_size=17920, num_hidden_layers=40, num_attention_heads=40,
                   num_key_value_heads=10)
# Qwen/Qwen2-0.5B, Qwen2-1.5B and Qwen2-7B (config.json of the checkpoints; the reference's --llm qwen2 loads Qwen2-0.5B).
# Llama's arithmetic with a bias on q_proj / k_proj / v_proj. 0.5B's widths (896, qkv 1152) miss the 256-column GEMM tile.
QWEN2_0_5B = dict(model_type="qwen2", vocab_size=151936, hidden_size=896, intermediate_size=4864, num_hidden_layers=24,
                  num_attention_heads=14, num_key_value_heads=2, max_position_embeddings=131072, rms_norm_eps=1e-6,
                  rope_theta=1000000.0, hidden_act="silu", use_sliding_window=False, sliding_window=131072,
                  max_window_layers=24, tie_word_embeddings=True)
QWEN2_1_5B = dict(QWEN2_0_5B, hidden_size=1536, intermediate_size=8960, num_hidden_layers=28, num_attention_heads=12,
                  max_window_layers=28)
QWEN2_7B = dict(QWEN2_1_5B, vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_attention_heads=28,
                num_key_value_heads=4, tie_word_embeddings=False)
# Qwen/Qwen3-0.6B, Qwen3-1.7B, Qwen3-4B and Qwen3-8B (config.json of the checkpoints). Llama's arithmetic plus an RMSNorm over
# head_dim on every q and k head between the projection and the rotation; head_dim 128 comes from the config (0.6B: 16 heads
# of 128 on a hidden size of 1024), no biases.
QWEN3_0_6B = dict(model_type="qwen3", vocab_size=151936, hidden_size=1024, intermediate_size=3072, num_hidden_layers=28,
                  num_attention_heads=16, num_key_value_heads=8, head_dim=128, max_position_embeddings=40960, rms_norm_eps=1e-6,
                  rope_theta=1000000.0, rope_scaling=None, hidden_act="silu", attention_bias=False, use_sliding_window=False,
                  sliding_window=None, max_window_layers=28, tie_word_embeddings=True)
QWEN3_1_7B = dict(QWEN3_0_6B, hidden_size=2048, intermediate_size=6144)
QWEN3_4B = dict(QWEN3_0_6B, hidden_size=2560, intermediate_size=9728, num_hidden_layers=36, num_attention_heads=32,
                max_window_layers=36)
QWEN3_8B = dict(QWEN3_4B, hidden_size=4096, intermediate_size=12288, tie_word_embeddings=False)

# model_type -> backbone family of the kernels (LrLlamaArch). Llama-2 / Llama-3 and Mistral share Llama's arithmetic.
LLAMA_FAMILY = ("llama", "mistral")
GEMMA_FAMILY = ("gemma",)
GEMMA3_FAMILY = ("gemma3_text",)
GEMMA2_FAMILY = ("gemma2",)
PHI3_FAMILY = ("phi3",)
QWEN2_FAMILY = ("qwen2",)
QWEN3_FAMILY = ("qwen3",)
SUPPORTED_MODEL_TYPES = (LLAMA_FAMILY + PHI3_FAMILY + QWEN2_FAMILY + QWEN3_FAMILY + GEMMA_FAMILY + GEMMA3_FAMILY
                         + GEMMA2_FAMILY)
# what a gemma2 config must spell out (the two caps may be null): none of them has a default the kernels could assume
GEMMA2_REQUIRED_KEYS = ("query_pre_attn_scalar", "attn_logit_softcapping", "final_logit_softcapping", "sliding_window", "head_dim")
# what a gemma3_text config must spell out, besides one of layer_types / sliding_window_pattern (rope_local_base_freq may instead
# come as transformers 5's rope_parameters["sliding_attention"]["rope_theta"])
GEMMA3_REQUIRED_KEYS = ("head_dim", "query_pre_attn_scalar", "sliding_window", "rope_local_base_freq")
# what a phi3 config must spell out (sliding_window may be null = none); every published Phi-3 config.json has all three
PHI3_REQUIRED_KEYS = ("hidden_act", "original_max_position_embeddings", "sliding_window")
# what a qwen2 config must spell out (sliding_window may be null); every published Qwen2 config.json has all four
QWEN2_REQUIRED_KEYS = ("hidden_act", "use_sliding_window", "sliding_window", "max_window_layers")
# what a qwen3 config must spell out; every published dense Qwen3 config.json has all three (head_dim is not hidden / heads)
QWEN3_REQUIRED_KEYS = ("head_dim", "hidden_act", "attention_bias")


_LLAMA3_NUMBERS = ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings")


def rope_parameters(config: dict):
    """(rope_theta, llama3 scaling dict or None) of a HF config dict. The scaling sits in `rope_scaling` (transformers <= 4)
    or `rope_parameters` (transformers 5, which also moves rope_theta there); its `rope_type` (legacy key `type`) is
    "default" / absent (plain RoPE) or "llama3" with all four numbers. Anything else raises NotImplementedError: the
    rotary table cannot be computed from it."""
    rp = config.get("rope_parameters")
    rs = config.get("rope_scaling")
    theta = config.get("rope_theta")
    if theta is None and isinstance(rp, dict):
        theta = rp.get("rope_theta")
    src = rs if rs is not None else rp
    if src is None:
        return float(theta if theta is not None else 10000.0), None
    kind = (src.get("rope_type") or src.get("type") or "default") if isinstance(src, dict) else src
    if kind == "default":
        return float(theta if theta is not None else 10000.0), None
    if kind != "llama3":
        raise NotImplementedError(f"rope_scaling={src!r}: the rotary tables implement plain RoPE and rope_type 'llama3' only")
    missing = [k for k in _LLAMA3_NUMBERS if src.get(k) is None]
    if missing:
        raise NotImplementedError(f"rope_scaling={src!r}: rope_type 'llama3' needs {', '.join(missing)}")
    return float(theta if theta is not None else 10000.0), {k: src[k] for k in _LLAMA3_NUMBERS}


def _is_pos_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and 0 < v < float("inf")


def gemma3_parameters(config: dict) -> dict:
    """What a gemma3_text config says about its layers: dict(window, sliding = [bool per layer], theta_global, theta_local,
    factor = the global layers' linear scaling factor or None). Both spellings of the four rotary numbers are read: rope_theta /
    rope_local_base_freq / rope_scaling (transformers 4) and rope_parameters = {"full_attention": {...}, "sliding_attention":
    {...}} (transformers 5). Raises NotImplementedError (with the "supported families" text) for anything the kernels do not
    compute: a missing key, caps, biases, another activation, a rope scaling other than linear on the global layers."""
    mt = config.get("model_type")
    supported = f"supported families: {', '.join(SUPPORTED_MODEL_TYPES)}"

    def refuse(why):
        raise NotImplementedError(f"model_type {mt!r} {why}; {supported}")

    rp = config.get("rope_parameters")
    v5 = isinstance(rp, dict) and isinstance(rp.get("full_attention"), dict) and isinstance(rp.get("sliding_attention"), dict)
    missing = [k for k in GEMMA3_REQUIRED_KEYS if config.get(k) is None and not (k == "rope_local_base_freq" and v5)]
    if config.get("layer_types") is None and config.get("sliding_window_pattern") is None:
        missing.append("layer_types / sliding_window_pattern")
    if missing:
        refuse(f"config lacks {', '.join(missing)}: window, layer kinds, local rotary base, score scale and head_dim have no "
               "defaults the kernels could assume")
    act = config.get("hidden_activation") or config.get("hidden_act")
    if act != "gelu_pytorch_tanh":
        refuse(f"with hidden_activation={act!r}: the kernels implement gelu_pytorch_tanh")
    for k in ("attn_logit_softcapping", "final_logit_softcapping"):
        if config.get(k) is not None:
            refuse(f"with {k}={config[k]!r}: Gemma-3 has no soft caps and the windowed kernels have no capped form")
    if config.get("attention_bias"):
        refuse(f"with attention_bias={config['attention_bias']!r}: q/k norms and q/k/v/o biases together are not implemented")
    hd, W, L = config["head_dim"], config["sliding_window"], config["num_hidden_layers"]
    if not (isinstance(hd, int) and not isinstance(hd, bool) and 16 <= hd <= 256 and hd & (hd - 1) == 0):
        refuse(f"with head_dim={hd!r}: the q/k norm kernels take a power of two from 16 to 256")
    if not (isinstance(W, int) and not isinstance(W, bool) and W >= 1):
        refuse(f"with sliding_window={W!r}: a positive integer")
    if not _is_pos_number(config["query_pre_attn_scalar"]) or config["query_pre_attn_scalar"] != hd:
        refuse(f"with query_pre_attn_scalar={config['query_pre_attn_scalar']!r} != head_dim: the uncapped attention kernels scale "
               "by head_dim ** -0.5")
    lt = config.get("layer_types")
    if lt is not None:
        if len(lt) != L or any(t not in ("sliding_attention", "full_attention") for t in lt):
            refuse(f"with layer_types={lt!r}: {L} entries of 'sliding_attention' / 'full_attention'")
        sliding = [t == "sliding_attention" for t in lt]
    else:
        pat = config["sliding_window_pattern"]
        if not (isinstance(pat, int) and not isinstance(pat, bool) and pat >= 1):
            refuse(f"with sliding_window_pattern={pat!r}: a positive integer")
        sliding = [(i + 1) % pat != 0 for i in range(L)]
    if v5:
        g, loc = rp["full_attention"], rp["sliding_attention"]
        theta_g, theta_l = g.get("rope_theta"), loc.get("rope_theta")
        if (loc.get("rope_type") or loc.get("type") or "default") != "default":
            refuse(f"with rope_parameters['sliding_attention']={loc!r}: the sliding layers rotate unscaled")
        scaling = g
    else:
        theta_g, theta_l, scaling = config.get("rope_theta", 1000000.0), config["rope_local_base_freq"], config.get("rope_scaling")
    if not _is_pos_number(theta_g) or not _is_pos_number(theta_l):
        refuse(f"with rotary bases {theta_g!r} (global) and {theta_l!r} (sliding): positive finite numbers")
    factor = None
    if scaling is not None:
        kind = (scaling.get("rope_type") or scaling.get("type") or "default") if isinstance(scaling, dict) else scaling
        if kind == "linear":
            factor = scaling.get("factor")
            if not _is_pos_number(factor):
                refuse(f"with rope scaling {scaling!r}: rope_type 'linear' needs a positive finite factor")
        elif kind != "default":
            refuse(f"with rope scaling {scaling!r}: the global layers' table implements plain RoPE and rope_type 'linear' only")
    return dict(window=W, sliding=sliding, theta_global=float(theta_g), theta_local=float(theta_l),
                factor=float(factor) if factor is not None else None)


def model_family(config: dict) -> str:
    """'llama', 'gemma', 'gemma2', 'gemma3', 'phi3', 'qwen2' or 'qwen3' for a HF config dict (a missing model_type means llama); anything else raises:
    the kernels implement those families' arithmetic only, and a checkpoint of another family would load (same tensor names)
    and then score silently wrong. A gemma2, phi3 or qwen2 config is accepted only when it is complete (GEMMA2_REQUIRED_KEYS,
    PHI3_REQUIRED_KEYS, QWEN2_REQUIRED_KEYS). phi3 is Llama's arithmetic behind fused qkv_proj / gate_up_proj Linears
    (from_state_dict splits them); qwen2 is Llama's arithmetic with q/k/v biases (lr_llama_set_qkv_bias); qwen3 (complete by
    QWEN3_REQUIRED_KEYS; the dense models only) is Llama's arithmetic with per-head q/k RMSNorms (lr_llama_set_qk_norm); gemma3
    (model_type "gemma3_text", complete by gemma3_parameters) is Gemma's with sandwich norms, (1 + w) q/k norms, sliding-window
    layers and a rotary table per layer kind (lr_llama_set_gemma3)."""
    mt = config.get("model_type") or "llama"
    if mt in LLAMA_FAMILY:
        rope_parameters(config)   # plain RoPE or a complete llama3 rule; raises otherwise
        return "llama"
    if mt in GEMMA_FAMILY:
        if rope_parameters(config)[1] is not None:
            raise NotImplementedError(f"gemma with rope_scaling={config.get('rope_scaling') or config.get('rope_parameters')!r}: "
                                      "scaled RoPE is implemented for the llama family only")
        act = config.get("hidden_activation") or config.get("hidden_act") or "gelu_pytorch_tanh"
        if act not in ("gelu_pytorch_tanh", "gelu"):
            raise NotImplementedError(f"gemma with hidden_activation={act!r}: the kernels implement gelu_pytorch_tanh")
        return "gemma"
    supported = f"supported families: {', '.join(SUPPORTED_MODEL_TYPES)}"
    if mt in GEMMA3_FAMILY:
        gemma3_parameters(config)   # complete and computable, or NotImplementedError
        return "gemma3"
    if mt == "gemma3":
        raise NotImplementedError(f"model_type 'gemma3' is the multimodal wrapper (vision tower + text model): the ranker serves "
                                  f"the text-only checkpoints, model_type 'gemma3_text' (google/gemma-3-1b-pt, -1b-it); {supported}")
    if mt in GEMMA2_FAMILY:
        missing = [k for k in GEMMA2_REQUIRED_KEYS if k not in config or (config[k] is None and "softcapping" not in k)]
        if missing:
            raise NotImplementedError(f"model_type {mt!r} config lacks {', '.join(missing)}: soft caps, score scale, window "
                                      f"and head_dim have no defaults the kernels could assume; {supported}")
        act = config.get("hidden_activation") or config.get("hidden_act")
        if act != "gelu_pytorch_tanh":
            raise NotImplementedError(f"model_type {mt!r} with hidden_activation={act!r}: the kernels implement "
                                      f"gelu_pytorch_tanh; {supported}")
        if rope_parameters(config)[1] is not None:
            raise NotImplementedError(f"model_type {mt!r} with rope_scaling="
                                      f"{config.get('rope_scaling') or config.get('rope_parameters')!r}: scaled RoPE is "
                                      f"implemented for the llama family only; {supported}")
        for k in ("attn_logit_softcapping", "final_logit_softcapping", "query_pre_attn_scalar"):
            v = config[k]
            if v is not None and not (isinstance(v, (int, float)) and 0 < v < float("inf")):
                raise NotImplementedError(f"model_type {mt!r} with {k}={v!r}: a positive finite number"
                                          f"{' or null' if 'softcapping' in k else ''}; {supported}")
        if config["attn_logit_softcapping"] is None and config["query_pre_attn_scalar"] != config["head_dim"]:
            raise NotImplementedError(f"model_type {mt!r} with query_pre_attn_scalar={config['query_pre_attn_scalar']!r} != "
                                      f"head_dim and no attn_logit_softcapping: the uncapped attention kernels scale by "
                                      f"head_dim ** -0.5; {supported}")
        return "gemma2"
    if mt in PHI3_FAMILY:
        missing = [k for k in PHI3_REQUIRED_KEYS if k not in config or (config[k] is None and k != "sliding_window")]
        if missing:
            raise NotImplementedError(f"model_type {mt!r} config lacks {', '.join(missing)}: a Phi-3 config.json spells them "
                                      f"out, and the kernels assume no defaults for them; {supported}")
        if config["hidden_act"] != "silu":
            raise NotImplementedError(f"model_type {mt!r} with hidden_act={config['hidden_act']!r}: the kernels implement "
                                      f"silu (SwiGLU); {supported}")
        try:
            scaled = rope_parameters(config)[1] is not None   # longrope / su raise here
        except NotImplementedError as e:
            raise NotImplementedError(f"model_type {mt!r} with {e}; {supported}") from None
        if scaled:
            raise NotImplementedError(f"model_type {mt!r} with rope_scaling="
                                      f"{config.get('rope_scaling') or config.get('rope_parameters')!r}: Phi-3 is served "
                                      f"with plain RoPE only (no longrope / Phi-3-128k); {supported}")
        prf = config.get("partial_rotary_factor")
        if prf is None and isinstance(config.get("rope_parameters"), dict):
            prf = config["rope_parameters"].get("partial_rotary_factor")
        if prf is not None and prf != 1:
            raise NotImplementedError(f"model_type {mt!r} with partial_rotary_factor={prf!r}: the rotary epilogue rotates the "
                                      f"whole head; {supported}")
        sw = config["sliding_window"]
        if sw is not None and not (isinstance(sw, int) and sw > 0):
            raise NotImplementedError(f"model_type {mt!r} with sliding_window={sw!r}: a positive integer or null; {supported}")
        return "phi3"
    if mt in QWEN2_FAMILY:
        missing = [k for k in QWEN2_REQUIRED_KEYS if k not in config or (config[k] is None and k != "sliding_window")]
        if missing:
            raise NotImplementedError(f"model_type {mt!r} config lacks {', '.join(missing)}: a Qwen2 config.json spells them "
                                      f"out, and the kernels assume no defaults for them; {supported}")
        if config["hidden_act"] != "silu":
            raise NotImplementedError(f"model_type {mt!r} with hidden_act={config['hidden_act']!r}: the kernels implement "
                                      f"silu (SwiGLU); {supported}")
        try:
            scaled = rope_parameters(config)[1] is not None   # yarn, dynamic, ... raise here
        except NotImplementedError as e:
            raise NotImplementedError(f"model_type {mt!r} with {e}; {supported}") from None
        if scaled:
            raise NotImplementedError(f"model_type {mt!r} with rope_scaling="
                                      f"{config.get('rope_scaling') or config.get('rope_parameters')!r}: Qwen2 is served "
                                      f"with plain RoPE only; {supported}")
        hd = config.get("head_dim")
        if hd is not None and hd != config["hidden_size"] // config["num_attention_heads"]:
            raise NotImplementedError(f"model_type {mt!r} with head_dim={hd!r} != hidden_size / num_attention_heads = "
                                      f"{config['hidden_size'] // config['num_attention_heads']}; {supported}")
        if not isinstance(config["use_sliding_window"], bool):
            raise NotImplementedError(f"model_type {mt!r} with use_sliding_window={config['use_sliding_window']!r}: true or "
                                      f"false; {supported}")
        sw = config["sliding_window"]
        if config["use_sliding_window"] and not (isinstance(sw, int) and not isinstance(sw, bool) and sw > 0):
            raise NotImplementedError(f"model_type {mt!r} with use_sliding_window and sliding_window={sw!r}: a positive "
                                      f"integer; {supported}")
        return "qwen2"
    if mt in QWEN3_FAMILY:
        missing = [k for k in QWEN3_REQUIRED_KEYS if config.get(k) is None]
        if missing:
            raise NotImplementedError(f"model_type {mt!r} config lacks {', '.join(missing)}: a Qwen3 config.json spells them "
                                      f"out, and the kernels assume no defaults for them; {supported}")
        hd = config["head_dim"]
        if not (isinstance(hd, int) and not isinstance(hd, bool) and 16 <= hd <= 256 and hd & (hd - 1) == 0):
            raise NotImplementedError(f"model_type {mt!r} with head_dim={hd!r}: the q/k norm kernels take a power of two from "
                                      f"16 to 256; {supported}")
        if config["hidden_act"] != "silu":
            raise NotImplementedError(f"model_type {mt!r} with hidden_act={config['hidden_act']!r}: the kernels implement "
                                      f"silu (SwiGLU); {supported}")
        if config["attention_bias"] is not False:
            raise NotImplementedError(f"model_type {mt!r} with attention_bias={config['attention_bias']!r}: q/k norms and "
                                      f"q/k/v/o biases together are not implemented; {supported}")
        if config.get("use_sliding_window"):
            raise NotImplementedError(f"model_type {mt!r} with use_sliding_window={config['use_sliding_window']!r}: the "
                                      f"kernels attend to the whole causal range; {supported}")
        lt = config.get("layer_types")
        if lt is not None and any(t != "full_attention" for t in lt):
            raise NotImplementedError(f"model_type {mt!r} with layer_types={sorted(set(lt))!r}: every layer must be "
                                      f"full_attention; {supported}")
        try:
            scaled = rope_parameters(config)[1] is not None   # yarn, dynamic, ... raise here
        except NotImplementedError as e:
            raise NotImplementedError(f"model_type {mt!r} with {e}; {supported}") from None
        if scaled:
            raise NotImplementedError(f"model_type {mt!r} with rope_scaling="
                                      f"{config.get('rope_scaling') or config.get('rope_parameters')!r}: Qwen3 is served "
                                      f"with plain RoPE only; {supported}")
        return "qwen3"
    if mt == "qwen3_moe":
        raise NotImplementedError(f"model_type 'qwen3_moe': the mixture-of-experts Qwen3 models have no kernels here (the "
                                  f"dense ones are model_type 'qwen3'); {supported}")
    raise NotImplementedError(f"model_type {mt!r} is not supported by the ranker's kernels; supported families: "
                              f"{', '.join(SUPPORTED_MODEL_TYPES)}")


@dataclass
class CausalLMOutput:
    """Subset of transformers' CausalLMOutputWithPast that the scoring path reads."""
    loss: torch.Tensor | None
    logits: torch.Tensor
    past_key_values: None = None
    hidden_states: None = None
    attentions: None = None

    def __getitem__(self, i):
        return ((self.loss, self.logits) if self.loss is not None else (self.logits,))[i]


def pack_prompts(seqs) -> tuple[np.ndarray, np.ndarray]:
    """list of token-id sequences -> (packed int32 ids, cu_seqlens int32 [B+1])."""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    if (lens < 1).any():
        raise ValueError("empty prompt")
    cu = np.zeros(len(seqs) + 1, np.int32)
    cu[1:] = np.cumsum(lens)
    ids = np.concatenate([np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs])
    return ids, cu


def common_prefix_len(ids: np.ndarray, cu: np.ndarray) -> int:
    """Length of the longest token prefix shared by ALL prompts of a packed batch, capped at min(T) - 1 so every prompt
    keeps at least one token of its own (0 for a single prompt: nothing to share)."""
    B = len(cu) - 1
    if B < 2:
        return 0
    lens = np.diff(cu)
    n = int(lens.min()) - 1
    if n <= 0:
        return 0
    head = ids[cu[0]: cu[0] + n]
    for b in range(1, B):
        neq = np.nonzero(ids[cu[b]: cu[b] + n] != head[:n])[0]
        if neq.size:
            n = int(neq[0])
            if n == 0:
                return 0
    return n


def unpad_left(input_ids, attention_mask=None):
    """Left-padded [B,T] batch (trainer/llm.py:34-37 pads ids with 0, mask with 0) -> list of
    per-prompt id arrays."""
    ids = np.asarray(input_ids.cpu() if isinstance(input_ids, torch.Tensor) else input_ids)
    if attention_mask is None:
        return [row for row in ids]
    m = np.asarray(attention_mask.cpu() if isinstance(attention_mask, torch.Tensor) else attention_mask)
    out = []
    for r, mr in zip(ids, m):
        n = int(mr.sum())
        if n and not mr[-n:].all():
            raise ValueError("attention_mask must be left padding (ones form a suffix)")
        out.append(r[len(r) - n:])
    return out


# the Linears of a decoder layer an adapter may sit on (_abi.LORA_MODULES: the one list, in the kernels' order) -> HF block
LORA_MODULE_BLOCK = {m: "mlp" if m in ("gate_proj", "up_proj", "down_proj") else "self_attn" for m in A.LORA_MODULES}
_LORA_KEY = re.compile(r"^model\.layers\.(\d+)\.(self_attn|mlp)\.([a-z]+_proj)\.lora_([AB])\.weight$")


def expand_target_modules(target_modules):
    """peft's `target_modules` (a list of names, or the string "all-linear") -> tuple of names in the kernels' order.
    A name that is no Linear of a Llama decoder layer (phi-3's fused qkv_proj, lm_head, ...) raises."""
    if isinstance(target_modules, str):
        target_modules = [target_modules]
    names = set()
    for m in target_modules or ():
        names.update(LORA_MODULE_BLOCK if m == "all-linear" else [m])
    bad = sorted(names - set(LORA_MODULE_BLOCK))
    if bad:
        raise NotImplementedError(f"target_modules {bad}: adapters are supported on {', '.join(LORA_MODULE_BLOCK)}")
    if not names:
        raise ValueError("target_modules is empty")
    return tuple(m for m in LORA_MODULE_BLOCK if m in names)


def check_adapter_config(ac):
    """adapter_config.json -> (r, alpha, target modules). Anything that changes what W + (alpha/r) B A means is refused by the
    name of its field (it would otherwise load and score silently wrong); missing optional keys take peft's defaults."""
    def refuse(field, why):
        raise NotImplementedError(f"adapter_config.json: {field}={ac.get(field)!r}: {why}")

    if str(ac.get("peft_type", "LORA")).upper() != "LORA":
        refuse("peft_type", "only LoRA adapters are merged at load")
    if ac.get("use_dora", False):
        refuse("use_dora", "DoRA's magnitude vectors are not implemented")
    if ac.get("use_rslora", False):
        refuse("use_rslora", "the scaling is alpha / r, not alpha / sqrt(r)")
    for field in ("rank_pattern", "alpha_pattern"):
        if ac.get(field):
            refuse(field, "per-module ranks / alphas are not implemented")
    if ac.get("bias", "none") != "none":
        refuse("bias", "trained biases are not implemented (the base Linears have none)")
    if ac.get("fan_in_fan_out", False):
        refuse("fan_in_fan_out", "transposed base weights are not implemented")
    if ac.get("modules_to_save"):
        refuse("modules_to_save", "fully trained copies of base modules are not implemented")
    if "r" not in ac or "lora_alpha" not in ac:
        raise ValueError("adapter_config.json: r and lora_alpha are required")
    tm = ac.get("target_modules")
    return ac["r"], ac["lora_alpha"], (expand_target_modules(tm) if tm else None)


def adapter_weights(tensors, r, target_modules=None):
    """{PEFT tensor name: array} -> {"model.layers.{l}.{block}.{module}.lora_{A,B}.weight": fp32 array}. Every tensor must belong
    to a Linear of a decoder layer (one of `target_modules` when the config names them), have rank r, and come as an A/B pair."""
    w = {}
    for k, v in tensors.items():
        name = k.replace("base_model.model.", "", 1).replace(".default", "")
        m = _LORA_KEY.match(name)
        if not m or LORA_MODULE_BLOCK.get(m.group(3)) != m.group(2):
            raise NotImplementedError(f"adapter tensor {k!r} maps to no Linear of a decoder layer "
                                      f"({', '.join(LORA_MODULE_BLOCK)})")
        if target_modules is not None and m.group(3) not in target_modules:
            raise ValueError(f"adapter tensor {k!r} is not among adapter_config.json's target_modules {list(target_modules)}")
        v = np.asarray(v, dtype=np.float32)
        if v.ndim != 2 or v.shape[0 if m.group(4) == "A" else 1] != r:
            raise ValueError(f"adapter tensor {k!r} has shape {v.shape}: rank {r} expected")
        w[name] = v
    for name in w:
        other = name.replace("lora_A", "lora_B") if "lora_A" in name else name.replace("lora_B", "lora_A")
        if other not in w:
            raise ValueError(f"adapter tensor {name!r} has no partner {other!r}")
    return w


def load_peft_adapter(adapter_path):
    """A local PEFT LoRA directory (adapter_config.json + adapter_model.safetensors) -> the `lora` argument of
    LlamaRanker.from_state_dict. Runs on the host alone."""
    from safetensors import safe_open

    r, alpha, modules = check_adapter_config(json.load(open(os.path.join(adapter_path, "adapter_config.json"))))
    t = {}
    with safe_open(os.path.join(adapter_path, "adapter_model.safetensors"), framework="pt", device="cpu") as f:
        for k in f.keys():
            t[k] = f.get_tensor(k).float().numpy()
    return dict(r=r, alpha=alpha, weights=adapter_weights(t, r, modules), target_modules=modules)


class PromptCache:
    """LlamaRanker.new_prompt_cache: `table` is the device table [num_slots][slot_bytes] of rotated keys and values
    (include/llamarec_mi355x.h, lr_llama_extend_verbalize), `ids[s]` the token ids slot s holds rows for. The table has no
    device-side length: ids is the only record, and shortening ids[s] is the whole of a rollback."""

    def __init__(self, table, num_slots, max_tokens):
        self.table, self.num_slots, self.max_tokens = table, num_slots, max_tokens
        self.ids = [[] for _ in range(num_slots)]


class LlamaRanker:
    """One replica of the ranker's weights on one MI355X + the prefill/verbalizer entry points."""

    def __init__(self, config: dict, device="cuda:0"):
        self.config = dict(config)
        self.device = torch.device(device)
        c = self.config
        self.family = model_family(c)
        if self.family == "gemma3":   # two tables per call (lr_llama_set_gemma3); the handle's rope_theta is the global layers'
            self.gemma3 = gemma3_parameters(c)
            self.rope_theta, self.rope_scaling = self.gemma3["theta_global"], None
        else:
            self.rope_theta, self.rope_scaling = rope_parameters(c)   # scaling: None (plain RoPE) or the llama3 numbers
        self.hd = c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"]
        # Mistral's sliding window: the kernels attend to the whole causal range, so a longer prompt is refused
        # (Gemma-2: its even layers' window; within it the window is the plain causal mask)
        # (Phi-3: every layer's window, 2047 for mini-4k; null means none)
        # (Qwen2: only with use_sliding_window, then on the layers from max_window_layers on; false: the window is ignored)
        # (Gemma-3: its sliding layers ARE windowed -- lr_llama_set_gemma3 -- so nothing is refused for length)
        windowed = (c.get("model_type") == "mistral" or self.family in ("gemma2", "phi3")
                    or (self.family == "qwen2" and c["use_sliding_window"]))
        self.max_prompt_len = c.get("sliding_window") if windowed else None
        self._window_owner = {"gemma2": "Gemma-2", "phi3": "Phi-3", "qwen2": "Qwen2"}.get(self.family, "Mistral")
        self._h = C.c_void_p()
        self._tensors = {}
        self._ws = None
        self._layers_arr = None
        self._folded_arr = None
        # RMSNorm folded into the next projection (set_fold_norms): OFF by default. Numerically it is one more valid bf16
        # realisation (as close to the fp32 oracle as the separate pass: tools/parity_growth.py), but on this GEMM it does
        # not pay: the norm passes it removes (2.6 ms of a 163 ms step) cost less than the rstd sweep (1.3 ms) plus the
        # epilogue's dependent rstd load, which nothing hides at one workgroup per CU (GEMMs 1370 -> 1347 TF/s):
        # 164.2 vs 163.5 ms per step in a same-box A/B
        self.fold_norms = False
        self.training = False
        # Qwen2's widths may miss the 256-column GEMM tile (0.5B: 896 and 1152): its default GEMM variant is 6, auto with a
        # ragged last column tile (set_variants overrides it; no other family's default changes)
        # (Gemma-3 too: gemma-3-1b's hidden width 1152 misses it)
        self.default_gemm_variant = 6 if self.family in ("qwen2", "gemma3") else 0

    # -- construction ------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, state_dict, config, device="cuda:0", lora=None, nf4=False):
        """state_dict: HF LlamaForCausalLM names -> torch tensors / numpy arrays (any float dtype).
        lora: optional dict(r=8, alpha=32, weights={"...q_proj.lora_A.weight": A, "...lora_B.weight": B}).
        nf4: pass every Linear of the base through the NF4 + double-quantisation round trip first, like the
        reference's BitsAndBytesConfig (train_ranker.py:49-56; lm_head, embeddings and norms stay as they are --
        bitsandbytes skips lm_head); the adapter is merged AFTER it, as peft adds it to the dequantised output."""
        self = cls(config, device)
        dev = self.device
        scratch = {}

        def nf4_roundtrip(w):
            w = w.to(torch.bfloat16).contiguous()
            need = lib().lr_nf4_scratch_bytes(w.numel())
            if scratch.get("n", 0) < need:
                scratch["buf"], scratch["n"] = torch.empty(need, dtype=torch.uint8, device=dev), need
            with torch.cuda.device(dev):
                check(lib().lr_nf4_roundtrip_bf16(w.data_ptr(), w.numel(), 1, w.data_ptr(), scratch["buf"].data_ptr(),
                                                  scratch["n"], stream_ptr()), "lr_nf4_roundtrip_bf16")
            return w

        def t(name):
            w = state_dict[name]
            if not isinstance(w, torch.Tensor):
                w = torch.from_numpy(np.ascontiguousarray(w))
            return w.to(dev)

        def linear(name):
            return nf4_roundtrip(t(name)) if nf4 else t(name)

        def merged(name):
            w = linear(name).float()
            if lora is not None:
                base = name[: -len(".weight")]
                ka, kb = base + ".lora_A.weight", base + ".lora_B.weight"
                if ka in lora["weights"]:
                    a = torch.as_tensor(np.asarray(lora["weights"][ka])).to(dev).float()
                    b = torch.as_tensor(np.asarray(lora["weights"][kb])).to(dev).float()
                    w = w + (lora["alpha"] / lora["r"]) * (b @ a)
            return w

        L = config["num_hidden_layers"]
        if lora is not None:   # a key no Linear below would pick up (another layer count, lm_head, ...) must not vanish silently
            known = {f"model.layers.{i}.{blk}.{m}.lora_{ab}.weight" for i in range(L) for m, blk in LORA_MODULE_BLOCK.items()
                     for ab in "AB"}
            stray = sorted(set(lora["weights"]) - known)
            if stray:
                raise NotImplementedError(f"adapter tensors that map to no Linear of this model's decoder layers: {stray[:4]}")
        phi3 = self.family == "phi3"
        if phi3:
            if lora is not None and lora["weights"]:   # a Phi-3 checkpoint has no separate q_proj ... for an adapter to target
                raise NotImplementedError("adapter tensors that map to no Linear of this model's decoder layers: a phi3 base "
                                          f"stores fused qkv_proj / gate_up_proj Linears: {sorted(lora['weights'])[:4]}")
            if config.get("tie_word_embeddings") and "lm_head.weight" not in state_dict:
                raise NotImplementedError("model_type 'phi3' with tie_word_embeddings and no lm_head.weight: Phi-3's head is "
                                          "untied")
            nh, nkv = config["num_attention_heads"], config["num_key_value_heads"]

            def split_rows(name, sizes):
                """The fused Linear as stored (NF4 round trip included: bitsandbytes quantises it whole), cut into row blocks"""
                w = merged(name)
                if w.shape[0] != sum(sizes):
                    raise ValueError(f"{name}: {w.shape[0]} rows, expected {' + '.join(map(str, sizes))}")
                return torch.split(w, sizes, 0)
        T = self._tensors
        if self.family == "qwen2":
            for i in range(L):
                for n in "qkv":
                    if f"model.layers.{i}.self_attn.{n}_proj.bias" not in state_dict:
                        raise KeyError(f"model_type 'qwen2': model.layers.{i}.self_attn.{n}_proj.bias is missing (Qwen2's "
                                       "q/k/v Linears have biases)")
        if self.family in ("qwen3", "gemma3"):
            owner = "Qwen3" if self.family == "qwen3" else "Gemma-3"
            for i in range(L):
                for n in "qk":
                    if f"model.layers.{i}.self_attn.{n}_norm.weight" not in state_dict:
                        raise KeyError(f"model_type {config.get('model_type')!r}: model.layers.{i}.self_attn.{n}_norm.weight is "
                                       f"missing ({owner} norms every q and k head)")
        T["embed"] = t("model.embed_tokens.weight").to(torch.bfloat16).contiguous()
        T["final_norm"] = t("model.norm.weight").to(torch.bfloat16).contiguous()
        T["lm_head"] = (t("lm_head.weight") if "lm_head.weight" in state_dict else T["embed"]).to(torch.bfloat16).contiguous()
        for i in range(L):
            p = f"model.layers.{i}."
            if phi3:
                # q | k | v rows of qkv_proj; gate | up halves of gate_up_proj (HF: up * silu(gate) of chunk(2))
                q, k, v = split_rows(p + "self_attn.qkv_proj.weight", [nh * self.hd, nkv * self.hd, nkv * self.hd])
                gate, up = split_rows(p + "mlp.gate_up_proj.weight", [config["intermediate_size"]] * 2)
            else:
                q, k, v = (merged(p + f"self_attn.{n}_proj.weight") for n in "qkv")
                gate, up = merged(p + "mlp.gate_proj.weight"), merged(p + "mlp.up_proj.weight")
            T[f"{i}.wqkv"] = torch.cat([self._interleave_rope_rows(q), self._interleave_rope_rows(k), v],
                                       0).to(torch.bfloat16).contiguous()
            if self.family == "qwen2":
                # the biases in wqkv's row order: q and k through the same pair interleave as the weight rows, v plain. They
                # stay out of the NF4 round trip (bitsandbytes quantises weights only) and no adapter touches them.
                bq, bk, bv = (t(p + f"self_attn.{n}_proj.bias").float().reshape(-1, 1) for n in "qkv")
                T[f"{i}.bqkv"] = torch.cat([self._interleave_rope_rows(bq), self._interleave_rope_rows(bk), bv],
                                           0).reshape(-1).to(torch.bfloat16).contiguous()
            if self.family in ("qwen3", "gemma3"):
                # the [head_dim] norm weights in a head's packed column order: the permutation of a head's rows of wq / wk,
                # once at load. They stay out of the NF4 round trip (Linears only) and no adapter touches them.
                for n in "qk":
                    wn = t(p + f"self_attn.{n}_norm.weight").float().reshape(-1, 1)
                    if wn.shape[0] != self.hd:
                        raise ValueError(f"{p}self_attn.{n}_norm.weight: {wn.shape[0]} elements, expected head_dim = {self.hd}")
                    T[f"{i}.{n}_norm"] = self._interleave_rope_rows(wn).reshape(-1).to(torch.bfloat16).contiguous()
            T[f"{i}.wo"] = merged(p + "self_attn.o_proj.weight").to(torch.bfloat16).contiguous()
            T[f"{i}.wgu"] = self._interleave_gate_up(gate, up)
            T[f"{i}.wdown"] = merged(p + "mlp.down_proj.weight").to(torch.bfloat16).contiguous()
            T[f"{i}.input_norm"] = t(p + "input_layernorm.weight").to(torch.bfloat16).contiguous()
            if self.family in ("gemma2", "gemma3"):
                # LrLlamaLayerWeights.post_norm is the norm in FRONT of the MLP: Gemma-2's pre_feedforward_layernorm. HF's
                # post_attention_layernorm acts on the attention output there (LrGemma2Ext.attn_out_norm).
                T[f"{i}.post_norm"] = t(p + "pre_feedforward_layernorm.weight").to(torch.bfloat16).contiguous()
                T[f"{i}.attn_out_norm"] = t(p + "post_attention_layernorm.weight").to(torch.bfloat16).contiguous()
                T[f"{i}.mlp_out_norm"] = t(p + "post_feedforward_layernorm.weight").to(torch.bfloat16).contiguous()
            else:
                T[f"{i}.post_norm"] = t(p + "post_attention_layernorm.weight").to(torch.bfloat16).contiguous()
        self._create()
        return self

    @classmethod
    def random_init(cls, config, seed=42, std=0.02, device="cuda:0"):
        """Random bf16 weights ~ N(0, std) generated directly on the GPU (BASELINE.md section 3:
        no checkpoints exist offline). Norm weights are ones."""
        self = cls(config, device)
        c, dev = self.config, self.device
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        d, f, v = c["hidden_size"], c["intermediate_size"], c["vocab_size"]
        nh, nkv, hd = c["num_attention_heads"], c["num_key_value_heads"], self.hd

        def rnd(*shape):
            return (torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * std).to(torch.bfloat16)

        T = self._tensors
        # unit norm scale: w = 1 for Llama, w = 0 for Gemma's (1 + w); Gemma's lm_head is the (tied) embedding
        gemma = self.family in ("gemma", "gemma2", "gemma3")
        norm = torch.zeros if gemma else torch.ones
        T["embed"] = rnd(v, d)
        T["final_norm"] = norm(d, dtype=torch.bfloat16, device=dev)
        T["lm_head"] = T["embed"] if gemma else rnd(v, d)
        for i in range(c["num_hidden_layers"]):
            T[f"{i}.wqkv"] = rnd((nh + 2 * nkv) * hd, d)
            if self.family == "qwen2":
                T[f"{i}.bqkv"] = rnd((nh + 2 * nkv) * hd)
            if self.family in ("qwen3", "gemma3"):
                T[f"{i}.q_norm"] = norm(hd, dtype=torch.bfloat16, device=dev)
                T[f"{i}.k_norm"] = norm(hd, dtype=torch.bfloat16, device=dev)
            T[f"{i}.wo"] = rnd(d, nh * hd)
            T[f"{i}.wgu"] = rnd(2 * f, d)  # already in the interleaved gate/up layout (random anyway)
            T[f"{i}.wdown"] = rnd(d, f)
            T[f"{i}.input_norm"] = norm(d, dtype=torch.bfloat16, device=dev)
            T[f"{i}.post_norm"] = norm(d, dtype=torch.bfloat16, device=dev)
            if self.family in ("gemma2", "gemma3"):
                T[f"{i}.attn_out_norm"] = norm(d, dtype=torch.bfloat16, device=dev)
                T[f"{i}.mlp_out_norm"] = norm(d, dtype=torch.bfloat16, device=dev)
        self._create()
        return self

    @classmethod
    def from_pretrained(cls, path, device="cuda:0", adapter_path=None, load_in_4bit=False):
        """Local HF directory (config.json + *.safetensors), optionally a PEFT LoRA adapter directory
        (adapter_config.json + adapter_model.safetensors) merged at load. load_in_4bit: the reference's NF4 round trip
        of the base Linears (see from_state_dict). The family follows config.json's model_type (model_family).
        No network access."""
        from safetensors import safe_open

        cfg = json.load(open(os.path.join(path, "config.json")))
        model_family(cfg)   # refuse an unsupported checkpoint before reading gigabytes of it
        sd = {}
        for fn in sorted(os.listdir(path)):
            if fn.endswith(".safetensors"):
                with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as f:
                    for k in f.keys():
                        sd[k] = f.get_tensor(k)
        return cls.from_state_dict(sd, cfg, device, load_peft_adapter(adapter_path) if adapter_path else None,
                                   nf4=load_in_4bit)

    def _interleave_rope_rows(self, w):
        """Rows of every head reordered to (0, hd/2, 1, hd/2+1, ...): rotation pairs become adjacent
        output columns for the fused rotary epilogue (== lr_llama_pack_qkv)."""
        hd = self.hd
        heads = w.shape[0] // hd
        return w.view(heads, 2, hd // 2, w.shape[1]).transpose(1, 2).reshape(heads * hd, w.shape[1])

    @staticmethod
    def _interleave_gate_up(gate, up):
        f, d = gate.shape
        if f % 16:
            raise ValueError("intermediate_size must be a multiple of 16")
        g = gate.to(torch.bfloat16).view(f // 16, 16, d)
        u = up.to(torch.bfloat16).view(f // 16, 16, d)
        return torch.stack([g, u], dim=1).reshape(2 * f, d).contiguous()

    def arch(self):
        """The LrLlamaArch of this ranker's family (include/llamarec_mi355x.h)."""
        if self.family in ("gemma", "gemma2", "gemma3"):
            # HF GemmaModel / Gemma2Model / Gemma3TextModel: hidden * torch.tensor(hidden_size ** 0.5, dtype=bf16)
            scale = float(torch.tensor(self.config["hidden_size"] ** 0.5, dtype=torch.bfloat16))
            return A.LrLlamaArch(norm_style=1, mlp_act=1, embed_scale=scale)
        return A.LrLlamaArch(norm_style=0, mlp_act=0, embed_scale=1.0)

    def _create(self):
        c, T = self.config, self._tensors
        cfg = A.LrLlamaConfig(
            vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
            num_layers=c["num_hidden_layers"], num_heads=c["num_attention_heads"],
            num_kv_heads=c["num_key_value_heads"], head_dim=self.hd,
            max_positions=int(c.get("max_position_embeddings", 4096)), rms_eps=float(c["rms_norm_eps"]),
            rope_theta=self.rope_theta)
        L = c["num_hidden_layers"]
        arr = (A.LrLlamaLayerWeights * L)()
        for i in range(L):
            for field in ("input_norm", "wqkv", "wo", "post_norm", "wgu", "wdown"):
                setattr(arr[i], field, T[f"{i}.{field}"].data_ptr())
        desc = A.LrLlamaWeightsDesc(embed=T["embed"].data_ptr(), final_norm=T["final_norm"].data_ptr(),
                                    lm_head=T["lm_head"].data_ptr(), layers=arr)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            check(lib().lr_llama_create_ex(C.byref(cfg), C.byref(self.arch()), C.byref(desc), C.byref(h)), "lr_llama_create_ex")
        self._h, self._layers_arr = h, arr
        if self.rope_scaling is not None:
            rs = self.rope_scaling
            words = A.LrRopeScaling(kind=1, factor=float(rs["factor"]), low_freq_factor=float(rs["low_freq_factor"]),
                                    high_freq_factor=float(rs["high_freq_factor"]),
                                    original_max_positions=int(rs["original_max_position_embeddings"]))
            check(lib().lr_llama_set_rope_scaling(self._h, C.byref(words)), "lr_llama_set_rope_scaling")
        if self.family == "gemma2":
            ext, self._gemma2_arrs = self.gemma2_ext()
            check(lib().lr_llama_set_gemma2(self._h, C.byref(ext)), "lr_llama_set_gemma2")
        if "0.bqkv" in T:
            self._bqkv_arr = (C.c_void_p * L)(*[T[f"{i}.bqkv"].data_ptr() for i in range(L)])
            check(lib().lr_llama_set_qkv_bias(self._h, self._bqkv_arr), "lr_llama_set_qkv_bias")
        if self.family == "gemma3":
            ext, self._gemma3_arrs = self.gemma3_ext()
            check(lib().lr_llama_set_gemma3(self._h, C.byref(ext)), "lr_llama_set_gemma3")
        elif "0.q_norm" in T:
            self._qk_norm_arrs = ((C.c_void_p * L)(*[T[f"{i}.q_norm"].data_ptr() for i in range(L)]),
                                  (C.c_void_p * L)(*[T[f"{i}.k_norm"].data_ptr() for i in range(L)]))
            check(lib().lr_llama_set_qk_norm(self._h, *self._qk_norm_arrs), "lr_llama_set_qk_norm")
        if self.default_gemm_variant:
            self.set_variants(gemm=self.default_gemm_variant)
        if self.fold_norms:
            self.set_fold_norms(True)

    def gemma2_ext(self):
        """(LrGemma2Ext, the two pointer arrays it names) of a gemma2 ranker: caps, the score scale
        query_pre_attn_scalar ** -0.5 and, once the weights are loaded, the out-norms of the sandwich."""
        c, T, L = self.config, self._tensors, self.config["num_hidden_layers"]
        ext = A.LrGemma2Ext(attn_softcap=float(c["attn_logit_softcapping"] or 0.0),
                            final_softcap=float(c["final_logit_softcapping"] or 0.0),
                            attn_scale=float(c["query_pre_attn_scalar"]) ** -0.5)
        arrs = None
        if "0.attn_out_norm" in T:
            arrs = ((C.c_void_p * L)(*[T[f"{i}.attn_out_norm"].data_ptr() for i in range(L)]),
                    (C.c_void_p * L)(*[T[f"{i}.mlp_out_norm"].data_ptr() for i in range(L)]))
            ext.attn_out_norm, ext.mlp_out_norm = arrs
        return ext, arrs

    def gemma3_ext(self):
        """(LrGemma3Ext, the arrays it names) of a gemma3 ranker: window, layer kinds, the local rotary base, the global
        layers' linear factor and the four per-layer norm arrays."""
        g, T, L = self.gemma3, self._tensors, self.config["num_hidden_layers"]
        kinds = (C.c_uint8 * L)(*[1 if s else 0 for s in g["sliding"]])
        arrs = tuple((C.c_void_p * L)(*[T[f"{i}.{n}"].data_ptr() for i in range(L)])
                     for n in ("q_norm", "k_norm", "attn_out_norm", "mlp_out_norm"))
        ext = A.LrGemma3Ext(sliding_window=int(g["window"]), rope_theta_local=g["theta_local"],
                            global_linear_factor=float(g["factor"] or 0.0), attn_scale=0.0, layer_is_sliding=kinds)
        ext.q_norm, ext.k_norm, ext.attn_out_norm, ext.mlp_out_norm = arrs
        return ext, (kinds,) + arrs

    def set_fold_norms(self, enable=True):
        """Fold the two RMSNorms of every layer into the following projection (include/llamarec_mi355x.h,
        lr_llama_set_folded_norms): wqkv * diag(input_norm) and wgu * diag(post_norm) are built once on the GPU and
        kept beside the originals (+66 % of the q/k/v/gate/up bytes; the originals serve LoRA fine-tuning and the
        pruned last layer). Opt-in: see the note at LlamaRanker.fold_norms."""
        T, L = self._tensors, self.config["num_hidden_layers"]
        if enable and self.family in ("gemma", "gemma2", "gemma3"):
            raise NotImplementedError("folded norms: Gemma's (1 + w) RMSNorm cannot be folded into bf16 weights at HF's rounding")
        if enable and self.family == "qwen2":
            raise NotImplementedError("folded norms: not with Qwen2's q/k/v biases (lr_llama_set_qkv_bias)")
        if enable and self.family == "qwen3":
            raise NotImplementedError("folded norms: not with Qwen3's q/k norms (lr_llama_set_qk_norm)")
        if not enable:
            check(lib().lr_llama_set_folded_norms(self._h, None, None), "lr_llama_set_folded_norms")
            for i in range(L):
                T.pop(f"{i}.wqkv_folded", None)
                T.pop(f"{i}.wgu_folded", None)
            self._folded_arr = None
            self.fold_norms = False
            return self
        qa, ga = (C.c_void_p * L)(), (C.c_void_p * L)()
        with torch.cuda.device(self.device):
            for i in range(L):
                for name, norm, arr in (("wqkv", "input_norm", qa), ("wgu", "post_norm", ga)):
                    w = T[f"{i}.{name}"]
                    out = torch.empty_like(w)
                    check(lib().lr_fold_norm_bf16(w.data_ptr(), T[f"{i}.{norm}"].data_ptr(), w.shape[0], w.shape[1],
                                                  out.data_ptr(), stream_ptr()), "lr_fold_norm_bf16")
                    T[f"{i}.{name}_folded"] = out
                    arr[i] = out.data_ptr()
            torch.cuda.synchronize()
            check(lib().lr_llama_set_folded_norms(self._h, qa, ga), "lr_llama_set_folded_norms")
        self._folded_arr = (qa, ga)
        self.fold_norms = True
        return self

    def set_variants(self, gemm=0, attention=0):
        """Kernel selection (include/llamarec_mi355x.h): 0 = auto; gemm=5 = latency mode for the online
        single-user path (split-K where a short prompt would leave most CUs idle); gemm=6 = auto with the MFMA tile on a ragged
        last column tile (widths that are multiples of 64 but not of 256: a qwen2 ranker's default); gemm=7 = the row-invariant
        latency mode, the one to set for ranker sessions: 5 with the split fixed by the weight's shape and the rows launched in
        chunks, so a row's bits do not depend on the launch's row count -- extend_verbalize runs it and returns the bits of
        prefill_verbalize under 7, and up to 256 prompt tokens 7 is 5 bit for bit. It needs widths on the 256 x 64 tile (an error otherwise). A large batch under 7 is many serial launches:
        bulk scoring stays on auto. attention: 1 generic, 2 / 3 head_dim 128,
        4 head_dim 256, 5 head_dim 64 (scoring only: no lse), 7 head_dim 96 (scoring only: no lse), 6 = head_dim-64 MFMA attention for training (5's forward, writing
        lse when a LoRA engine runs on this base, and the head_dim-64 MFMA backward; the LoRA step's auto at head_dim 64),
        8 = the same pair at head_dim 96 (7's forward writing lse, the head_dim-96 MFMA backward; the LoRA step's auto at
        head_dim 96), 9 = the same pair at head_dim 256 (4's forward writing lse, the head_dim-256 MFMA backward; the LoRA
        step's auto at head_dim 256; no soft-capped form)."""
        check(lib().lr_llama_set_variants(self._h, gemm, attention), "lr_llama_set_variants")
        return self

    def set_last_layer_pruning(self, enable=True):
        check(lib().lr_llama_set_last_layer_pruning(self._h, int(bool(enable))), "lr_llama_set_last_layer_pruning")
        return self

    def eval(self):
        return self

    def __del__(self):
        try:
            if self._h.value:
                lib().lr_llama_destroy(self._h)
        except Exception:
            pass

    # -- scoring -----------------------------------------------------------------------------
    def _check_lengths(self, cu_host):
        if self.max_prompt_len is not None and int(np.diff(cu_host).max()) > self.max_prompt_len:
            raise NotImplementedError(f"a prompt of {int(np.diff(cu_host).max())} tokens exceeds {self._window_owner}'s sliding window of "
                                      f"{self.max_prompt_len}: the kernels attend to the whole causal range")

    def _workspace(self, n_tokens, n_seqs):
        need = lib().lr_llama_workspace_bytes(self._h, n_tokens, n_seqs)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _packed(self, seqs):
        ids, cu = pack_prompts(seqs)
        return (torch.from_numpy(ids).to(self.device), torch.from_numpy(cu).to(self.device), cu)

    def prefill_verbalize_packed(self, ids_dev, cu_dev, cu_host, label_ids_dev, out=None, prefix_len=0):
        """Device-resident inputs (the benchmark's timed region starts here). prefix_len > 0: the caller has checked
        (common_prefix_len on the host ids) that all prompts start with the same prefix_len tokens; they are then run
        once per batch (bit-identical scores, lr_llama_prefill_verbalize_prefix)."""
        B, Cn = len(cu_host) - 1, label_ids_dev.numel()
        self._check_lengths(cu_host)
        if out is None:
            out = torch.empty((B, Cn), dtype=torch.float32, device=self.device)
        ws = self._workspace(int(cu_host[-1]), B)
        with torch.cuda.device(self.device):
            check(lib().lr_llama_prefill_verbalize_prefix(
                self._h, ids_dev.data_ptr(), cu_dev.data_ptr(), cu_host.ctypes.data, B, int(prefix_len),
                label_ids_dev.data_ptr(), Cn, out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()),
                "lr_llama_prefill_verbalize_prefix")
        return out

    def prefill_verbalize(self, seqs, label_token_ids, share_prefix=True):
        """scores[b, c] = logit of label word c at the last token of prompt b (fp32 [B, C]). The prompts' common
        prefix (the template text) is evaluated once unless share_prefix is False."""
        ids_host, cu_host = pack_prompts(seqs)
        P = common_prefix_len(ids_host, cu_host) if share_prefix else 0
        lab = torch.as_tensor(np.asarray(label_token_ids, dtype=np.int32)).to(self.device)
        return self.prefill_verbalize_packed(torch.from_numpy(ids_host).to(self.device),
                                             torch.from_numpy(cu_host).to(self.device), cu_host, lab, prefix_len=P)

    # -- sessions: a per-user K / V cache of the prompt prefix (include/llamarec_mi355x.h, lr_llama_extend_verbalize) ------
    def new_prompt_cache(self, num_slots, max_tokens):
        """A table of `num_slots` slots of `max_tokens` prompt positions each, and the host list of the token ids every slot
        holds K / V rows for (PromptCache). Nothing is zeroed: a row is read only after a call has written it."""
        c = self.config
        slot_bytes = int(lib().lr_llama_kv_cache_slot_bytes(c["num_hidden_layers"], c["num_key_value_heads"], self.hd,
                                                            int(max_tokens)))
        if num_slots < 1 or slot_bytes == 0:
            raise ValueError(f"prompt cache: num_slots {num_slots}, max_tokens {max_tokens}")
        table = torch.empty((int(num_slots), slot_bytes), dtype=torch.uint8, device=self.device)
        return PromptCache(table, int(num_slots), int(max_tokens))

    def extend_verbalize(self, cache, slots, new_ids_list, label_token_ids, keep=None, cached_len=None):
        """scores[b, c] (fp32 [B, C]) of the prompts  cache.ids[slots[b]][:cached_len[b]] + new_ids_list[b]  at their last
        token, prefilling only the new ids. cached_len defaults to everything the slot holds; a smaller value rolls the
        slot back. keep[b] (default: all) leading new tokens count as cached afterwards. Bit-identical to
        prefill_verbalize of the whole prompts in the default GEMM mode, and under set_variants(7, 0) -- the mode for online
        use -- to prefill_verbalize under 7 (see the header for the attention variants; gemm variant 5 runs the default-mode
        products here)."""
        B = len(slots)
        seqs = [np.asarray(s, dtype=np.int32).reshape(-1) for s in new_ids_list]
        slots_h = np.asarray(slots, dtype=np.int32).reshape(-1)
        if len(seqs) != B or B < 1:
            raise ValueError(f"extend_verbalize: {B} slots, {len(seqs)} id lists")
        held = [len(cache.ids[s]) if 0 <= s < cache.num_slots else 0 for s in slots_h.tolist()]
        cl_h = np.asarray(held if cached_len is None else cached_len, dtype=np.int32).reshape(-1)
        keep_h = np.asarray([len(s) for s in seqs] if keep is None else keep, dtype=np.int32).reshape(-1)
        if len(cl_h) != B or len(keep_h) != B:
            raise ValueError("extend_verbalize: cached_len and keep take one value per slot")
        if any(int(c) > n for c, n in zip(cl_h, held)):
            raise ValueError(f"extend_verbalize: cached_len {cl_h.tolist()} exceeds what the slots hold {held}")
        ids_h = np.concatenate(seqs) if seqs else np.zeros(0, np.int32)
        cu_h = np.zeros(B + 1, np.int32)
        cu_h[1:] = np.cumsum([len(s) for s in seqs])
        dev = self.device
        lab = torch.as_tensor(np.asarray(label_token_ids, dtype=np.int32)).to(dev)
        # one upload: slots | cached_len | cu | ids
        meta = torch.from_numpy(np.concatenate([slots_h, cl_h, cu_h, ids_h]).astype(np.int32)).to(dev)
        slots_d, cl_d, cu_d, ids_d = meta[:B], meta[B:2 * B], meta[2 * B:3 * B + 1], meta[3 * B + 1:]
        out = torch.empty((B, lab.numel()), dtype=torch.float32, device=dev)
        n = max(int(cu_h[-1]), 1)
        need = lib().lr_llama_extend_workspace_bytes(self._h, n, B, cache.max_tokens)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(lib().lr_llama_extend_verbalize(
                self._h, cache.table.data_ptr(), cache.num_slots, cache.max_tokens, slots_d.data_ptr(), slots_h.ctypes.data,
                cl_d.data_ptr(), cl_h.ctypes.data, ids_d.data_ptr(), cu_d.data_ptr(), cu_h.ctypes.data, keep_h.ctypes.data, B,
                lab.data_ptr(), lab.numel(), out.data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream_ptr()),
                "lr_llama_extend_verbalize")
        for b, s in enumerate(slots_h.tolist()):
            cache.ids[s] = cache.ids[s][:int(cl_h[b])] + seqs[b][:int(keep_h[b])].tolist()
        return out

    def last_logits(self, seqs):
        ids, cu, cu_host = self._packed(seqs)
        B = len(cu_host) - 1
        self._check_lengths(cu_host)
        out = torch.empty((B, self.config["vocab_size"]), dtype=torch.float32, device=self.device)
        ws = self._workspace(int(cu_host[-1]), B)
        with torch.cuda.device(self.device):
            check(lib().lr_llama_last_logits(self._h, ids.data_ptr(), cu.data_ptr(), cu_host.ctypes.data, B,
                                             out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()),
                  "lr_llama_last_logits")
        return out

    def forward(self, input_ids=None, attention_mask=None, labels=None, **_unused):
        """Patched-forward compatible call (model/llm.py:35-143): last-position logits in fp32;
        in eval with labels the loss is the constant -1.0 (model/llm.py:128-129)."""
        logits = self.last_logits(unpad_left(input_ids, attention_mask))
        loss = torch.tensor(-1.0) if labels is not None else None
        return CausalLMOutput(loss=loss, logits=logits)

    __call__ = forward
