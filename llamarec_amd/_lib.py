"""Loader for libllamarec_mi355x.so (the C-ABI HIP library). There is NO fallback: if the
library is missing or a call fails, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# LLAMAREC_LIB selects another BUILD of the same library (same-box A/B runs of two commits: tools/gpu_ab_lib.sh) without
# overwriting the product file; it is never a fallback -- a missing file raises like the default one.
LIB_PATH = os.environ.get("LLAMAREC_LIB") or os.path.join(_HERE, "lib", "libllamarec_mi355x.so")
_lib = None


class LlamaRecError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol include/llamarec_mi355x.h declares
PROTOTYPES = {
    "lr_last_error": (C.c_char_p, []),
    "lr_version": (C.c_char_p, []),
    "lr_lru_packed_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lr_lru_pack": (C.c_int, [C.POINTER(A.LrLruWeightsDesc), C.c_void_p, C.c_size_t]),
    "lr_lru_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "lr_lru_destroy": (None, [C.c_void_p]),
    "lr_lru_set_encoder_pipeline": (C.c_int, [C.c_void_p, C.c_int32]),
    "lr_lru_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lr_lru_encode_last": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lru_retrieve_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lru_topk_path": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_int32), C.c_void_p]),
    "lr_lru_scores_last": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lru_user_state_row_bytes": (C.c_size_t, [C.c_int32]),
    "lr_lru_user_state_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "lr_lru_user_state_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_void_p, C.c_void_p]),
    "lr_lru_retrieve_topk_user_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lru_user_state_encode_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lr_lru_user_state_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lru_retrieve_topk_seed_user_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                       C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_size_t, C.c_void_p]),
    "lr_rank_histogram": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "lr_rank_classes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_profile_start": (C.c_int, [C.c_int32]),
    "lr_profile_stop": (C.c_int, []),
    "lr_profile_collect": (C.c_int, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int64)]),
    "lr_profile_records": (C.c_int64, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "lr_gemm_bf16_nt_epi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_gemm_bf16_nt_bias_epi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lr_gemm_bf16_nt_residual_rmsnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_int32,
                                                   C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_gemm_bf16_nt_residual_rmsnorm_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_int32,
                                                      C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_rope_table_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lr_rope_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "lr_rope_table_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.POINTER(A.LrRopeScaling), C.c_void_p]),
    "lr_metrics_from_histogram": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "lr_lru_train_state_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "lr_lru_train_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "lr_lru_train_destroy": (None, [C.c_void_p]),
    "lr_lru_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "lr_lru_train_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lru_train_apply": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "lr_lru_train_set_graph": (C.c_int, [C.c_void_p, C.c_int32]),
    "lr_lru_train_set_fused": (C.c_int, [C.c_void_p, C.c_int32]),
    "lr_lru_train_set_deterministic": (C.c_int, [C.c_void_p, C.c_int32]),
    "lr_lru_train_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_size_t)]),
    "lr_lru_train_param_range": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lr_lru_train_ce_parity_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "lr_lru_train_ce_parity": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_lru_train_ce_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "lr_llama_create": (C.c_int, [C.POINTER(A.LrLlamaConfig), C.POINTER(A.LrLlamaWeightsDesc),
                                  C.POINTER(C.c_void_p)]),
    "lr_llama_create_ex": (C.c_int, [C.POINTER(A.LrLlamaConfig), C.POINTER(A.LrLlamaArch), C.POINTER(A.LrLlamaWeightsDesc),
                                     C.POINTER(C.c_void_p)]),
    "lr_llama_destroy": (None, [C.c_void_p]),
    "lr_llama_set_variants": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "lr_llama_set_last_layer_pruning": (C.c_int, [C.c_void_p, C.c_int32]),
    "lr_llama_set_rope_scaling": (C.c_int, [C.c_void_p, C.POINTER(A.LrRopeScaling)]),
    "lr_llama_set_gemma2": (C.c_int, [C.c_void_p, C.POINTER(A.LrGemma2Ext)]),
    "lr_llama_set_gemma3": (C.c_int, [C.c_void_p, C.POINTER(A.LrGemma3Ext)]),
    "lr_llama_set_qkv_bias": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lr_llama_set_qk_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_qk_norm_rope_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_qk_norm_rope_ex_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "lr_qk_norm_bwd_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]),
    "lr_fold_norm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lr_llama_set_folded_norms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_llama_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "lr_llama_prefill_verbalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
    "lr_llama_prefill_verbalize_prefix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                    C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p]),
    "lr_common_prefix_len": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    # ranker sessions: a per-user K / V cache of the prompt prefix
    "lr_llama_kv_cache_slot_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lr_llama_extend_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lr_llama_extend_verbalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_attention_varlen_cached": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_llama_last_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_llama_pack_gate_up": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_llama_pack_qkv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p]),
    "lr_gemm_bf16_nt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p]),
    "lr_gemm_bf16_nt_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_gemm_splitk_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_size_t, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]),
    "lr_attention_varlen": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_attention_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "lr_attention_varlen_ws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_attention_varlen_prefix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_attention_last_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_attention_varlen_softcap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    "lr_attention_last_rows_softcap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                                 C.c_void_p]),
    "lr_attention_varlen_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_attention_last_rows_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_residual_postnorm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_float, C.c_void_p]),
    "lr_rmsnorm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p]),
    "lr_nf4_scratch_bytes": (C.c_size_t, [C.c_size_t]),
    "lr_nf4_roundtrip_bf16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "lr_nf4_dynamic_map": (C.c_int, [C.POINTER(C.c_float)]),
    "lr_transpose_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lr_llama_lora_state_bytes": (C.c_size_t, [C.c_void_p, C.POINTER(A.LrLoraTrainConfig)]),
    "lr_llama_lora_create": (C.c_int, [C.c_void_p, C.POINTER(A.LrLlamaWeightsTDesc), C.POINTER(A.LrLoraTrainConfig),
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lr_llama_lora_state_bytes_ex": (C.c_size_t, [C.c_void_p, C.POINTER(A.LrLoraTrainConfig), C.POINTER(A.LrLoraTargets)]),
    "lr_llama_lora_create_ex": (C.c_int, [C.c_void_p, C.POINTER(A.LrLlamaWeightsTDesc), C.POINTER(A.LrLoraTrainConfig),
                                          C.POINTER(A.LrLoraTargets), C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_void_p)]),
    "lr_llama_lora_destroy": (None, [C.c_void_p]),
    "lr_llama_lora_buffers": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "lr_llama_lora_param_range": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_size_t)]),
    "lr_llama_lora_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lr_llama_lora_set_deterministic": (C.c_int, [C.c_void_p, C.c_int32]),
    "lr_llama_lora_get_progress": (C.c_int, [C.c_void_p, C.POINTER(A.LrLoraProgress), C.c_void_p]),
    "lr_llama_lora_set_progress": (C.c_int, [C.c_void_p, C.POINTER(A.LrLoraProgress), C.c_void_p]),
    "lr_llama_lora_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "lr_llama_lora_apply": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "lr_llama_lora_eval_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "lr_llama_lora_prefill_verbalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_void_p]),
    # variant (the int32 before the scratch / stream): 1 generic, 2 = head_dim-128 MFMA, 6 = the head_dim-64 MFMA training
    # pair (forward writing lse, two-pass backward); 4 and 5 write no lse and have no backward
    "lr_attention_varlen_lse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_attention_bwd_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lr_attention_varlen_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_attention_varlen_bwd_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_void_p]),
    # the prefill's norm, head, embedding and metadata kernels alone (exposed for parity tests)
    "lr_llama_head_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_void_p]),
    "lr_llama_embed_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                      C.c_void_p]),
    "lr_llama_token_meta": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_gather_rows_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lr_rms_rstd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "lr_gemm_bf16_nt_rowscale_epi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    # the LoRA step's small kernels alone (exposed for parity tests)
    "lr_lora_skinny_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_int32, C.c_float, C.c_uint32, C.c_float, C.c_void_p]),
    "lr_lora_tn_det_floats": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lr_lora_tn_f32": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_float, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_float,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "lr_lora_expand_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_int32, C.c_float, C.c_uint32, C.c_float, C.c_void_p]),
    "lr_swiglu_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_swiglu_bwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lr_rmsnorm_bwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32, C.c_float,
                                      C.c_void_p]),
    "lr_lora_rope_fwd_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "lr_rope_bwd_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_swiglu_lora_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_int32, C.c_float, C.c_void_p]),
    "lr_lora_prep_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lr_lora_prep_module_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p]),
    "lr_ce_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int32,
                             C.c_void_p]),
    "lr_rowdot_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lr_lora_adamw_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_void_p]),
}


def lib():
    """The loaded library with prototypes set. Raises LlamaRecError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LlamaRecError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        # torch first: it bundles its own libamdhip64, and whichever HIP runtime a process loads FIRST is the one that owns
        # the devices -- with this library (linked against /opt/rocm's runtime) loaded before torch, its calls then fail with
        # "no ROCm-capable device is detected" (seen when build() and smoke() ran in one process). Loaded after torch the
        # library binds to the runtime torch already brought in, whatever the import order of the caller.
        import torch  # noqa: F401

        l = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(l, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().lr_last_error().decode("utf-8", "replace")
        raise LlamaRecError(f"{what} failed (rc={rc}): {msg}")


def stream_ptr(stream=None) -> int:
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)
