// api_llama.hip -- C ABI entry points for stage 2 (declared in include/llamarec_mi355x.h):
// one Llama prefill over packed prompts + verbalizer gather at each prompt's last token.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "llama_kernels.h"

typedef unsigned short u16;

extern "C" int lr_llama_create_ex(const LrLlamaConfig* cfg, const LrLlamaArch* arch, const LrLlamaWeightsDesc* w,
                                  lr_llama_t** out) {
  if (!cfg || !w || !out || !w->layers) LR_FAIL(LR_EINVAL, "lr_llama_create: null argument");
  const LrLlamaArch llama_arch = {0, 0, 1.0f, {0, 0, 0, 0, 0}};
  if (!arch) arch = &llama_arch;
  if (arch->norm_style < 0 || arch->norm_style > 1 || arch->mlp_act < 0 || arch->mlp_act > 1 ||
      !(arch->embed_scale > 0.f) || arch->embed_scale != arch->embed_scale)
    LR_FAIL(LR_EINVAL, "lr_llama_create_ex: arch norm_style=%d mlp_act=%d embed_scale=%g", arch->norm_style, arch->mlp_act,
            (double)arch->embed_scale);
  for (int i = 0; i < 5; ++i)
    if (arch->reserved[i]) LR_FAIL(LR_EINVAL, "lr_llama_create_ex: arch reserved word %d is not zero", i);
  if (cfg->num_layers < 1 || cfg->num_heads < 1 || cfg->num_kv_heads < 1 || cfg->vocab_size < 1)
    LR_FAIL(LR_EINVAL, "lr_llama_create: bad config");
  if (cfg->hidden_size % 8 != 0 || cfg->intermediate_size % 16 != 0)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_create: hidden_size %% 8 and intermediate_size %% 16 must be 0");
  if (cfg->num_heads % cfg->num_kv_heads != 0 || cfg->head_dim < 4 || cfg->head_dim % 4 != 0 ||
      cfg->head_dim > 256)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_create: heads=%d kv_heads=%d head_dim=%d", cfg->num_heads,
            cfg->num_kv_heads, cfg->head_dim);
  if (cfg->max_positions < 1) LR_FAIL(LR_EINVAL, "lr_llama_create: max_positions");
  if (!w->embed || !w->final_norm || !w->lm_head) LR_FAIL(LR_EINVAL, "lr_llama_create: null weight");
  for (int i = 0; i < cfg->num_layers; ++i) {
    const LrLlamaLayerWeights& l = w->layers[i];
    if (!l.input_norm || !l.wqkv || !l.wo || !l.post_norm || !l.wgu || !l.wdown)
      LR_FAIL(LR_EINVAL, "lr_llama_create: layer %d has a null weight", i);
  }
  lr_llama* h = (lr_llama*)calloc(1, sizeof(lr_llama));
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_create: out of host memory");
  h->cfg = *cfg;
  h->arch = *arch;
  h->embed = w->embed;
  h->final_norm = w->final_norm;
  h->lm_head = w->lm_head;
  h->prune_last = 1;
  h->layers = (LrLlamaLayerWeights*)malloc(sizeof(LrLlamaLayerWeights) * cfg->num_layers);
  memcpy(h->layers, w->layers, sizeof(LrLlamaLayerWeights) * cfg->num_layers);
  LR_CHECK_HIP(hipGetDevice(&h->device));
  *out = h;
  return LR_OK;
}

extern "C" int lr_llama_create(const LrLlamaConfig* cfg, const LrLlamaWeightsDesc* w, lr_llama_t** out) {
  return lr_llama_create_ex(cfg, nullptr, w, out);
}

extern "C" int lr_llama_set_variants(lr_llama_t* h, int32_t gemm_variant, int32_t attention_variant) {
  if (!h || (gemm_variant != 0 && gemm_variant != 1 && gemm_variant != 4 && gemm_variant != 5 && gemm_variant != 6 && gemm_variant != 7) ||
      attention_variant < 0 || attention_variant > 9)
    LR_FAIL(LR_EINVAL, "lr_llama_set_variants: gemm in {0, 1, 4, 5, 6, 7}, attention in {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}");
  h->gemm_variant = gemm_variant;
  h->attn_variant = attention_variant;
  return LR_OK;
}

extern "C" int lr_llama_set_rope_scaling(lr_llama_t* h, const LrRopeScaling* s) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_set_rope_scaling: null handle");
  LR_RUN(lr_check_rope_scaling(s, "lr_llama_set_rope_scaling"));
  if (s) h->rope_scaling = *s;
  else memset(&h->rope_scaling, 0, sizeof(h->rope_scaling));
  return LR_OK;
}

static bool finite_nonneg(float v) { return v >= 0.f && v < __builtin_inff(); }   // false for NaN too

extern "C" int lr_llama_set_gemma2(lr_llama_t* h, const LrGemma2Ext* e) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_set_gemma2: null handle");
  const int L = h->cfg.num_layers;
  const uint16_t **an = nullptr, **mn = nullptr;
  float scale = 0.f;
  if (e) {   // every check before the handle changes
    if (!finite_nonneg(e->attn_softcap) || !finite_nonneg(e->final_softcap) || !finite_nonneg(e->attn_scale))
      LR_FAIL(LR_EINVAL, "lr_llama_set_gemma2: attn_softcap=%g final_softcap=%g attn_scale=%g (finite and >= 0)",
              (double)e->attn_softcap, (double)e->final_softcap, (double)e->attn_scale);
    for (int i = 0; i < 5; ++i)
      if (e->reserved[i]) LR_FAIL(LR_EINVAL, "lr_llama_set_gemma2: reserved word %d is not zero", i);
    if ((e->attn_out_norm == nullptr) != (e->mlp_out_norm == nullptr))
      LR_FAIL(LR_EINVAL, "lr_llama_set_gemma2: give both out-norm arrays or neither");
    if (e->attn_out_norm)
      for (int l = 0; l < L; ++l)
        if (!e->attn_out_norm[l] || !e->mlp_out_norm[l]) LR_FAIL(LR_EINVAL, "lr_llama_set_gemma2: layer %d has a null out-norm", l);
    // any extension: a Gemma handle. (Such a handle has no LoRA engine -- lr_llama_lora_create refuses it -- so no engine
    // can be left running uncapped training attention beside a capped prefill.)
    if (h->arch.norm_style != 1)
      LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_gemma2: caps and out-norms need a handle with the Gemma norm (norm_style %d)",
              h->arch.norm_style);
    const float own = 1.0f / sqrtf((float)h->cfg.head_dim);
    scale = e->attn_scale > 0.f ? e->attn_scale : own;
    if (!(e->attn_softcap > 0.f) && scale != own)
      LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_gemma2: attn_scale %g without a soft cap (the uncapped kernels scale by "
              "head_dim^-0.5 = %g)", (double)scale, (double)own);
    if (h->wqkv_folded) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_gemma2: the handle has folded norms");
    if (h->gemma3) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_gemma2: the handle has a Gemma-3 extension (lr_llama_set_gemma3)");
    if (h->q_norm) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_gemma2: the handle has q/k norms (lr_llama_set_qk_norm)");
    if (e->attn_out_norm) {
      an = (const uint16_t**)malloc(sizeof(void*) * L);
      mn = (const uint16_t**)malloc(sizeof(void*) * L);
      if (!an || !mn) {
        free(an);
        free(mn);
        LR_FAIL(LR_EINVAL, "lr_llama_set_gemma2: out of host memory");
      }
      memcpy(an, e->attn_out_norm, sizeof(void*) * L);
      memcpy(mn, e->mlp_out_norm, sizeof(void*) * L);
    }
  }
  if (!e && h->gemma3) return LR_OK;   // nothing of Gemma-2 is set: the out-norms are the Gemma-3 extension's
  free(h->attn_out_norm);
  free(h->mlp_out_norm);
  h->attn_out_norm = an;
  h->mlp_out_norm = mn;
  h->gemma2 = e ? 1 : 0;
  h->attn_softcap = e ? e->attn_softcap : 0.f;
  h->final_softcap = e ? e->final_softcap : 0.f;
  h->attn_scale = (e && e->attn_softcap > 0.f) ? scale : 0.f;
  return LR_OK;
}

extern "C" int lr_llama_set_qkv_bias(lr_llama_t* h, const uint16_t* const* bqkv) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_set_qkv_bias: null handle");
  const int L = h->cfg.num_layers;
  const uint16_t** own = nullptr;
  if (bqkv) {   // every check before the handle changes
    for (int l = 0; l < L; ++l)
      if (!bqkv[l]) LR_FAIL(LR_EINVAL, "lr_llama_set_qkv_bias: layer %d has a null bias", l);
    for (int l = 0; l < L; ++l)   // the K | V slice starts nh head_dim elements in: both ends 8-byte aligned
      if ((reinterpret_cast<uintptr_t>(bqkv[l]) & 7) || (h->cfg.num_heads * h->cfg.head_dim) % 4 != 0)
        LR_FAIL(LR_EINVAL, "lr_llama_set_qkv_bias: layer %d's bias is not 8-byte aligned", l);
    if (h->wqkv_folded) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qkv_bias: the handle has folded norms");
    if (h->gemma3) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qkv_bias: the handle has a Gemma-3 extension (lr_llama_set_gemma3)");
    if (h->q_norm) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qkv_bias: the handle has q/k norms (lr_llama_set_qk_norm)");
    own = (const uint16_t**)malloc(sizeof(void*) * L);
    if (!own) LR_FAIL(LR_EINVAL, "lr_llama_set_qkv_bias: out of host memory");
    memcpy(own, bqkv, sizeof(void*) * L);
  }
  free(h->bqkv);
  h->bqkv = own;
  return LR_OK;
}

extern "C" int lr_llama_set_qk_norm(lr_llama_t* h, const uint16_t* const* q_norm, const uint16_t* const* k_norm) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_set_qk_norm: null handle");
  const int L = h->cfg.num_layers;
  const uint16_t **qn = nullptr, **kn = nullptr;
  if ((q_norm == nullptr) != (k_norm == nullptr)) LR_FAIL(LR_EINVAL, "lr_llama_set_qk_norm: give both arrays or neither");
  // (NULL, NULL too: the norms of such a handle are the extension's, and lr_llama_set_gemma3(h, NULL) takes them off)
  if (h->gemma3) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qk_norm: the handle has a Gemma-3 extension (lr_llama_set_gemma3)");
  if (q_norm) {   // every check before the handle changes
    for (int l = 0; l < L; ++l)
      if (!q_norm[l] || !k_norm[l]) LR_FAIL(LR_EINVAL, "lr_llama_set_qk_norm: layer %d has a null norm weight", l);
    for (int l = 0; l < L; ++l)   // the sweeps load the weights 16 bytes at a time
      if ((reinterpret_cast<uintptr_t>(q_norm[l]) | reinterpret_cast<uintptr_t>(k_norm[l])) & 15)
        LR_FAIL(LR_EINVAL, "lr_llama_set_qk_norm: layer %d's norm weights are not 16-byte aligned", l);
    if (h->wqkv_folded) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qk_norm: the handle has folded norms");
    if (h->gemma2) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qk_norm: the handle has a Gemma-2 extension (lr_llama_set_gemma2)");
    if (h->bqkv) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qk_norm: the handle has q/k/v biases (lr_llama_set_qkv_bias)");
    if (!lr_qk_norm_head_dim_ok(h->cfg.head_dim))
      LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_qk_norm: head_dim %d (a power of two from 16 to 256)", h->cfg.head_dim);
    qn = (const uint16_t**)malloc(sizeof(void*) * L);
    kn = (const uint16_t**)malloc(sizeof(void*) * L);
    if (!qn || !kn) {
      free(qn);
      free(kn);
      LR_FAIL(LR_EINVAL, "lr_llama_set_qk_norm: out of host memory");
    }
    memcpy(qn, q_norm, sizeof(void*) * L);
    memcpy(kn, k_norm, sizeof(void*) * L);
  }
  free(h->q_norm);
  free(h->k_norm);
  h->q_norm = qn;
  h->k_norm = kn;
  return LR_OK;
}

// Gemma-3: see include/llamarec_mi355x.h. The extension fills the handle's out-norm and q/k-norm arrays (run_body reads them as it
// does for Gemma-2 and Qwen3) and adds what is Gemma-3's own: the window, the layer kinds and the second rotary table.
extern "C" int lr_llama_set_gemma3(lr_llama_t* h, const LrGemma3Ext* e) {
  const char* who = "lr_llama_set_gemma3";
  if (!h) LR_FAIL(LR_EINVAL, "%s: null handle", who);
  const int L = h->cfg.num_layers;
  if (!e) {
    if (!h->gemma3) return LR_OK;
    free(h->attn_out_norm);
    free(h->mlp_out_norm);
    free(h->q_norm);
    free(h->k_norm);
    free(h->layer_sliding);
    h->attn_out_norm = h->mlp_out_norm = h->q_norm = h->k_norm = nullptr;
    h->layer_sliding = nullptr;
    h->gemma3 = h->window = 0;
    h->rope_theta_local = h->global_linear_factor = 0.f;
    return LR_OK;
  }
  // every check before the handle changes
  if (e->sliding_window < 1) LR_FAIL(LR_EINVAL, "%s: sliding_window %d (>= 1)", who, e->sliding_window);
  if (!(e->rope_theta_local > 0.f) || !(e->rope_theta_local < __builtin_inff()) || !finite_nonneg(e->global_linear_factor) ||
      !finite_nonneg(e->attn_scale))
    LR_FAIL(LR_EINVAL, "%s: rope_theta_local=%g (finite and > 0) global_linear_factor=%g attn_scale=%g (finite and >= 0)", who,
            (double)e->rope_theta_local, (double)e->global_linear_factor, (double)e->attn_scale);
  for (int i = 0; i < 4; ++i)
    if (e->reserved[i]) LR_FAIL(LR_EINVAL, "%s: reserved word %d is not zero", who, i);
  if (!e->layer_is_sliding || !e->q_norm || !e->k_norm || !e->attn_out_norm || !e->mlp_out_norm)
    LR_FAIL(LR_EINVAL, "%s: a null array (layer kinds, q_norm, k_norm, attn_out_norm, mlp_out_norm)", who);
  for (int l = 0; l < L; ++l) {
    if (e->layer_is_sliding[l] > 1) LR_FAIL(LR_EINVAL, "%s: layer %d's kind is %d (0 global, 1 sliding)", who, l, e->layer_is_sliding[l]);
    if (!e->q_norm[l] || !e->k_norm[l] || !e->attn_out_norm[l] || !e->mlp_out_norm[l])
      LR_FAIL(LR_EINVAL, "%s: layer %d has a null norm weight", who, l);
    // the sweep and the sandwich-norm kernel load their weights 16 bytes at a time
    if ((reinterpret_cast<uintptr_t>(e->q_norm[l]) | reinterpret_cast<uintptr_t>(e->k_norm[l]) |
         reinterpret_cast<uintptr_t>(e->attn_out_norm[l]) | reinterpret_cast<uintptr_t>(e->mlp_out_norm[l])) & 15)
      LR_FAIL(LR_EINVAL, "%s: layer %d's norm weights are not 16-byte aligned", who, l);
  }
  if (h->arch.norm_style != 1)
    LR_FAIL(LR_EUNSUPPORTED, "%s: needs a handle with the Gemma norm (norm_style %d)", who, h->arch.norm_style);
  if (h->wqkv_folded) LR_FAIL(LR_EUNSUPPORTED, "%s: the handle has folded norms", who);
  if (h->gemma2) LR_FAIL(LR_EUNSUPPORTED, "%s: the handle has a Gemma-2 extension (lr_llama_set_gemma2)", who);
  if (h->bqkv) LR_FAIL(LR_EUNSUPPORTED, "%s: the handle has q/k/v biases (lr_llama_set_qkv_bias)", who);
  if (h->q_norm && !h->gemma3) LR_FAIL(LR_EUNSUPPORTED, "%s: the handle has Qwen3 q/k norms (lr_llama_set_qk_norm)", who);
  if (!lr_qk_norm_head_dim_ok(h->cfg.head_dim))
    LR_FAIL(LR_EUNSUPPORTED, "%s: head_dim %d (the q/k norm sweep takes a power of two from 16 to 256)", who, h->cfg.head_dim);
  const float own = 1.0f / sqrtf((float)h->cfg.head_dim);
  if (e->attn_scale > 0.f && e->attn_scale != own)
    LR_FAIL(LR_EUNSUPPORTED, "%s: attn_scale %g (the uncapped kernels scale by head_dim^-0.5 = %g)", who, (double)e->attn_scale,
            (double)own);
  const uint16_t** arr[4] = {nullptr, nullptr, nullptr, nullptr};
  const uint16_t* const* src[4] = {e->attn_out_norm, e->mlp_out_norm, e->q_norm, e->k_norm};
  uint8_t* kinds = (uint8_t*)malloc((size_t)L);
  bool ok = kinds != nullptr;
  for (int i = 0; i < 4; ++i) {
    arr[i] = (const uint16_t**)malloc(sizeof(void*) * L);
    ok = ok && arr[i];
  }
  if (!ok) {
    free(kinds);
    for (int i = 0; i < 4; ++i) free(arr[i]);
    LR_FAIL(LR_EINVAL, "%s: out of host memory", who);
  }
  for (int i = 0; i < 4; ++i) memcpy(arr[i], src[i], sizeof(void*) * L);
  memcpy(kinds, e->layer_is_sliding, (size_t)L);
  free(h->attn_out_norm);
  free(h->mlp_out_norm);
  free(h->q_norm);
  free(h->k_norm);
  free(h->layer_sliding);
  h->attn_out_norm = arr[0];
  h->mlp_out_norm = arr[1];
  h->q_norm = arr[2];
  h->k_norm = arr[3];
  h->layer_sliding = kinds;
  h->gemma3 = 1;
  h->window = e->sliding_window;
  h->rope_theta_local = e->rope_theta_local;
  h->global_linear_factor = (e->global_linear_factor > 0.f && e->global_linear_factor != 1.0f) ? e->global_linear_factor : 0.f;
  return LR_OK;
}

extern "C" int lr_llama_set_last_layer_pruning(lr_llama_t* h, int32_t enable) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_set_last_layer_pruning: null handle");
  h->prune_last = enable ? 1 : 0;
  return LR_OK;
}

extern "C" void lr_llama_destroy(lr_llama_t* h) {
  if (!h) return;
  free(h->layers);
  free(h->wqkv_folded);
  free(h->wgu_folded);
  free(h->attn_out_norm);
  free(h->mlp_out_norm);
  free(h->bqkv);
  free(h->q_norm);
  free(h->k_norm);
  free(h->layer_sliding);
  free(h);
}

extern "C" int lr_fold_norm_bf16(const uint16_t* w, const uint16_t* norm_w, int32_t rows, int32_t cols, uint16_t* out,
                                 void* hip_stream) {
  if (!w || !norm_w || !out || rows < 1 || cols < 8) LR_FAIL(LR_EINVAL, "lr_fold_norm_bf16: bad argument");
  return lr_launch_fold_norm(w, norm_w, out, (size_t)rows, cols, (hipStream_t)hip_stream);
}

extern "C" int lr_llama_set_folded_norms(lr_llama_t* h, const uint16_t* const* wqkv_folded,
                                         const uint16_t* const* wgu_folded) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_set_folded_norms: null handle");
  if ((h->arch.norm_style != 0 || h->arch.mlp_act != 0) && (wqkv_folded || wgu_folded))
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_folded_norms: Llama arch only (a Gemma norm (1 + w) cannot be folded into bf16 "
            "weights at HF's rounding, and the GeGLU epilogue takes no row scale)");
  if (h->gemma2 && (wqkv_folded || wgu_folded))
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_folded_norms: not with a Gemma-2 extension (lr_llama_set_gemma2)");
  if (h->bqkv && (wqkv_folded || wgu_folded))
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_folded_norms: not with q/k/v biases (lr_llama_set_qkv_bias)");
  if (h->gemma3 && (wqkv_folded || wgu_folded))
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_folded_norms: not with a Gemma-3 extension (lr_llama_set_gemma3)");
  if (h->q_norm && (wqkv_folded || wgu_folded))
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_set_folded_norms: not with q/k norms (lr_llama_set_qk_norm)");
  free(h->wqkv_folded);
  free(h->wgu_folded);
  h->wqkv_folded = h->wgu_folded = nullptr;
  if (!wqkv_folded && !wgu_folded) return LR_OK;  // back to the separate RMSNorm pass
  if (!wqkv_folded || !wgu_folded) LR_FAIL(LR_EINVAL, "lr_llama_set_folded_norms: give both arrays or neither");
  const int L = h->cfg.num_layers;
  for (int l = 0; l < L; ++l)
    if (!wqkv_folded[l] || !wgu_folded[l]) LR_FAIL(LR_EINVAL, "lr_llama_set_folded_norms: layer %d has a null matrix", l);
  h->wqkv_folded = (const uint16_t**)malloc(sizeof(void*) * L);
  h->wgu_folded = (const uint16_t**)malloc(sizeof(void*) * L);
  memcpy(h->wqkv_folded, wqkv_folded, sizeof(void*) * L);
  memcpy(h->wgu_folded, wgu_folded, sizeof(void*) * L);
  return LR_OK;
}

struct LlamaWs {
  int32_t *tok_pos, *tok_src, *last_rows, *last_pos, *seg_start;
  float *rope, *rstd;
  float* rope_local;                          // Gemma-3: the sliding layers' fp32 table (null without the extension)
  u16 *x, *xn, *qkv, *att, *hmid;
  u16 *x_last, *xn_last, *att_last, *h_last, *q_last;  // compact [B][.] buffers of the pruned last layer
  LrGemmSplitK splitk;                        // fp32 partial planes of the split-K GEMMs (gemm variants 5, 7)
  unsigned* rope16;                           // the rope table as packed bf16 (cos | sin << 16) pairs
  long long* row_off;                         // extend call only: every new row's cache-row offset in a layer (kv_cache_meta_kernel)
  int32_t* prefix_bad;                        // device word: a prompt broke the shared-prefix promise (token_meta_kernel)
  void* attn_items;                           // work-item list of the 256-row attention kernel (llama_attn256.hip)
  size_t attn_items_bytes;
  bool compact;                               // ws.x_last (not ws.x) holds the final residual rows
  size_t total;
};

static LlamaWs carve(const LrLlamaConfig& c, int max_tokens, int max_seqs, char* base, bool two_rope_tables) {
  LlamaWs w;
  w.compact = false;
  w.row_off = nullptr;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += lr_align_up(bytes, 256);
    return base + at;
  };
  const size_t n = (size_t)max_tokens;
  const size_t qkv_w = (size_t)(c.num_heads + 2 * c.num_kv_heads) * c.head_dim;
  w.tok_pos = (int32_t*)take(n * 4);
  w.tok_src = (int32_t*)take(n * 4);
  // the table is built for the batch's longest prompt, which has at most max_tokens rows (max_positions is 131 072 in a
  // Llama-3.1 / 3.2 config)
  const size_t rope_rows = (size_t)(c.max_positions < max_tokens ? c.max_positions : max_tokens);
  w.rope = (float*)take(rope_rows * (c.head_dim / 2) * 2 * sizeof(float));
  w.rope16 = (unsigned*)take(rope_rows * (c.head_dim / 2) * sizeof(unsigned));
  // (the q/k sweep, the only reader of a Gemma-3 handle's tables, reads the fp32 form)
  w.rope_local = two_rope_tables ? (float*)take(rope_rows * (c.head_dim / 2) * 2 * sizeof(float)) : nullptr;
  w.rstd = (float*)take(n * sizeof(float));
  w.x = (u16*)take(n * c.hidden_size * 2);
  w.xn = (u16*)take(n * c.hidden_size * 2);
  w.qkv = (u16*)take(n * qkv_w * 2);
  w.att = (u16*)take(n * (size_t)c.num_heads * c.head_dim * 2);
  w.hmid = (u16*)take(n * c.intermediate_size * 2);
  const size_t nb = (size_t)(max_seqs > 0 ? max_seqs : 1);
  w.last_rows = (int32_t*)take(nb * 4);
  w.last_pos = (int32_t*)take(nb * 4);
  w.seg_start = (int32_t*)take((nb + 2) * 4);
  w.x_last = (u16*)take(nb * c.hidden_size * 2);
  w.xn_last = (u16*)take(nb * c.hidden_size * 2);
  w.att_last = (u16*)take(nb * (size_t)c.num_heads * c.head_dim * 2);
  w.h_last = (u16*)take(nb * c.intermediate_size * 2);
  w.q_last = (u16*)take(nb * (size_t)c.num_heads * c.head_dim * 2);
  w.splitk = {.ws = (float*)take(LR_SPLITK_WS_BYTES), .bytes = LR_SPLITK_WS_BYTES};
  w.prefix_bad = (int32_t*)take(sizeof(int32_t));
  w.attn_items_bytes = lr_attn256_ws_bytes(max_tokens, (int)nb + 1, c.num_heads);
  w.attn_items = take(w.attn_items_bytes);
  w.total = o;
  return w;
}

extern "C" size_t lr_llama_workspace_bytes(const lr_llama_t* h, int32_t max_tokens, int32_t max_seqs) {
  if (!h || max_tokens < 1) return 0;
  if (max_seqs < 1) max_seqs = 1;
  if (max_seqs > max_tokens) max_seqs = max_tokens;
  return carve(h->cfg, max_tokens, max_seqs, nullptr, h->gemma3 != 0).total;
}

// What run_body derives from a prompt batch before any launch: the internal layout, the carved workspace and seg_host, the
// host copy of the segment starts (launch geometry of the attention kernels).
// prefix_len = P > 0: the first P tokens of every prompt are the same (the caller's promise) and are run ONCE as segment 0
// of the internal layout (llama_elem.hip, token_meta_kernel); the other segments attend to its K/V rows. Every row then sees
// exactly the operands of the unshared run, so the scores are bit-identical to prefix_len = 0.
struct PrefillPlan {
  int P, n, S, maxT;              // shared prefix in effect, internal rows, segments, longest prompt
  bool windowed;                  // Gemma-3 with a prompt longer than the window: the sliding layers run windowed kernels
  std::vector<int32_t> seg_host;  // [S + 1]
  LlamaWs ws;
};
static int plan_batch(const lr_llama_t* h, const int32_t* cu_host, int B, int P, void* workspace, size_t workspace_bytes,
                      PrefillPlan* out) {
  const LrLlamaConfig& c = h->cfg;
  int minT = 0;
  LR_RUN(lr_check_segments(cu_host, B, "llama prefill", &minT, &out->maxT));
  if (out->maxT > c.max_positions)
    LR_FAIL(LR_EINVAL, "llama prefill: prompt of %d tokens exceeds max_positions %d", out->maxT, c.max_positions);
  if (P < 0 || (P > 0 && P >= minT))
    LR_FAIL(LR_EINVAL, "llama prefill: shared prefix of %d tokens, shortest prompt has %d (every prompt keeps >= 1 own token)",
            P, minT);
  if (B == 1 || !lr_attention_reads_prefix(h->attn_variant, c.head_dim, h->attn_softcap)) P = 0;
  // Gemma-3: a prompt longer than the window makes the sliding layers windowed, and the windowed kernels read no shared prefix:
  // the call runs every prompt whole (same scores). Within the window the window is the causal mask and nothing changes.
  out->windowed = h->gemma3 && out->maxT > h->window;
  if (out->windowed) P = 0;
  const int n_in = cu_host[B];
  out->ws = carve(c, n_in, B, (char*)workspace, h->gemma3 != 0);
  if (out->ws.total > workspace_bytes)
    LR_FAIL(LR_EWORKSPACE, "llama prefill: workspace needs %zu bytes for %d tokens, have %zu", out->ws.total, n_in,
            workspace_bytes);
  out->P = P;
  out->n = P > 0 ? n_in - (B - 1) * P : n_in;
  out->S = P > 0 ? B + 1 : B;
  out->seg_host.assign((size_t)out->S + 1, 0);   // P > 0: segment 0 = the prefix, then each prompt's own rows
  for (int b = 0; b <= B; ++b) out->seg_host[b + (P > 0)] = P + cu_host[b] - b * P;
  return LR_OK;
}

// B-row products (the pruned last layer): split-K over the 256-column tiles (weight streaming spread over 64-128 CUs
// instead of N / 64 workgroups of the small-tile kernel: 23 rows x 4096 x 4096 took 134 us there). With B <= 256 rows there
// is one row tile, so the split count depends on the weight's shape only and a prompt's arithmetic stays the same whatever
// else is in the batch; more prompts than that take the small-tile kernel as before. (Shapes the 256-tile kernel does not
// take fall back to it inside lr_launch_gemm.)
// The latency modes (gemm variants 5 and 7) split whatever B is; a variant-7 handle passes 7, which at B <= 256 is 5's split
// and past that keeps a prompt's arithmetic independent of the batch.
static int b_row_gemm_variant(const lr_llama_t* h, int B) {
  if (h->gemm_variant == 7) return 7;
  return (h->gemm_variant == 5 || ((h->gemm_variant == 0 || h->gemm_variant == 6) && B <= 256)) ? 5 : 1;   // 6 routes as auto
}

// Runs the transformer body; leaves the residual stream (before the final norm) in ws.x (all internal rows) or,
// after a pruned last layer, in ws.x_last (one row per prompt).
static int run_body(lr_llama_t* h, const int32_t* ids, const int32_t* cu, const int32_t* cu_host, int B, int prefix_len,
                    void* workspace, size_t workspace_bytes, hipStream_t st, LlamaWs* out_ws) {
  if (!h || !ids || !cu || !cu_host || !workspace) LR_FAIL(LR_EINVAL, "llama prefill: null argument");
  PrefillPlan plan;
  LR_RUN(plan_batch(h, cu_host, B, prefix_len, workspace, workspace_bytes, &plan));
  const LrLlamaConfig& c = h->cfg;
  const int P = plan.P, n = plan.n, S = plan.S;
  LlamaWs& ws = plan.ws;
  const int d = c.hidden_size, f = c.intermediate_size, nh = c.num_heads, nkv = c.num_kv_heads, hd = c.head_dim;
  const int ns = h->arch.norm_style;                               // 0 Llama, 1 Gemma RMSNorm
  const int epi_mlp = h->arch.mlp_act == 1 ? LR_EPI_GEGLU : LR_EPI_SWIGLU;
  const int gv = h->gemm_variant, pv = b_row_gemm_variant(h, B);
  LrAttnKernel attn_kernel;
  // Gemma-2 (lr_llama_set_gemma2): soft-capped scores, and o_proj / down_proj results normalised before they join the residual
  const float a_scale = h->attn_scale, a_cap = h->attn_softcap;
  const bool sandwich = h->attn_out_norm != nullptr;
  LR_RUN(lr_resolve_attention({.variant = h->attn_variant, .hd = hd, .prefix_len = P, .have_items_ws = true, .prefill = true,
                               .cap = a_cap}, &attn_kernel));
  // the MFMA kernels over ALL rows (188 us for 14.8 k tokens, 16 us for one prompt) beat the scalar kernel over the B last
  // rows (459 / 295 us), so a pruned last layer attends everything and keeps the last rows
  const bool attn_mfma = (hd == 128 && attn_kernel != LR_ATTN_GENERIC) || attn_kernel == LR_ATTN_HD256 ||
                         attn_kernel == LR_ATTN_HD64 || attn_kernel == LR_ATTN_HD96;
  const LrAttnArgs attn = {.qkv = ws.qkv, .out = ws.att, .cu = ws.seg_start, .cu_host = plan.seg_host.data(), .S = S,
                           .n_tok = n, .nh = nh, .nkv = nkv, .hd = hd, .prefix_len = P, .items_ws = ws.attn_items,
                           .scale = a_scale, .cap = a_cap};
  struct LayerRows { u16 *att, *x, *xn, *hmid; int M, gemm_variant; };   // what o_proj and the MLP run on
  const LayerRows full = {ws.att, ws.x, ws.xn, ws.hmid, n, gv}, last = {ws.att_last, ws.x_last, ws.xn_last, ws.h_last, B, pv};
  auto rope = [&](const int32_t* tok_pos, int rot_cols) {
    return LrGemmRope{.tok_pos = tok_pos, .cs = ws.rope, .cs16 = ws.rope16, .head_dim = hd, .rot_cols = rot_cols};
  };
  LR_RUN(lr_launch_token_meta(cu, B, P, ws.seg_start, ws.tok_pos, ws.tok_src, ws.last_rows, st, ws.last_pos, ids,
                              ws.prefix_bad));
  if (h->gemma3) {   // global layers: rope_theta with the linear factor; sliding layers: rope_theta_local, unscaled
    const LrRopeScaling lin = {2, h->global_linear_factor, 0.f, 0.f, 0, {0, 0, 0}};
    LR_RUN(lr_launch_rope_table(ws.rope, plan.maxT, hd, c.rope_theta, st, ws.rope16, h->global_linear_factor > 0.f ? &lin : nullptr));
    LR_RUN(lr_launch_rope_table(ws.rope_local, plan.maxT, hd, h->rope_theta_local, st));
  } else {
    LR_RUN(lr_launch_rope_table(ws.rope, plan.maxT, hd, c.rope_theta, st, ws.rope16, &h->rope_scaling));
  }
  if (attn_kernel == LR_ATTN_ROWS256)
    LR_RUN(lr_launch_attn256_items(ws.seg_start, S, n, nh, P, ws.attn_items, ws.attn_items_bytes, st));
  LR_RUN(lr_launch_embed(ids, ws.tok_src, h->embed, c.vocab_size, d, ws.x, n, st, h->arch.embed_scale));
  bool input_normed = false;   // ws.xn already holds RMSNorm(ws.x) with this layer's input_norm
#ifdef LR_EXPERIMENTS   // timing-only arm (never in the product library): the row statistics of layer 0 serve every layer
  static const bool exp_rstd_once = getenv("LR_EXP_RSTD_ONCE") && getenv("LR_EXP_RSTD_ONCE")[0] == '1';
#define EXP_SKIP_SWEEP (exp_rstd_once && l > 0)
#else
#define EXP_SKIP_SWEEP false
#endif
  for (int l = 0; l < c.num_layers; ++l) {
    const LrLlamaLayerWeights& w = h->layers[l];
    // RMSNorm: either its own pass (read + write every row), or -- folded -- only the row statistic, with the norm
    // weight already inside the projection matrix and rstd applied to the accumulator rows in the GEMM epilogue
    const bool folded = h->wqkv_folded != nullptr;
    const bool last_pruned = l == c.num_layers - 1 && h->prune_last;
    // Pruned last layer, on a kernel with a last-row mode (head_dim 64, 96, 128, 256): only each prompt's last token is consumed after it (model/llm.py:131), so Q is
    // needed for B rows only -- K and V for all of them. The projection runs on the K | V rows of wqkv (2/3 of the
    // product) for every row and on its Q rows for the B last rows; the attention kernel then evaluates ONE query row
    // per (prompt, head) over the prompt's keys instead of every tile.
    // Gemma-3: a sliding layer reads the local rotary table and, when the call has a prompt longer than the window
    // (plan.windowed), attends through the window: HD256's windowed kernels where HD256 was resolved, the generic kernel with
    // the window everywhere else (no other MFMA kernel has a windowed form)
    const bool sliding = h->gemma3 && h->layer_sliding[l];
    const float* const rope_l = sliding ? ws.rope_local : ws.rope;
    const int qk_ns = h->gemma3 ? 1 : 0;   // the sweep's norm: Gemma's (1 + w) in fp32, or Qwen3's
    const int win = (plan.windowed && sliding) ? h->window : 0;
    const LrAttnKernel kernel_l = (win && attn_kernel != LR_ATTN_HD256) ? LR_ATTN_GENERIC : attn_kernel;
    const bool mfma_l = win ? kernel_l == LR_ATTN_HD256 : attn_mfma;
    LrAttnArgs attn_l = attn;
    attn_l.window = win;
    const bool last_q_only = last_pruned && !folded && lr_attention_has_last_row_mode(kernel_l, hd) && gv != 1;
    if (folded && !EXP_SKIP_SWEEP) LR_RUN(lr_launch_rms_rstd(ws.x, ws.rstd, n, d, c.rms_eps, st));
    if (!folded && !input_normed) LR_RUN(lr_launch_rmsnorm(ws.x, w.input_norm, ws.xn, n, d, c.rms_eps, nullptr, st, ns));
    const int q_w = nh * hd, kv_w = 2 * nkv * hd;
    const u16* const bias = h->bqkv ? h->bqkv[l] : nullptr;   // Qwen2: [q_w + kv_w] in wqkv's row order (never folded)
    // Qwen3 (lr_llama_set_qk_norm; never folded, never with a bias): each QKV product stores plainly -- in latency mode the
    // split-K reduce does -- and one sweep per product norms every q / k head and rotates it (lr_launch_qk_norm_rope)
    const u16 *const qn = h->q_norm ? h->q_norm[l] : nullptr, *const kn = h->k_norm ? h->k_norm[l] : nullptr;
    const int epi_qkv = qn ? LR_EPI_STORE : LR_EPI_ROPE;
    if (last_q_only) {
      LR_RUN(lr_launch_gemm({.A = ws.xn, .B = w.wqkv + (size_t)q_w * d, .C = ws.qkv, .M = n, .N = kv_w, .K = d,
                             .epi = epi_qkv, .variant = gv, .rope = qn ? LrGemmRope{} : rope(ws.tok_pos, kv_w / 2),
                             .bias = bias ? bias + q_w : nullptr, .splitk = ws.splitk}, st));
      if (qn) LR_RUN(lr_launch_qk_norm_rope(ws.qkv, n, kv_w, 0, nkv, hd, nullptr, kn, c.rms_eps, ws.tok_pos, rope_l, st, qk_ns));
      LR_RUN(lr_launch_gather_rows(ws.xn, ws.last_rows, B, d, ws.xn_last, st));
      LR_RUN(lr_launch_gemm({.A = ws.xn_last, .B = w.wqkv, .C = ws.q_last, .M = B, .N = q_w, .K = d, .epi = epi_qkv,
                             .variant = pv, .rope = qn ? LrGemmRope{} : rope(ws.last_pos, q_w), .bias = bias,
                             .splitk = ws.splitk}, st));
      if (qn) LR_RUN(lr_launch_qk_norm_rope(ws.q_last, B, q_w, nh, 0, hd, qn, nullptr, c.rms_eps, ws.last_pos, rope_l, st, qk_ns));
      LR_RUN(lr_launch_attention_last(ws.qkv, ws.q_last, ws.att_last, attn.cu, attn.cu_host, S, n, nh, nkv, hd, st, P, a_scale,
                                      a_cap, win));
    } else {
      LR_RUN(lr_launch_gemm({.A = folded ? ws.x : ws.xn, .B = folded ? h->wqkv_folded[l] : w.wqkv, .C = ws.qkv, .M = n,
                             .N = q_w + kv_w, .K = d, .epi = epi_qkv, .variant = gv,
                             .rope = qn ? LrGemmRope{} : rope(ws.tok_pos, q_w + kv_w / 2),
                             .row_scale = folded ? ws.rstd : nullptr, .bias = bias, .splitk = ws.splitk}, st));
      if (qn) LR_RUN(lr_launch_qk_norm_rope(ws.qkv, n, q_w + kv_w, nh, nkv, hd, qn, kn, c.rms_eps, ws.tok_pos, rope_l, st, qk_ns));
    }
    if (!last_pruned) {
      LR_RUN(lr_launch_attention(attn_l, kernel_l, st));
    } else {
      // Only each prompt's LAST token is consumed after the final layer (model/llm.py:131), so the
      // last layer needs K/V for every token but attention output, o_proj, and the MLP for B rows only.
      // last_q_only: ws.att_last already holds the attention rows of the last tokens
      if (!last_q_only && mfma_l) {
        LR_RUN(lr_launch_attention(attn_l, kernel_l, st));
        LR_RUN(lr_launch_gather_rows(ws.att, ws.last_rows, B, nh * hd, ws.att_last, st));
      } else if (!last_q_only) {
        LR_RUN(lr_launch_attention_rows(ws.qkv, ws.att_last, cu, B, ws.last_rows, B, nh, nkv, hd, st, a_scale, a_cap, win));
      }
      LR_RUN(lr_launch_gather_rows(ws.x, ws.last_rows, B, d, ws.x_last, st));
      ws.compact = true;   // and this was the last layer
    }
    // o_proj and the MLP: on every row, or -- pruned last layer -- on the B compact rows (b_row_gemm_variant, never folded)
    const LayerRows& r = last_pruned ? last : full;
    const bool fold_mlp = folded && !last_pruned;
    if (sandwich) {
      // Both products store plainly into r.xn, which is free by then (its last reader was the QKV, resp. the gate-up, product;
      // the split-K form of the latency mode reduces without a residual), and one element-wise kernel per product normalises
      // that row, adds it to r.x in place and writes the norm the next product reads back into r.xn. Never folded.
      LR_RUN(lr_launch_gemm({.A = r.att, .B = w.wo, .C = r.xn, .M = r.M, .N = d, .K = nh * hd, .variant = r.gemm_variant,
                             .splitk = ws.splitk}, st));
      LR_RUN(lr_launch_residual_postnorm(r.x, r.xn, h->attn_out_norm[l], w.post_norm, r.xn, r.M, d, c.rms_eps, st));
      LR_RUN(lr_launch_gemm({.A = r.xn, .B = w.wgu, .C = r.hmid, .M = r.M, .N = 2 * f, .K = d, .epi = epi_mlp,
                             .variant = r.gemm_variant, .splitk = ws.splitk}, st));
      LR_RUN(lr_launch_gemm({.A = r.hmid, .B = w.wdown, .C = r.xn, .M = r.M, .N = d, .K = f, .variant = r.gemm_variant,
                             .splitk = ws.splitk}, st));
      const u16* next_norm = l + 1 < c.num_layers ? h->layers[l + 1].input_norm : nullptr;
      LR_RUN(lr_launch_residual_postnorm(r.x, r.xn, h->mlp_out_norm[l], next_norm, r.xn, r.M, d, c.rms_eps, st));
      input_normed = next_norm != nullptr;
      continue;
    }
    bool post_normed = false;   // a split-K product's reduce pass also writes the RMSNorm that follows (same bits)
    LR_RUN(lr_launch_gemm({.A = r.att, .B = w.wo, .C = r.x, .R = r.x, .M = r.M, .N = d, .K = nh * hd, .epi = LR_EPI_RESIDUAL,
                           .variant = r.gemm_variant, .splitk = ws.splitk,
                           .then_norm = {.w = fold_mlp ? nullptr : w.post_norm, .out = r.xn, .eps = c.rms_eps, .style = ns,
                                         .done = &post_normed}}, st));
    if (fold_mlp && !EXP_SKIP_SWEEP) LR_RUN(lr_launch_rms_rstd(r.x, ws.rstd, r.M, d, c.rms_eps, st));
    if (!fold_mlp && !post_normed) LR_RUN(lr_launch_rmsnorm(r.x, w.post_norm, r.xn, r.M, d, c.rms_eps, nullptr, st, ns));
    LR_RUN(lr_launch_gemm({.A = fold_mlp ? r.x : r.xn, .B = fold_mlp ? h->wgu_folded[l] : w.wgu, .C = r.hmid, .M = r.M,
                           .N = 2 * f, .K = d, .epi = epi_mlp, .variant = r.gemm_variant,
                           .row_scale = fold_mlp ? ws.rstd : nullptr, .splitk = ws.splitk}, st));
    // down_proj; its reduce pass (latency mode) also writes the NEXT layer's input RMSNorm when there is one and it reads
    // ws.xn (not folded)
    LR_RUN(lr_launch_gemm({.A = r.hmid, .B = w.wdown, .C = r.x, .R = r.x, .M = r.M, .N = d, .K = f, .epi = LR_EPI_RESIDUAL,
                           .variant = r.gemm_variant, .splitk = ws.splitk,
                           .then_norm = {.w = l + 1 < c.num_layers && !folded ? h->layers[l + 1].input_norm : nullptr,
                                         .out = r.xn, .eps = c.rms_eps, .style = ns, .done = &input_normed}}, st));
  }
#undef EXP_SKIP_SWEEP
  *out_ws = ws;
  return LR_OK;
}

static int prefill_head(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens, const int32_t* cu_seqlens_host,
                        int32_t B, int32_t prefix_len, const int32_t* class_ids, int32_t C, float* out, void* workspace,
                        size_t workspace_bytes, hipStream_t st) {
  LlamaWs ws;
  LR_RUN(run_body(h, packed_ids, cu_seqlens, cu_seqlens_host, B, prefix_len, workspace, workspace_bytes, st, &ws));
  return lr_launch_head(ws.compact ? ws.x_last : ws.x, ws.compact ? nullptr : ws.last_rows, h->final_norm, h->lm_head,
                        class_ids, B, C, h->cfg.hidden_size, h->cfg.rms_eps, out, h->cfg.vocab_size, st, ws.prefix_bad,
                        h->arch.norm_style, h->final_softcap);
}

extern "C" int lr_llama_prefill_verbalize(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                                          const int32_t* cu_seqlens_host, int32_t B,
                                          const int32_t* label_token_ids, int32_t C, float* out_scores,
                                          void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!label_token_ids || !out_scores || C < 1) LR_FAIL(LR_EINVAL, "lr_llama_prefill_verbalize: bad label ids / output");
  return prefill_head(h, packed_ids, cu_seqlens, cu_seqlens_host, B, 0, label_token_ids, C, out_scores, workspace,
                      workspace_bytes, (hipStream_t)hip_stream);
}

extern "C" int lr_llama_prefill_verbalize_prefix(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                                                 const int32_t* cu_seqlens_host, int32_t B, int32_t prefix_len,
                                                 const int32_t* label_token_ids, int32_t C, float* out_scores,
                                                 void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!label_token_ids || !out_scores || C < 1)
    LR_FAIL(LR_EINVAL, "lr_llama_prefill_verbalize_prefix: bad label ids / output");
  return prefill_head(h, packed_ids, cu_seqlens, cu_seqlens_host, B, prefix_len, label_token_ids, C, out_scores, workspace,
                      workspace_bytes, (hipStream_t)hip_stream);
}

extern "C" int lr_llama_last_logits(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                                    const int32_t* cu_seqlens_host, int32_t B, float* out_logits,
                                    void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!out_logits) LR_FAIL(LR_EINVAL, "lr_llama_last_logits: null output");
  return prefill_head(h, packed_ids, cu_seqlens, cu_seqlens_host, B, 0, nullptr, h ? h->cfg.vocab_size : 0, out_logits,
                      workspace, workspace_bytes, (hipStream_t)hip_stream);
}

extern "C" int32_t lr_common_prefix_len(const int32_t* packed_ids_host, const int32_t* cu_seqlens_host, int32_t B) {
  if (!packed_ids_host || !cu_seqlens_host || B < 2) return 0;
  int n = 0x7fffffff;
  for (int b = 0; b < B; ++b) {
    const int t = cu_seqlens_host[b + 1] - cu_seqlens_host[b];
    if (t - 1 < n) n = t - 1;
  }
  if (n <= 0) return 0;
  const int32_t* head = packed_ids_host + cu_seqlens_host[0];
  for (int b = 1; b < B && n > 0; ++b) {
    const int32_t* p = packed_ids_host + cu_seqlens_host[b];
    int i = 0;
    while (i < n && p[i] == head[i]) ++i;
    n = i;
  }
  return n;
}

extern "C" int lr_llama_pack_gate_up(const uint16_t* gate, const uint16_t* up, int32_t inter, int32_t hidden,
                                     uint16_t* out) {
  if (!gate || !up || !out || inter < 16 || inter % 16 != 0 || hidden < 1)
    LR_FAIL(LR_EINVAL, "lr_llama_pack_gate_up: inter=%d (must be a multiple of 16) hidden=%d", inter, hidden);
  for (int t = 0; t < inter / 16; ++t) {
    memcpy(out + (size_t)(32 * t) * hidden, gate + (size_t)(16 * t) * hidden, (size_t)16 * hidden * 2);
    memcpy(out + (size_t)(32 * t + 16) * hidden, up + (size_t)(16 * t) * hidden, (size_t)16 * hidden * 2);
  }
  return LR_OK;
}

extern "C" int lr_llama_pack_qkv(const uint16_t* q, const uint16_t* k, const uint16_t* v, int32_t num_heads,
                                 int32_t num_kv_heads, int32_t head_dim, int32_t hidden, uint16_t* out) {
  if (!q || !k || !v || !out || num_heads < 1 || num_kv_heads < 1 || head_dim < 2 || head_dim % 2 || hidden < 1)
    LR_FAIL(LR_EINVAL, "lr_llama_pack_qkv: bad arguments");
  const int half = head_dim / 2;
  const size_t rb = (size_t)hidden * 2;
  size_t o = 0;
  for (int part = 0; part < 2; ++part) {
    const uint16_t* src = part == 0 ? q : k;
    const int heads = part == 0 ? num_heads : num_kv_heads;
    for (int hh = 0; hh < heads; ++hh)
      for (int i = 0; i < half; ++i) {
        memcpy(out + (o++) * hidden, src + ((size_t)hh * head_dim + i) * hidden, rb);
        memcpy(out + (o++) * hidden, src + ((size_t)hh * head_dim + half + i) * hidden, rb);
      }
  }
  memcpy(out + o * hidden, v, (size_t)num_kv_heads * head_dim * rb);
  return LR_OK;
}

extern "C" int lr_gemm_splitk_plan(int32_t variant, int32_t M, int32_t N, int32_t K, size_t workspace_bytes, int32_t* splits,
                                   int32_t* rows_per_launch) {
  return lr_gemm_splitk_plan_of(variant, M, N, K, workspace_bytes, splits, rows_per_launch);
}

extern "C" int lr_gemm_bf16_nt(const uint16_t* A, const uint16_t* B, uint16_t* C, int32_t M, int32_t N,
                               int32_t K, int32_t variant, void* hip_stream) {
  if (!A || !B || !C) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt: null pointer");
  return lr_launch_gemm({.A = A, .B = B, .C = C, .M = M, .N = N, .K = K, .variant = variant}, (hipStream_t)hip_stream);
}

extern "C" int lr_gemm_bf16_nt_ws(const uint16_t* A, const uint16_t* B, uint16_t* C, int32_t M, int32_t N,
                                  int32_t K, int32_t variant, void* workspace, size_t workspace_bytes,
                                  void* hip_stream) {
  if (!A || !B || !C) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_ws: null pointer");
  return lr_launch_gemm({.A = A, .B = B, .C = C, .M = M, .N = N, .K = K, .variant = variant,
                         .splitk = {.ws = (float*)workspace, .bytes = workspace_bytes}}, (hipStream_t)hip_stream);
}

extern "C" int lr_gemm_bf16_nt_epi(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M,
                                   int32_t N, int32_t K, int32_t epilogue, int32_t variant, const int32_t* tok_pos,
                                   const float* rope_cs, int32_t rope_positions, int32_t head_dim, int32_t rot_cols,
                                   void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!A || !B || !C) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_epi: null pointer");
  if (epilogue < LR_EPI_STORE || epilogue > LR_EPI_GEGLU || epilogue == LR_EPI_PARTIAL)
    LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_epi: epilogue %d", epilogue);
  // the packed half of lr_rope_table's buffer sits behind the fp32 half
  const unsigned* cs16 = (rope_cs && rope_positions > 0 && head_dim >= 2)
                             ? reinterpret_cast<const unsigned*>(rope_cs + (size_t)rope_positions * head_dim) : nullptr;
  return lr_launch_gemm({.A = A, .B = B, .C = C, .R = R, .M = M, .N = N, .K = K, .epi = epilogue, .variant = variant,
                         .rope = {.tok_pos = tok_pos, .cs = rope_cs, .cs16 = cs16, .head_dim = head_dim, .rot_cols = rot_cols},
                         .splitk = {.ws = (float*)workspace, .bytes = workspace_bytes}}, (hipStream_t)hip_stream);
}

extern "C" int lr_gemm_bf16_nt_bias_epi(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M,
                                        int32_t N, int32_t K, int32_t epilogue, int32_t variant, const int32_t* tok_pos,
                                        const float* rope_cs, int32_t rope_positions, int32_t head_dim, int32_t rot_cols,
                                        void* workspace, size_t workspace_bytes, const uint16_t* bias, void* hip_stream) {
  if (!A || !B || !C) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_bias_epi: null pointer");
  if (epilogue < LR_EPI_STORE || epilogue > LR_EPI_GEGLU || epilogue == LR_EPI_PARTIAL)
    LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_bias_epi: epilogue %d", epilogue);
  const unsigned* cs16 = (rope_cs && rope_positions > 0 && head_dim >= 2)
                             ? reinterpret_cast<const unsigned*>(rope_cs + (size_t)rope_positions * head_dim) : nullptr;
  return lr_launch_gemm({.A = A, .B = B, .C = C, .R = R, .M = M, .N = N, .K = K, .epi = epilogue, .variant = variant,
                         .rope = {.tok_pos = tok_pos, .cs = rope_cs, .cs16 = cs16, .head_dim = head_dim, .rot_cols = rot_cols},
                         .bias = bias, .splitk = {.ws = (float*)workspace, .bytes = workspace_bytes}}, (hipStream_t)hip_stream);
}

extern "C" int lr_gemm_bf16_nt_residual_rmsnorm_ex(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R,
                                                   int32_t M, int32_t N, int32_t K, int32_t variant, const uint16_t* norm_w,
                                                   uint16_t* norm_out, float eps, int32_t norm_style, int32_t fuse,
                                                   int32_t* was_fused, void* workspace, size_t workspace_bytes,
                                                   void* hip_stream) {
  if (!A || !B || !C || !R || !norm_w || !norm_out) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_residual_rmsnorm: null pointer");
  if (norm_style != 0 && norm_style != 1) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_residual_rmsnorm_ex: norm_style %d", norm_style);
  hipStream_t st = (hipStream_t)hip_stream;
  bool done = false;
  LR_RUN(lr_launch_gemm({.A = A, .B = B, .C = C, .R = R, .M = M, .N = N, .K = K, .epi = LR_EPI_RESIDUAL, .variant = variant,
                         .splitk = {.ws = (float*)workspace, .bytes = workspace_bytes},
                         .then_norm = {.w = fuse ? norm_w : nullptr, .out = norm_out, .eps = eps, .style = norm_style,
                                       .done = &done}}, st));
  if (was_fused) *was_fused = done ? 1 : 0;
  if (done) return LR_OK;
  return lr_launch_rmsnorm(C, norm_w, norm_out, M, N, eps, nullptr, st, norm_style);
}

extern "C" int lr_gemm_bf16_nt_residual_rmsnorm(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R,
                                                int32_t M, int32_t N, int32_t K, int32_t variant, const uint16_t* norm_w,
                                                uint16_t* norm_out, float eps, int32_t fuse, int32_t* was_fused,
                                                void* workspace, size_t workspace_bytes, void* hip_stream) {
  return lr_gemm_bf16_nt_residual_rmsnorm_ex(A, B, C, R, M, N, K, variant, norm_w, norm_out, eps, 0, fuse, was_fused,
                                             workspace, workspace_bytes, hip_stream);
}

extern "C" size_t lr_rope_table_bytes(int32_t max_positions, int32_t head_dim) {
  if (max_positions < 1 || head_dim < 2) return 0;
  return (size_t)max_positions * (head_dim / 2) * (2 * sizeof(float) + sizeof(unsigned));
}

extern "C" int lr_rope_table(float* cs, int32_t max_positions, int32_t head_dim, float theta, void* hip_stream) {
  if (!cs || max_positions < 1 || head_dim < 2) LR_FAIL(LR_EINVAL, "lr_rope_table: bad argument");
  return lr_launch_rope_table(cs, max_positions, head_dim, theta, (hipStream_t)hip_stream,
                              reinterpret_cast<unsigned*>(cs + (size_t)max_positions * head_dim));
}

extern "C" int lr_rope_table_ex(float* cs, int32_t max_positions, int32_t head_dim, float theta, const LrRopeScaling* s,
                                void* hip_stream) {
  if (!cs || max_positions < 1 || head_dim < 2) LR_FAIL(LR_EINVAL, "lr_rope_table_ex: bad argument");
  return lr_launch_rope_table(cs, max_positions, head_dim, theta, (hipStream_t)hip_stream,
                              reinterpret_cast<unsigned*>(cs + (size_t)max_positions * head_dim), s);
}

extern "C" int lr_attention_varlen(const uint16_t* qkv, uint16_t* out, const int32_t* cu_seqlens,
                                   const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads,
                                   int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* hip_stream) {
  if (!qkv || !out || !cu_seqlens || !cu_seqlens_host || B < 1) LR_FAIL(LR_EINVAL, "lr_attention_varlen: bad argument");
  if (int rc = lr_check_segments(cu_seqlens_host, B, "lr_attention_varlen")) return rc;
  LrAttnKernel kernel;
  if (int rc = lr_resolve_attention({.variant = variant, .hd = head_dim}, &kernel)) return rc;
  return lr_launch_attention({.qkv = qkv, .out = out, .cu = cu_seqlens, .cu_host = cu_seqlens_host, .S = B,
                              .n_tok = cu_seqlens_host[B], .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim},
                             kernel, (hipStream_t)hip_stream);
}

// Host checks of the two shared-prefix entry points, before any launch: segments, segment 0 = the prefix, head shapes and
// the (variant, head_dim) pairs whose kernel has the mode.
static int check_prefix_request(const char* who, const int32_t* cu_host, int S, int prefix_len, int nh, int nkv, int hd,
                                int variant) {
  if (!cu_host || S < 1 || prefix_len < 0 || nh < 1 || nkv < 1) LR_FAIL(LR_EINVAL, "%s: bad argument", who);
  if (int rc = lr_check_segments(cu_host, S, who)) return rc;
  if (nh % nkv != 0) LR_FAIL(LR_EINVAL, "%s: num_heads %d not a multiple of num_kv_heads %d", who, nh, nkv);
  if (prefix_len > 0 && (S < 2 || cu_host[1] != prefix_len))
    LR_FAIL(LR_EINVAL, "%s: segment 0 has %d rows, the shared prefix %d (and a prompt must follow it)", who, cu_host[1], prefix_len);
  const bool ok = (hd == 128 && (variant == 0 || variant == 2)) || (hd == 64 && (variant == 0 || variant == 5)) ||
                  (hd == 96 && (variant == 0 || variant == 7 || variant == 8)) || (hd == 256 && (variant == 0 || variant == 4 || variant == 9));
  if (!ok)
    LR_FAIL(LR_EUNSUPPORTED, "%s: variant %d at head_dim %d (0 / 2 at 128, 0 / 5 at 64, 0 / 7 / 8 at 96, 0 / 4 / 9 at 256)", who, variant, hd);
  return LR_OK;
}

extern "C" int lr_attention_varlen_prefix(const uint16_t* qkv, uint16_t* out, const int32_t* seg_starts,
                                          const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                                          int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* hip_stream) {
  if (!qkv || !out || !seg_starts) LR_FAIL(LR_EINVAL, "lr_attention_varlen_prefix: null pointer");
  LR_RUN(check_prefix_request("lr_attention_varlen_prefix", seg_starts_host, S, prefix_len, num_heads, num_kv_heads, head_dim,
                              variant));
  LrAttnKernel kernel;
  LR_RUN(lr_resolve_attention({.variant = variant, .hd = head_dim, .prefix_len = prefix_len, .prefill = true}, &kernel));
  return lr_launch_attention({.qkv = qkv, .out = out, .cu = seg_starts, .cu_host = seg_starts_host, .S = S,
                              .n_tok = seg_starts_host[S], .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim,
                              .prefix_len = prefix_len}, kernel, (hipStream_t)hip_stream);
}

extern "C" int lr_attention_last_rows(const uint16_t* kv, const uint16_t* q_last, uint16_t* out_last, const int32_t* seg_starts,
                                      const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                                      int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* hip_stream) {
  if (!kv || !q_last || !out_last || !seg_starts) LR_FAIL(LR_EINVAL, "lr_attention_last_rows: null pointer");
  LR_RUN(check_prefix_request("lr_attention_last_rows", seg_starts_host, S, prefix_len, num_heads, num_kv_heads, head_dim,
                              variant));
  return lr_launch_attention_last(kv, q_last, out_last, seg_starts, seg_starts_host, S, seg_starts_host[S], num_heads,
                                  num_kv_heads, head_dim, (hipStream_t)hip_stream, prefix_len);
}

// cap = 0: the uncapped entry point's own path (and bits); a scale other than head_dim^-0.5 then has no kernel
static int check_softcap_request(const char* who, float scale, float cap, int hd, bool* capped) {
  if (!finite_nonneg(scale) || !finite_nonneg(cap)) LR_FAIL(LR_EINVAL, "%s: scale %g cap %g (finite and >= 0)", who, (double)scale, (double)cap);
  *capped = cap > 0.f;
  if (!*capped && scale > 0.f && hd > 0 && scale != 1.0f / sqrtf((float)hd))
    LR_FAIL(LR_EUNSUPPORTED, "%s: scale %g without a cap (the uncapped kernels scale by head_dim^-0.5)", who, (double)scale);
  return LR_OK;
}

extern "C" int lr_attention_varlen_softcap(const uint16_t* qkv, uint16_t* out, const int32_t* seg_starts,
                                           const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                                           int32_t num_kv_heads, int32_t head_dim, float scale, float cap, int32_t variant,
                                           void* hip_stream) {
  const char* who = "lr_attention_varlen_softcap";
  bool capped;
  LR_RUN(check_softcap_request(who, scale, cap, head_dim, &capped));
  if (!capped)
    return lr_attention_varlen_prefix(qkv, out, seg_starts, seg_starts_host, S, prefix_len, num_heads, num_kv_heads, head_dim,
                                      variant, hip_stream);
  if (!qkv || !out || !seg_starts) LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  if (!seg_starts_host || S < 1 || prefix_len < 0 || num_heads < 1 || num_kv_heads < 1 || head_dim < 1 || head_dim > 256)
    LR_FAIL(LR_EINVAL, "%s: bad argument", who);
  LR_RUN(lr_check_segments(seg_starts_host, S, who));
  if (num_heads % num_kv_heads != 0)
    LR_FAIL(LR_EINVAL, "%s: num_heads %d not a multiple of num_kv_heads %d", who, num_heads, num_kv_heads);
  if (prefix_len > 0 && (S < 2 || seg_starts_host[1] != prefix_len))
    LR_FAIL(LR_EINVAL, "%s: segment 0 has %d rows, the shared prefix %d (and a prompt must follow it)", who, seg_starts_host[1],
            prefix_len);
  LrAttnKernel kernel;
  LR_RUN(lr_resolve_attention({.variant = variant, .hd = head_dim, .prefix_len = prefix_len, .prefill = true, .cap = cap},
                              &kernel));
  const float sc = scale > 0.f ? scale : 1.0f / sqrtf((float)head_dim);
  return lr_launch_attention({.qkv = qkv, .out = out, .cu = seg_starts, .cu_host = seg_starts_host, .S = S,
                              .n_tok = seg_starts_host[S], .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim,
                              .prefix_len = prefix_len, .scale = sc, .cap = cap}, kernel, (hipStream_t)hip_stream);
}

extern "C" int lr_attention_last_rows_softcap(const uint16_t* kv, const uint16_t* q_last, uint16_t* out_last,
                                              const int32_t* seg_starts, const int32_t* seg_starts_host, int32_t S,
                                              int32_t prefix_len, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim,
                                              float scale, float cap, int32_t variant, void* hip_stream) {
  const char* who = "lr_attention_last_rows_softcap";
  bool capped;
  LR_RUN(check_softcap_request(who, scale, cap, head_dim, &capped));
  if (!capped)
    return lr_attention_last_rows(kv, q_last, out_last, seg_starts, seg_starts_host, S, prefix_len, num_heads, num_kv_heads,
                                  head_dim, variant, hip_stream);
  if (!kv || !q_last || !out_last || !seg_starts) LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  if (!seg_starts_host || S < 1 || prefix_len < 0 || num_heads < 1 || num_kv_heads < 1) LR_FAIL(LR_EINVAL, "%s: bad argument", who);
  LR_RUN(lr_check_segments(seg_starts_host, S, who));
  if (num_heads % num_kv_heads != 0)
    LR_FAIL(LR_EINVAL, "%s: num_heads %d not a multiple of num_kv_heads %d", who, num_heads, num_kv_heads);
  if (prefix_len > 0 && (S < 2 || seg_starts_host[1] != prefix_len))
    LR_FAIL(LR_EINVAL, "%s: segment 0 has %d rows, the shared prefix %d (and a prompt must follow it)", who, seg_starts_host[1],
            prefix_len);
  LrAttnKernel kernel;
  LR_RUN(lr_resolve_attention({.variant = variant, .hd = head_dim, .prefix_len = prefix_len, .prefill = true, .cap = cap},
                              &kernel));
  if (kernel != LR_ATTN_HD256)
    LR_FAIL(LR_EUNSUPPORTED, "%s: variant %d at head_dim %d has no one-row mode with a cap (0 / 4 at 256)", who, variant, head_dim);
  return lr_launch_attention_last(kv, q_last, out_last, seg_starts, seg_starts_host, S, seg_starts_host[S], num_heads,
                                  num_kv_heads, head_dim, (hipStream_t)hip_stream, prefix_len,
                                  scale > 0.f ? scale : 1.0f / sqrtf((float)head_dim), cap);
}

// The windowed pair (Gemma-3's sliding layers). A window that masks nothing -- <= 0, or >= the longest segment -- is the plain
// causal call: the uncapped entry point's own path (and bits).
static int check_window_request(const char* who, const int32_t* cu_host, int S, int prefix_len, int nh, int nkv, int hd,
                                int window, bool* real) {
  *real = false;
  if (window <= 0) return LR_OK;
  int longest = 0;
  if (!cu_host || S < 1 || prefix_len < 0 || nh < 1 || nkv < 1 || hd < 1 || hd > 256) LR_FAIL(LR_EINVAL, "%s: bad argument", who);
  LR_RUN(lr_check_segments(cu_host, S, who, nullptr, &longest));
  if (window >= longest + (prefix_len > 0 ? prefix_len : 0)) return LR_OK;
  if (nh % nkv != 0) LR_FAIL(LR_EINVAL, "%s: num_heads %d not a multiple of num_kv_heads %d", who, nh, nkv);
  if (prefix_len > 0) LR_FAIL(LR_EUNSUPPORTED, "%s: a window of %d with a shared prefix of %d (the windowed kernels read none)", who,
                              window, prefix_len);
  *real = true;
  return LR_OK;
}

extern "C" int lr_attention_varlen_window(const uint16_t* qkv, uint16_t* out, const int32_t* seg_starts,
                                          const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                                          int32_t num_kv_heads, int32_t head_dim, int32_t window, int32_t variant,
                                          void* hip_stream) {
  const char* who = "lr_attention_varlen_window";
  bool real;
  LR_RUN(check_window_request(who, seg_starts_host, S, prefix_len, num_heads, num_kv_heads, head_dim, window, &real));
  if (!real)
    return lr_attention_varlen_prefix(qkv, out, seg_starts, seg_starts_host, S, prefix_len, num_heads, num_kv_heads, head_dim,
                                      variant, hip_stream);
  if (!qkv || !out || !seg_starts) LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  LrAttnKernel kernel;
  if (variant == 1 || ((variant == 0 || variant == 4) && head_dim != 256)) kernel = LR_ATTN_GENERIC;
  else if (variant == 0 || variant == 4) kernel = LR_ATTN_HD256;
  else LR_FAIL(LR_EUNSUPPORTED, "%s: variant %d has no windowed form (0 / 4: the head_dim-256 MFMA kernel, generic off head_dim "
               "256; 1 generic)", who, variant);
  return lr_launch_attention({.qkv = qkv, .out = out, .cu = seg_starts, .cu_host = seg_starts_host, .S = S,
                              .n_tok = seg_starts_host[S], .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim,
                              .window = window}, kernel, (hipStream_t)hip_stream);
}

extern "C" int lr_attention_last_rows_window(const uint16_t* kv, const uint16_t* q_last, uint16_t* out_last,
                                             const int32_t* seg_starts, const int32_t* seg_starts_host, int32_t S,
                                             int32_t prefix_len, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim,
                                             int32_t window, int32_t variant, void* hip_stream) {
  const char* who = "lr_attention_last_rows_window";
  bool real;
  LR_RUN(check_window_request(who, seg_starts_host, S, prefix_len, num_heads, num_kv_heads, head_dim, window, &real));
  if (!real)
    return lr_attention_last_rows(kv, q_last, out_last, seg_starts, seg_starts_host, S, prefix_len, num_heads, num_kv_heads,
                                  head_dim, variant, hip_stream);
  if (!kv || !q_last || !out_last || !seg_starts) LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  if (head_dim != 256 || (variant != 0 && variant != 4))
    LR_FAIL(LR_EUNSUPPORTED, "%s: variant %d at head_dim %d has no one-row mode with a window (0 / 4 at 256)", who, variant,
            head_dim);
  return lr_launch_attention_last(kv, q_last, out_last, seg_starts, seg_starts_host, S, seg_starts_host[S], num_heads,
                                  num_kv_heads, head_dim, (hipStream_t)hip_stream, 0, 0.f, 0.f, window);
}

extern "C" int lr_residual_postnorm_bf16(uint16_t* x, const uint16_t* hrows, const uint16_t* w_out, const uint16_t* w_next,
                                         uint16_t* xn, int32_t rows, int32_t d, float eps, void* hip_stream) {
  if (!x || !hrows || !w_out || rows < 1 || (w_next == nullptr) != (xn == nullptr) || !(eps >= 0.f) || !(eps < __builtin_inff()))
    LR_FAIL(LR_EINVAL, "lr_residual_postnorm_bf16: bad argument (w_next and xn go together)");
  return lr_launch_residual_postnorm(x, hrows, w_out, w_next, xn, rows, d, eps, (hipStream_t)hip_stream);
}

extern "C" int lr_rmsnorm_bf16(const uint16_t* x, const uint16_t* w, uint16_t* out, int32_t rows, int32_t d, float eps,
                               int32_t norm_style, void* hip_stream) {
  if (!x || !w || !out || rows < 1 || d < 8 || d % 8 != 0 || (norm_style != 0 && norm_style != 1) || !(eps >= 0.f) ||
      !(eps < __builtin_inff()))
    LR_FAIL(LR_EINVAL, "lr_rmsnorm_bf16: bad argument (rows %d, d %d a multiple of 8, norm_style %d)", rows, d, norm_style);
  return lr_launch_rmsnorm(x, w, out, rows, d, eps, nullptr, (hipStream_t)hip_stream, norm_style);
}

// ---- the prefill's norm, head, embedding and metadata kernels alone (exposed for parity tests) ---------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int lr_llama_head_bf16(const uint16_t* x, const int32_t* rows, const uint16_t* norm_w, const uint16_t* lm_head,
                                  const int32_t* class_ids, int32_t B, int32_t C, int32_t d, float eps, float* out,
                                  int32_t vocab, const int32_t* poison, int32_t norm_style, float final_softcap,
                                  void* hip_stream) {
  if (!x || !norm_w || !lm_head || !out) LR_FAIL(LR_EINVAL, "lr_llama_head_bf16: null pointer");
  if (B < 0 || C < 0 || vocab < 1) LR_FAIL(LR_EINVAL, "lr_llama_head_bf16: B %d, C %d, vocab %d", B, C, vocab);
  if (d < 8 || d % 8 != 0) LR_FAIL(LR_EINVAL, "lr_llama_head_bf16: d %d (a multiple of 8)", d);
  if (!finite_nonneg(eps)) LR_FAIL(LR_EINVAL, "lr_llama_head_bf16: eps %g (finite and >= 0)", (double)eps);
  if (norm_style != 0 && norm_style != 1) LR_FAIL(LR_EINVAL, "lr_llama_head_bf16: norm_style %d", norm_style);
  if (!finite_nonneg(final_softcap))
    LR_FAIL(LR_EINVAL, "lr_llama_head_bf16: final_softcap %g (finite and >= 0; 0 = none)", (double)final_softcap);
  if (final_softcap > 0.f && norm_style != 1)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_head_bf16: a final soft cap goes with the Gemma norm (norm_style 1)");
  // the normalised row lives in d * 2 bytes of dynamic LDS beside 16 static bytes; 64 KB without a raised attribute
  if ((size_t)d * sizeof(uint16_t) > (size_t)65536 - 64)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_head_bf16: d %d needs %zu bytes of LDS for the normalised row", d, (size_t)d * 2);
  if ((C + 31) / 32 > 65535) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_head_bf16: %d classes exceed the grid limit", C);
  if (!aligned16(lm_head)) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_head_bf16: lm_head must be 16-byte aligned");
  if (B == 0 || C == 0) return LR_OK;
  return lr_launch_head(x, rows, norm_w, lm_head, class_ids, B, C, d, eps, out, vocab, (hipStream_t)hip_stream, poison,
                        norm_style, final_softcap);
}

extern "C" int lr_llama_embed_bf16(const int32_t* ids, const int32_t* tok_src, const uint16_t* table, int32_t vocab, int32_t d,
                                   uint16_t* out, int32_t n, float scale, void* hip_stream) {
  if (!ids || !table || !out) LR_FAIL(LR_EINVAL, "lr_llama_embed_bf16: null pointer");
  if (n < 0 || vocab < 1) LR_FAIL(LR_EINVAL, "lr_llama_embed_bf16: n %d, vocab %d", n, vocab);
  if (d < 8 || d % 8 != 0) LR_FAIL(LR_EINVAL, "lr_llama_embed_bf16: d %d (a multiple of 8)", d);
  if (!(scale > -__builtin_inff()) || !(scale < __builtin_inff()))
    LR_FAIL(LR_EINVAL, "lr_llama_embed_bf16: scale %g is not finite", (double)scale);
  if (!aligned16(table) || !aligned16(out)) LR_FAIL(LR_EUNSUPPORTED, "lr_llama_embed_bf16: table and out must be 16-byte aligned");
  if (n == 0) return LR_OK;
  return lr_launch_embed(ids, tok_src, table, vocab, d, out, n, (hipStream_t)hip_stream, scale);
}

extern "C" int lr_llama_token_meta(const int32_t* cu, int32_t B, int32_t prefix_len, const int32_t* ids, int32_t* seg_start,
                                   int32_t* tok_pos, int32_t* tok_src, int32_t* last_rows, int32_t* last_pos,
                                   int32_t* prefix_bad, void* hip_stream) {
  if (!cu || !seg_start || !tok_pos) LR_FAIL(LR_EINVAL, "lr_llama_token_meta: null pointer");
  if (B < 0 || prefix_len < 0) LR_FAIL(LR_EINVAL, "lr_llama_token_meta: B %d, prefix_len %d", B, prefix_len);
  if (prefix_bad && !ids) LR_FAIL(LR_EINVAL, "lr_llama_token_meta: prefix_bad without ids (nothing would be verified)");
  if (B == 0) return LR_OK;
  return lr_launch_token_meta(cu, B, prefix_len, seg_start, tok_pos, tok_src, last_rows, (hipStream_t)hip_stream, last_pos, ids,
                              prefix_bad);
}

extern "C" int lr_gather_rows_bf16(const uint16_t* x, const int32_t* rows, int32_t n_rows, int32_t d, uint16_t* out,
                                   void* hip_stream) {
  if (!x || !rows || !out) LR_FAIL(LR_EINVAL, "lr_gather_rows_bf16: null pointer");
  if (n_rows < 0) LR_FAIL(LR_EINVAL, "lr_gather_rows_bf16: n_rows %d", n_rows);
  if (d < 8 || d % 8 != 0) LR_FAIL(LR_EINVAL, "lr_gather_rows_bf16: d %d (a multiple of 8)", d);
  if (!aligned16(x) || !aligned16(out)) LR_FAIL(LR_EUNSUPPORTED, "lr_gather_rows_bf16: x and out must be 16-byte aligned");
  return lr_launch_gather_rows(x, rows, n_rows, d, out, (hipStream_t)hip_stream);
}

extern "C" int lr_rms_rstd_f32(const uint16_t* x, float* rstd, int32_t rows, int32_t d, float eps, void* hip_stream) {
  if (!x || !rstd) LR_FAIL(LR_EINVAL, "lr_rms_rstd_f32: null pointer");
  if (rows < 0) LR_FAIL(LR_EINVAL, "lr_rms_rstd_f32: rows %d", rows);
  if (d < 8 || d % 8 != 0) LR_FAIL(LR_EINVAL, "lr_rms_rstd_f32: d %d (a multiple of 8)", d);
  if (!finite_nonneg(eps)) LR_FAIL(LR_EINVAL, "lr_rms_rstd_f32: eps %g (finite and >= 0)", (double)eps);
  if (!aligned16(x)) LR_FAIL(LR_EUNSUPPORTED, "lr_rms_rstd_f32: x must be 16-byte aligned");
  return lr_launch_rms_rstd(x, rstd, rows, d, eps, (hipStream_t)hip_stream);
}

extern "C" int lr_gemm_bf16_nt_rowscale_epi(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M,
                                            int32_t N, int32_t K, int32_t epilogue, int32_t variant, const int32_t* tok_pos,
                                            const float* rope_cs, int32_t rope_positions, int32_t head_dim, int32_t rot_cols,
                                            void* workspace, size_t workspace_bytes, const float* row_scale, void* hip_stream) {
  if (!A || !B || !C) LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_rowscale_epi: null pointer");
  if (epilogue < LR_EPI_STORE || epilogue > LR_EPI_GEGLU || epilogue == LR_EPI_PARTIAL)
    LR_FAIL(LR_EINVAL, "lr_gemm_bf16_nt_rowscale_epi: epilogue %d", epilogue);
  const unsigned* cs16 = (rope_cs && rope_positions > 0 && head_dim >= 2)
                             ? reinterpret_cast<const unsigned*>(rope_cs + (size_t)rope_positions * head_dim) : nullptr;
  return lr_launch_gemm({.A = A, .B = B, .C = C, .R = R, .M = M, .N = N, .K = K, .epi = epilogue, .variant = variant,
                         .rope = {.tok_pos = tok_pos, .cs = rope_cs, .cs16 = cs16, .head_dim = head_dim, .rot_cols = rot_cols},
                         .row_scale = row_scale, .splitk = {.ws = (float*)workspace, .bytes = workspace_bytes}},
                        (hipStream_t)hip_stream);
}

extern "C" int lr_qk_norm_rope_ex_bf16(uint16_t* buf, int32_t rows, int32_t ld, int32_t col0, int32_t nq, int32_t nk,
                                       int32_t head_dim, const uint16_t* q_norm, const uint16_t* k_norm, float eps,
                                       const int32_t* tok_pos, const float* rope_cs, void* hip_stream, int32_t norm_style) {
  if (norm_style != 0 && norm_style != 1) LR_FAIL(LR_EINVAL, "lr_qk_norm_rope_bf16: norm_style %d (0 Qwen3, 1 Gemma-3)", norm_style);
  if (!lr_qk_norm_head_dim_ok(head_dim))
    LR_FAIL(LR_EUNSUPPORTED, "lr_qk_norm_rope_bf16: head_dim %d (a power of two from 16 to 256)", head_dim);
  if (!buf || rows < 1 || ld < 8 || col0 < 0 || col0 % 8 != 0 || nq < 0 || nk < 0 || nq + nk < 1 ||
      (long long)col0 + (long long)(nq + nk) * head_dim > ld || !tok_pos || !rope_cs || !(eps >= 0.f) || !(eps < __builtin_inff()))
    LR_FAIL(LR_EINVAL, "lr_qk_norm_rope_bf16: bad argument (rows %d, ld %d, col0 %d a multiple of 8, %d + %d heads of %d)", rows,
            ld, col0, nq, nk, head_dim);
  return lr_launch_qk_norm_rope(buf + col0, rows, ld, nq, nk, head_dim, q_norm, k_norm, eps, tok_pos, rope_cs,
                                (hipStream_t)hip_stream, norm_style);
}

extern "C" int lr_qk_norm_rope_bf16(uint16_t* buf, int32_t rows, int32_t ld, int32_t col0, int32_t nq, int32_t nk,
                                    int32_t head_dim, const uint16_t* q_norm, const uint16_t* k_norm, float eps,
                                    const int32_t* tok_pos, const float* rope_cs, void* hip_stream) {
  return lr_qk_norm_rope_ex_bf16(buf, rows, ld, col0, nq, nk, head_dim, q_norm, k_norm, eps, tok_pos, rope_cs, hip_stream, 0);
}

extern "C" size_t lr_attention_workspace_bytes(int32_t total_tokens, int32_t B, int32_t num_heads) {
  if (total_tokens < 1 || B < 1 || num_heads < 1) return 0;
  return lr_attn256_ws_bytes(total_tokens, B, num_heads);
}

extern "C" int lr_attention_varlen_ws(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* cu_seqlens,
                                      const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads, int32_t num_kv_heads,
                                      int32_t head_dim, int32_t variant, void* workspace, size_t workspace_bytes,
                                      void* hip_stream) {
  if (!qkv || !out || !cu_seqlens || !cu_seqlens_host || B < 1) LR_FAIL(LR_EINVAL, "lr_attention_varlen_ws: bad argument");
  if (int rc = lr_check_segments(cu_seqlens_host, B, "lr_attention_varlen_ws")) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  const int n = cu_seqlens_host[B];
  LrAttnKernel kernel;
  // a variant-3 request always reaches the item-list builder, which reports a missing or short workspace (LR_EWORKSPACE)
  LR_RUN(lr_resolve_attention({.variant = variant, .hd = head_dim, .want_lse = lse != nullptr,
                               .have_items_ws = workspace != nullptr || variant == 3}, &kernel));
  if (kernel == LR_ATTN_ROWS256)
    if (int rc = lr_launch_attn256_items(cu_seqlens, B, n, num_heads, 0, workspace, workspace_bytes, st)) return rc;
  return lr_launch_attention({.qkv = qkv, .out = out, .lse = lse, .cu = cu_seqlens, .cu_host = cu_seqlens_host, .S = B,
                              .n_tok = n, .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim, .items_ws = workspace},
                             kernel, st);
}

// ---- ranker sessions: a per-user K / V cache of the prompt prefix ---------------------------------------------------
// Slot s of the caller's table = [num_layers][max_tokens] rows of [K rotated | V] (2 nkv hd bf16), padded to 256 bytes; row p of
// a layer is prompt position p. No header, no device-side length: what a slot holds is the caller's host state.
static size_t kv_slot_bytes(int num_layers, int nkv, int hd, int max_tokens) {
  return lr_align_up((size_t)num_layers * (size_t)max_tokens * 2 * nkv * hd * sizeof(u16), 256);
}

extern "C" size_t lr_llama_kv_cache_slot_bytes(int32_t num_layers, int32_t num_kv_heads, int32_t head_dim, int32_t max_tokens) {
  if (num_layers < 1 || num_kv_heads < 1 || head_dim < 4 || head_dim % 4 != 0 || head_dim > 256 || max_tokens < 1) return 0;
  return kv_slot_bytes(num_layers, num_kv_heads, head_dim, max_tokens);
}

// Host checks of a cached call, before any launch: the table, every prompt's slot, what it keeps and what it adds.
static int check_cache_request(const char* who, const void* table, int num_slots, int max_tokens, int max_positions, int nkv, int hd,
                               const int32_t* slots_host, const int32_t* cached_len_host, const int32_t* cu_host,
                               const int32_t* keep_host, int B) {
  if (!table || !slots_host || !cached_len_host || !cu_host) LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  if (reinterpret_cast<uintptr_t>(table) & 15) LR_FAIL(LR_EINVAL, "%s: the cache table is not 16-byte aligned", who);
  if (B < 1 || num_slots < 1 || max_tokens < 1) LR_FAIL(LR_EINVAL, "%s: B %d, num_slots %d, max_tokens %d", who, B, num_slots, max_tokens);
  if (cu_host[0] != 0) LR_FAIL(LR_EINVAL, "%s: cu_new[0] = %d (must be 0)", who, cu_host[0]);
  // one layer of a slot is what a key block's buffer descriptor addresses
  if ((long long)max_tokens * 2 * nkv * hd * 2 > 0x7fffffffLL)
    LR_FAIL(LR_EUNSUPPORTED, "%s: max_tokens %d rows of a slot layer exceed the 2 GiB a buffer descriptor addresses here", who, max_tokens);
  std::vector<int32_t> seen(slots_host, slots_host + B);
  for (int b = 0; b < B; ++b) {
    const int q_len = cu_host[b + 1] - cu_host[b], c = cached_len_host[b];
    if (slots_host[b] < 0 || slots_host[b] >= num_slots)
      LR_FAIL(LR_EINVAL, "%s: prompt %d names slot %d of %d", who, b, slots_host[b], num_slots);
    if (q_len < 1) LR_FAIL(LR_EINVAL, "%s: prompt %d adds %d tokens (at least 1)", who, b, q_len);
    if (c < 0) LR_FAIL(LR_EINVAL, "%s: prompt %d has cached_len %d", who, b, c);
    if ((long long)c + q_len > max_tokens)
      LR_FAIL(LR_EINVAL, "%s: prompt %d reaches %lld tokens, a slot holds %d", who, b, (long long)c + q_len, max_tokens);
    if ((long long)c + q_len > max_positions)
      LR_FAIL(LR_EINVAL, "%s: prompt %d reaches %lld tokens, max_positions is %d", who, b, (long long)c + q_len, max_positions);
    if (keep_host && (keep_host[b] < 0 || keep_host[b] > q_len))
      LR_FAIL(LR_EINVAL, "%s: prompt %d keeps %d of %d new tokens", who, b, keep_host[b], q_len);
  }
  for (int b = 0; b < B; ++b)   // B is a batch of users: the quadratic scan stays small
    for (int a = 0; a < b; ++a)
      if (seen[a] == seen[b]) LR_FAIL(LR_EINVAL, "%s: prompts %d and %d name the same slot %d", who, a, b, seen[b]);
  return LR_OK;
}

// The session calls run the plain Llama layer only, on the head_dim-128 MFMA kernel or the generic one.
static int check_cache_handle(const char* who, const lr_llama_t* h, bool* generic) {
  if (h->arch.norm_style != 0 || h->arch.mlp_act != 0 || h->gemma2 || h->gemma3)
    LR_FAIL(LR_EUNSUPPORTED, "%s: a handle with Gemma norms, soft caps or sliding windows has no cached form", who);
  if (h->attn_softcap > 0.f || h->final_softcap > 0.f) LR_FAIL(LR_EUNSUPPORTED, "%s: a handle with a soft cap has no cached form", who);
  if (h->q_norm) LR_FAIL(LR_EUNSUPPORTED, "%s: a handle with q/k norms has no cached form", who);
  if (h->bqkv) LR_FAIL(LR_EUNSUPPORTED, "%s: a handle with q/k/v biases has no cached form", who);
  if (h->wqkv_folded) LR_FAIL(LR_EUNSUPPORTED, "%s: a handle with folded norms has no cached form", who);
  const int v = h->attn_variant, hd = h->cfg.head_dim;
  if (v != 0 && v != 1 && v != 2)
    LR_FAIL(LR_EUNSUPPORTED, "%s: attention variant %d has no cached form (0 auto, 1 generic, 2 = head_dim-128 MFMA)", who, v);
  if (v == 2 && hd != 128) LR_FAIL(LR_EUNSUPPORTED, "%s: attention variant 2 needs head_dim 128 (got %d)", who, hd);
  *generic = v == 1 || hd != 128;
  return LR_OK;
}

// carve()'s buffers for the call's new rows, then rotary tables long enough for a whole cached prompt and the new rows' cache-row offsets
static LlamaWs carve_extend(const LrLlamaConfig& c, int max_new_tokens, int max_seqs, int max_tokens, char* base) {
  LlamaWs w = carve(c, max_new_tokens, max_seqs, base, false);
  size_t o = w.total;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += lr_align_up(bytes, 256);
    return base + at;
  };
  const size_t rope_rows = (size_t)(c.max_positions < max_tokens ? c.max_positions : max_tokens);
  w.rope = (float*)take(rope_rows * (c.head_dim / 2) * 2 * sizeof(float));
  w.rope16 = (unsigned*)take(rope_rows * (c.head_dim / 2) * sizeof(unsigned));
  w.row_off = (long long*)take((size_t)max_new_tokens * sizeof(long long));
  w.total = o;
  return w;
}

extern "C" size_t lr_llama_extend_workspace_bytes(const lr_llama_t* h, int32_t max_new_tokens, int32_t max_seqs, int32_t max_tokens) {
  if (!h || max_new_tokens < 1 || max_tokens < 1) return 0;
  if (max_seqs < 1) max_seqs = 1;
  if (max_seqs > max_new_tokens) max_seqs = max_new_tokens;
  return carve_extend(h->cfg, max_new_tokens, max_seqs, max_tokens, nullptr).total;
}

extern "C" int lr_llama_extend_verbalize(lr_llama_t* h, void* table, int32_t num_slots, int32_t max_tokens, const int32_t* slots,
                                         const int32_t* slots_host, const int32_t* cached_len, const int32_t* cached_len_host,
                                         const int32_t* new_ids, const int32_t* cu_new, const int32_t* cu_new_host,
                                         const int32_t* keep_host, int32_t B, const int32_t* label_token_ids, int32_t C,
                                         float* out_scores, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "lr_llama_extend_verbalize";
  if (!h || !slots || !cached_len || !new_ids || !cu_new || !keep_host || !label_token_ids || !out_scores || !workspace)
    LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  if (C < 1) LR_FAIL(LR_EINVAL, "%s: %d label ids", who, C);
  const LrLlamaConfig& c = h->cfg;
  const int d = c.hidden_size, f = c.intermediate_size, nh = c.num_heads, nkv = c.num_kv_heads, hd = c.head_dim;
  LR_RUN(check_cache_request(who, table, num_slots, max_tokens, c.max_positions, nkv, hd, slots_host, cached_len_host, cu_new_host,
                             keep_host, B));
  bool generic;
  LR_RUN(check_cache_handle(who, h, &generic));
  const int n = cu_new_host[B];
  int maxT = 0;
  for (int b = 0; b < B; ++b) {
    const int T = cached_len_host[b] + cu_new_host[b + 1] - cu_new_host[b];
    maxT = T > maxT ? T : maxT;
  }
  LlamaWs ws = carve_extend(c, n, B, max_tokens, (char*)workspace);
  if (ws.total > workspace_bytes)
    LR_FAIL(LR_EWORKSPACE, "%s: workspace needs %zu bytes for %d new tokens, have %zu", who, ws.total, n, workspace_bytes);
  hipStream_t st = (hipStream_t)hip_stream;
  // A row's bits must be those of the whole-prompt call in the handle's mode, so every n-row product must compute a row
  // independently of how many other rows its launch has. The default-mode products do. Variant 7 does too: its split is fixed by
  // the weight's shape and its row chunks couple nothing, so a variant-7 handle runs it here and gets the variant-7 whole prompt's
  // bits. Variant 5 chooses its split from the row count -- 160 new rows and the 460 of the whole prompt are summed in different
  // orders -- so a variant-5 handle runs the default-mode products here, with the default mode's bits.
  const int gv = h->gemm_variant == 5 ? 0 : h->gemm_variant;
  const int pv = gv == 7 ? 7 : ((gv == 0 || gv == 6) && B <= 256) ? 5 : 1;   // b_row_gemm_variant of that mode
  const int q_w = nh * hd, kv_w = 2 * nkv * hd;
  const long long slot_elems = (long long)(kv_slot_bytes(c.num_layers, nkv, hd, max_tokens) / sizeof(u16));
  // Variant 7, where the QKV product splits: its reduce pass stores K | V straight into the slot rows (LrGemmKvScatter) instead
  // of into ws.qkv for kv_cache_write_kernel to copy. LR_EXTEND_SEPARATE_CACHE_WRITE=1 keeps the two launches (tests and
  // benches only: the bitwise yardstick and the A/B arm; read per call).
  const char* const sep_env = getenv("LR_EXTEND_SEPARATE_CACHE_WRITE");
  const bool separate_write = gv != 7 || (sep_env && sep_env[0] == '1');
  auto reduce_writes_cache = [&](int N) {
    int splits = 1, rows = 0;
    return !separate_write && lr_gemm_splitk_plan_of(7, n, N, d, ws.splitk.bytes, &splits, &rows) == LR_OK && splits >= 2;
  };
  struct LayerRows { u16 *att, *x, *xn, *hmid; int M, gemm_variant; };   // what o_proj and the MLP run on
  const LayerRows full = {ws.att, ws.x, ws.xn, ws.hmid, n, gv}, last = {ws.att_last, ws.x_last, ws.xn_last, ws.h_last, B, pv};
  auto rope = [&](const int32_t* tok_pos, int rot_cols) {
    return LrGemmRope{.tok_pos = tok_pos, .cs = ws.rope, .cs16 = ws.rope16, .head_dim = hd, .rot_cols = rot_cols};
  };
  LR_RUN(lr_launch_kv_cache_meta(cu_new, cached_len, B, n, ws.tok_pos, ws.last_rows, ws.last_pos, st, slots, slot_elems, kv_w,
                                 ws.row_off));
  LR_RUN(lr_launch_rope_table(ws.rope, maxT, hd, c.rope_theta, st, ws.rope16, &h->rope_scaling));
  LR_RUN(lr_launch_embed(new_ids, nullptr, h->embed, c.vocab_size, d, ws.x, n, st, h->arch.embed_scale));
  bool input_normed = false;   // ws.xn already holds RMSNorm(ws.x) with this layer's input_norm
  for (int l = 0; l < c.num_layers; ++l) {
    const LrLlamaLayerWeights& w = h->layers[l];
    const bool last_pruned = l == c.num_layers - 1 && h->prune_last;
    // as run_body: Q for the last rows only where the kernel has a one-query-row mode; K | V for every new row either way,
    // because the next call reads them
    const bool last_q_only = last_pruned && !generic && gv != 1;
    u16* const kv_l = (u16*)table + (size_t)l * max_tokens * kv_w;
    LrAttnCachedArgs attn = {.q = ws.qkv, .q_ld = q_w + kv_w, .out = ws.att, .kv = kv_l, .slot_elems = slot_elems, .slots = slots,
                             .cached_len = cached_len, .cu = cu_new, .cached_len_host = cached_len_host, .cu_host = cu_new_host,
                             .B = B, .nh = nh, .nkv = nkv, .hd = hd, .generic = generic};
    if (!input_normed) LR_RUN(lr_launch_rmsnorm(ws.x, w.input_norm, ws.xn, n, d, c.rms_eps, nullptr, st, 0));
    if (last_q_only) {
      const bool fused = reduce_writes_cache(kv_w);   // every column is K | V: nothing goes to ws.qkv
      LR_RUN(lr_launch_gemm({.A = ws.xn, .B = w.wqkv + (size_t)q_w * d, .C = ws.qkv, .M = n, .N = kv_w, .K = d, .epi = LR_EPI_ROPE,
                             .variant = gv, .rope = rope(ws.tok_pos, kv_w / 2), .splitk = ws.splitk,
                             .kv_scatter = {.kv_layer = fused ? kv_l : nullptr, .row_off = ws.row_off, .col0 = 0}}, st));
      if (!fused) LR_RUN(lr_launch_kv_cache_write(ws.qkv, kv_w, 0, kv_w, cu_new, cached_len, slots, B, slot_elems, kv_l, n, st));
      LR_RUN(lr_launch_gather_rows(ws.xn, ws.last_rows, B, d, ws.xn_last, st));
      LR_RUN(lr_launch_gemm({.A = ws.xn_last, .B = w.wqkv, .C = ws.q_last, .M = B, .N = q_w, .K = d, .epi = LR_EPI_ROPE,
                             .variant = pv, .rope = rope(ws.last_pos, q_w), .splitk = ws.splitk}, st));
      attn.q = ws.q_last;
      attn.q_ld = q_w;
      attn.out = ws.att_last;
      attn.last = true;
      LR_RUN(lr_launch_attention_cached(attn, st));
    } else {
      const bool fused = reduce_writes_cache(q_w + kv_w);   // q stays in ws.qkv at its stride, the attention reads K | V from the slot
      LR_RUN(lr_launch_gemm({.A = ws.xn, .B = w.wqkv, .C = ws.qkv, .M = n, .N = q_w + kv_w, .K = d, .epi = LR_EPI_ROPE,
                             .variant = gv, .rope = rope(ws.tok_pos, q_w + kv_w / 2), .splitk = ws.splitk,
                             .kv_scatter = {.kv_layer = fused ? kv_l : nullptr, .row_off = ws.row_off, .col0 = q_w}}, st));
      if (!fused)
        LR_RUN(lr_launch_kv_cache_write(ws.qkv, q_w + kv_w, q_w, kv_w, cu_new, cached_len, slots, B, slot_elems, kv_l, n, st));
    }
    if (!last_pruned) {
      LR_RUN(lr_launch_attention_cached(attn, st));
    } else {
      if (!last_q_only && !generic) {   // every new row on the MFMA kernel, the last rows kept (run_body's order)
        LR_RUN(lr_launch_attention_cached(attn, st));
        LR_RUN(lr_launch_gather_rows(ws.att, ws.last_rows, B, nh * hd, ws.att_last, st));
      } else if (!last_q_only) {
        attn.out = ws.att_last;
        attn.last = true;
        attn.q_rows = ws.last_rows;
        LR_RUN(lr_launch_attention_cached(attn, st));
      }
      LR_RUN(lr_launch_gather_rows(ws.x, ws.last_rows, B, d, ws.x_last, st));
      ws.compact = true;   // and this was the last layer
    }
    const LayerRows& r = last_pruned ? last : full;
    bool post_normed = false;
    LR_RUN(lr_launch_gemm({.A = r.att, .B = w.wo, .C = r.x, .R = r.x, .M = r.M, .N = d, .K = nh * hd, .epi = LR_EPI_RESIDUAL,
                           .variant = r.gemm_variant, .splitk = ws.splitk,
                           .then_norm = {.w = w.post_norm, .out = r.xn, .eps = c.rms_eps, .style = 0, .done = &post_normed}}, st));
    if (!post_normed) LR_RUN(lr_launch_rmsnorm(r.x, w.post_norm, r.xn, r.M, d, c.rms_eps, nullptr, st, 0));
    LR_RUN(lr_launch_gemm({.A = r.xn, .B = w.wgu, .C = r.hmid, .M = r.M, .N = 2 * f, .K = d, .epi = LR_EPI_SWIGLU,
                           .variant = r.gemm_variant, .splitk = ws.splitk}, st));
    LR_RUN(lr_launch_gemm({.A = r.hmid, .B = w.wdown, .C = r.x, .R = r.x, .M = r.M, .N = d, .K = f, .epi = LR_EPI_RESIDUAL,
                           .variant = r.gemm_variant, .splitk = ws.splitk,
                           .then_norm = {.w = l + 1 < c.num_layers ? h->layers[l + 1].input_norm : nullptr, .out = r.xn,
                                         .eps = c.rms_eps, .style = 0, .done = &input_normed}}, st));
  }
  return lr_launch_head(ws.compact ? ws.x_last : ws.x, ws.compact ? nullptr : ws.last_rows, h->final_norm, h->lm_head,
                        label_token_ids, B, C, d, c.rms_eps, out_scores, c.vocab_size, st, nullptr, 0, 0.f);
}

extern "C" int lr_attention_varlen_cached(const uint16_t* qkv, uint16_t* out, void* table, int32_t num_slots, int32_t max_tokens,
                                          int32_t num_layers, int32_t layer, const int32_t* slots, const int32_t* slots_host,
                                          const int32_t* cached_len, const int32_t* cached_len_host, const int32_t* cu_q,
                                          const int32_t* cu_q_host, int32_t B, int32_t num_heads, int32_t num_kv_heads,
                                          int32_t head_dim, int32_t variant, void* hip_stream) {
  const char* who = "lr_attention_varlen_cached";
  if (!qkv || !out || !slots || !cached_len || !cu_q) LR_FAIL(LR_EINVAL, "%s: null pointer", who);
  if (num_heads < 1 || num_kv_heads < 1 || num_heads % num_kv_heads != 0 || head_dim < 4 || head_dim % 4 != 0 || head_dim > 256 ||
      num_layers < 1 || layer < 0 || layer >= num_layers)
    LR_FAIL(LR_EINVAL, "%s: heads %d / %d, head_dim %d, layer %d of %d", who, num_heads, num_kv_heads, head_dim, layer, num_layers);
  LR_RUN(check_cache_request(who, table, num_slots, max_tokens, 0x7fffffff, num_kv_heads, head_dim, slots_host, cached_len_host,
                             cu_q_host, nullptr, B));
  if (variant != 0 && variant != 1 && variant != 2)
    LR_FAIL(LR_EUNSUPPORTED, "%s: variant %d (0 auto, 1 generic, 2 = head_dim-128 MFMA)", who, variant);
  if (variant == 2 && head_dim != 128) LR_FAIL(LR_EUNSUPPORTED, "%s: variant 2 needs head_dim 128 (got %d)", who, head_dim);
  hipStream_t st = (hipStream_t)hip_stream;
  const int q_w = num_heads * head_dim, kv_w = 2 * num_kv_heads * head_dim, n = cu_q_host[B];
  const long long slot_elems = (long long)(kv_slot_bytes(num_layers, num_kv_heads, head_dim, max_tokens) / sizeof(u16));
  u16* const kv_l = (u16*)table + (size_t)layer * max_tokens * kv_w;
  LR_RUN(lr_launch_kv_cache_write(qkv, q_w + kv_w, q_w, kv_w, cu_q, cached_len, slots, B, slot_elems, kv_l, n, st));
  return lr_launch_attention_cached({.q = qkv, .q_ld = q_w + kv_w, .out = out, .kv = kv_l, .slot_elems = slot_elems, .slots = slots,
                                     .cached_len = cached_len, .cu = cu_q, .cached_len_host = cached_len_host, .cu_host = cu_q_host,
                                     .B = B, .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim,
                                     .generic = variant == 1 || head_dim != 128}, st);
}
