// llama_attn_hd256_softcap.hip -- the head_dim-256 MFMA attention (its text is attn_hd256_body in llama_attn_hd256_body.h: read
// it first) with soft-capped scores, cap * tanh(q.k * scale / cap), as Gemma-2 computes them: the body's SOFTCAP mode in the
// three forms variant 4 has, as kernels of their own in a translation unit of their own, so that the uncapped code objects of
// llama_attn_hd256.hip and llama_attn_hd256_prefix.hip hold what they held:
//
//   attn_hd256_softcap_kernel                 whole prompts
//   attn_hd256_softcap_prefix_kernel<false>   shared prompt prefix (prefix_len = P > 0)
//   attn_hd256_softcap_prefix_kernel<true>    the pruned last layer, one query row per prompt
//
// scale and cap are kernel arguments (query_pre_attn_scalar^-0.5 is a config value: 1/16 for gemma-2-2b / 9b, 1/12 for 27b).
// Contract as for variant 4: a row's bits depend on its own prompt only, and the prefix and last-row forms write the bits the
// whole-prompt kernel writes for the same row (same lines of the body; only the home of a staged K / V row differs).
// Forward only, no lse. Launch geometry, LDS (128 KiB) and the host checks are those of the uncapped launchers.
#include "llama_attn_hd256_body.h"

__global__ __launch_bounds__(512, 1) void attn_hd256_softcap_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                                    int nh, int nkv, int max_qblocks, int n_pairs, float scale,
                                                                    float cap) {
  attn_hd256_body<1, false, false, true>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, nullptr, scale, cap);
}

template <bool LASTQ>
__global__ __launch_bounds__(512, 1) void attn_hd256_softcap_prefix_kernel(const u16* __restrict__ qkv, u16* out,
                                                                           const int32_t* cu, int prefix_len, int nh, int nkv,
                                                                           int max_qblocks, int n_pairs,
                                                                           const u16* __restrict__ q_rows_last, float scale,
                                                                           float cap) {
  attn_hd256_body<1, LASTQ, true, true>(qkv, out, cu, prefix_len, nh, nkv, max_qblocks, n_pairs, q_rows_last, scale, cap);
}

static int check_cap(float scale, float cap) {
  if (!(cap > 0.f) || !(cap <= LR_SOFTCAP_MFMA_MAX) || !(scale > 0.f) || !(scale < __builtin_inff()))
    LR_FAIL(LR_EINVAL, "attention (soft cap, head_dim 256): scale %g cap %g (0 < cap <= %g: lr_resolve_attention sends larger "
            "caps to the generic kernel)", (double)scale, (double)cap, (double)LR_SOFTCAP_MFMA_MAX);
  return LR_OK;
}

// a.cap > 0, a.scale > 0; a.prefix_len = P > 0: segment 0 is the shared prefix the other segments continue
int lr_launch_attention_hd256_softcap(const LrAttnArgs& a, hipStream_t st) {
  const char *needs = "soft-capped MFMA attention needs head_dim 256", *no_lse = "attention: the head_dim-256 MFMA kernel writes no lse",
             *layout = "attention (soft cap, head_dim 256)";
  const auto cap_ok = [](const LrAttnArgs& a) { return check_cap(a.scale, a.cap); };
  if (a.prefix_len > 0)
    return lr_attn_launch_tiles<attn_hd256_softcap_prefix_kernel<false>, FA4_HD, FA4_QR, 512, FA4_LDS_BYTES, true>(
        "attn_hd256_softcap_kernel", needs, no_lse, cap_ok, layout, a, st, (const u16*)nullptr, a.scale, a.cap);
  return lr_attn_launch_tiles<attn_hd256_softcap_kernel, FA4_HD, FA4_QR, 512, FA4_LDS_BYTES, false>(
      "attn_hd256_softcap_kernel", needs, no_lse, cap_ok, layout, a, st, a.scale, a.cap);
}

// The pruned last layer with a cap
int lr_launch_attention_hd256_softcap_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu,
                                           const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int prefix_len, float scale,
                                           float cap, hipStream_t st) {
  LR_RUN(check_cap(scale, cap));
  return lr_attn_launch_last<attn_hd256_softcap_prefix_kernel<true>, FA4_HD, 512, FA4_LDS_BYTES>(
      "attn_hd256_softcap_prefix_kernel<last>", "attention (soft cap, last rows, head_dim 256)", kv, q_last, out_last, cu, cu_host,
      S, n_tok, nh, nkv, prefix_len, st, scale, cap);
}
