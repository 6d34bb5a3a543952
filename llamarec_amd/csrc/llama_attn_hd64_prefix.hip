// llama_attn_hd64_prefix.hip -- the head_dim-64 MFMA attention (variant 5; its text is attn_hd64_body in
// llama_attn_hd64_body.h: read it first) instantiated in the two modes attn_mfma128_kernel has in llama_attn.hip, as kernels of
// their own in a translation unit of their own, so that variant 5's code object holds variant 5 alone:
//
//   attn_hd64_prefix_kernel<false>  shared prompt prefix (prefix_len = P > 0): the body's PREFIX mode
//   attn_hd64_prefix_kernel<true>   the pruned last layer, one query row per prompt: the body's LASTQ mode
//
// Contract: a row's bits are those variant 5 writes for the same row of the same whole prompt. It holds because the block walk
// and the softmax are the same lines of the body in every mode; only the home of a staged K / V row differs, and the LDS image
// of a block is the same bytes either way (rows past the prompt's end are zero in both: the buffer descriptor's range check).
// The hand-placed `s_waitcnt vmcnt(0)` in front of every barrier covers both staging forms (the DMA is inline asm).
#include "llama_attn_hd64_body.h"

template <bool LASTQ>
__global__ __launch_bounds__(256, FA5_MIN_WG) void attn_hd64_prefix_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                                  int prefix_len, int nh, int nkv, int max_qblocks, int n_pairs,
                                                                  const u16* __restrict__ q_rows_last) {
  attn_hd64_body<LASTQ, true, false>(qkv, out, cu, prefix_len, nh, nkv, max_qblocks, n_pairs, nullptr, q_rows_last);
}

// cu / cu_host: segment starts [S + 1]; prefix_len = P > 0: segment 0 is the shared prefix the other segments continue
int lr_launch_attention_hd64_prefix(const LrAttnArgs& a, hipStream_t st) {
  const int S = a.S, n_tok = a.n_tok, nh = a.nh, nkv = a.nkv, hd = a.hd, P = a.prefix_len;
  if (n_tok <= 0 || S <= 0) return LR_OK;
  if (hd != FA5_HD) LR_FAIL(LR_EUNSUPPORTED, "attention variants 5 and 6 need head_dim 64 (got %d)", hd);
  if (nh < 1 || nkv < 1 || nh % nkv != 0)
    LR_FAIL(LR_EINVAL, "attention: num_heads %d not a multiple of num_kv_heads %d", nh, nkv);
  if (a.lse) LR_FAIL(LR_EINVAL, "attention: the head_dim-64 MFMA kernel writes no lse with a shared prefix");
  LR_RUN(lr_check_prefix_layout("attention (head_dim 64)", a.cu_host, S, n_tok, (nh + 2 * nkv) * hd, P));
  const LrAttnPlan pl = lr_attn_plan(a.cu_host, S, P, nh, hd, FA5_QROWS, nh);
  LrProfScope prof(LR_PROF_ATTN_MFMA, pl.work, st);
  LR_RUN(lr_attn_check_grid(pl));
  static bool lds_set[LR_MAX_DEVICES] = {};
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_hd64_prefix_kernel<false>), FA5_LDS_BYTES, lds_set)) return rc;
  hipLaunchKernelGGL(attn_hd64_prefix_kernel<false>, dim3((unsigned)pl.grid), dim3(256), FA5_LDS_BYTES, st, a.qkv, a.out, a.cu, P,
                     nh, nkv, pl.mq, (int)pl.n_pairs, (const u16*)nullptr);
  LR_CHECK_LAUNCH("attn_hd64_prefix_kernel");
  return LR_OK;
}

// The pruned last layer at head_dim 64 (lr_launch_attention_last): kv = [n_tok][2 nkv hd], q_last / out_last = [prompts][nh hd]
int lr_launch_attention_hd64_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu, const int32_t* cu_host,
                                  int S, int n_tok, int nh, int nkv, int prefix_len, hipStream_t st) {
  LR_RUN(lr_check_prefix_layout("attention (last rows, head_dim 64)", cu_host, S, n_tok, 2 * nkv * FA5_HD, prefix_len));
  const LrAttnPlan pl = lr_attn_plan_last(cu_host, S, prefix_len, nh, FA5_HD, 1);
  LrProfScope prof(LR_PROF_ATTN_MFMA, pl.work, st);
  LR_RUN(lr_attn_check_grid(pl));
  static bool lds_set[LR_MAX_DEVICES] = {};
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_hd64_prefix_kernel<true>), FA5_LDS_BYTES, lds_set)) return rc;
  hipLaunchKernelGGL(attn_hd64_prefix_kernel<true>, dim3((unsigned)pl.grid), dim3(256), FA5_LDS_BYTES, st, kv, out_last, cu,
                     prefix_len, nh, nkv, 0, (int)pl.n_pairs, q_last);
  LR_CHECK_LAUNCH("attn_hd64_prefix_kernel<last>");
  return LR_OK;
}
