// llama_attn_hd96_prefix.hip -- the head_dim-96 MFMA attention (variant 7; its text is attn_hd96_body in
// llama_attn_hd96_body.h: read it first) instantiated in its two other modes, as kernels of their own in a translation unit
// of their own, so that variant 7's code object holds variant 7 alone:
//
//   attn_hd96_prefix_kernel<false>  shared prompt prefix (prefix_len = P > 0): the body's PREFIX mode
//   attn_hd96_prefix_kernel<true>   the pruned last layer, one query row per prompt: the body's LASTQ mode
//
// Contract: a row's bits are those variant 7 writes for the same row of the same whole prompt. It holds because the block walk
// and the softmax are the same lines of the body in every mode; only the home of a staged K / V row differs, and the LDS image
// of a block is the same bytes either way (rows past the prompt's end are zero in both: the buffer descriptor's range check).
// The hand-placed `s_waitcnt vmcnt(0)` in front of every barrier covers both staging forms (the DMA is inline asm).
#include "llama_attn_hd96_body.h"

template <bool LASTQ>
__global__ __launch_bounds__(256, FA7_MIN_WG) void attn_hd96_prefix_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                                  int prefix_len, int nh, int nkv, int max_qblocks, int n_pairs,
                                                                  const u16* __restrict__ q_rows_last) {
  attn_hd96_body<LASTQ, true>(qkv, out, cu, prefix_len, nh, nkv, max_qblocks, n_pairs, q_rows_last);
}

// cu / cu_host: segment starts [S + 1]; prefix_len = P > 0: segment 0 is the shared prefix the other segments continue
int lr_launch_attention_hd96_prefix(const LrAttnArgs& a, hipStream_t st) {
  const int S = a.S, n_tok = a.n_tok, nh = a.nh, nkv = a.nkv, hd = a.hd, P = a.prefix_len;
  if (n_tok <= 0 || S <= 0) return LR_OK;
  if (hd != FA7_HD) LR_FAIL(LR_EUNSUPPORTED, "attention variant 7 needs head_dim 96 (got %d)", hd);
  if (nh < 1 || nkv < 1 || nh % nkv != 0)
    LR_FAIL(LR_EINVAL, "attention: num_heads %d not a multiple of num_kv_heads %d", nh, nkv);
  if (a.lse) LR_FAIL(LR_EINVAL, "attention: the head_dim-96 MFMA kernel writes no lse");
  LR_RUN(lr_check_prefix_layout("attention (head_dim 96)", a.cu_host, S, n_tok, (nh + 2 * nkv) * hd, P));
  const LrAttnPlan pl = lr_attn_plan(a.cu_host, S, P, nh, hd, FA7_QROWS, nh);
  LrProfScope prof(LR_PROF_ATTN_MFMA, pl.work, st);
  LR_RUN(lr_attn_check_grid(pl));
  static bool lds_set[LR_MAX_DEVICES] = {};
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_hd96_prefix_kernel<false>), FA7_LDS_BYTES, lds_set)) return rc;
  hipLaunchKernelGGL(attn_hd96_prefix_kernel<false>, dim3((unsigned)pl.grid), dim3(256), FA7_LDS_BYTES, st, a.qkv, a.out, a.cu, P,
                     nh, nkv, pl.mq, (int)pl.n_pairs, (const u16*)nullptr);
  LR_CHECK_LAUNCH("attn_hd96_prefix_kernel");
  return LR_OK;
}

// The pruned last layer at head_dim 96 (lr_launch_attention_last): kv = [n_tok][2 nkv hd], q_last / out_last = [prompts][nh hd]
int lr_launch_attention_hd96_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu, const int32_t* cu_host,
                                  int S, int n_tok, int nh, int nkv, int prefix_len, hipStream_t st) {
  LR_RUN(lr_check_prefix_layout("attention (last rows, head_dim 96)", cu_host, S, n_tok, 2 * nkv * FA7_HD, prefix_len));
  const LrAttnPlan pl = lr_attn_plan_last(cu_host, S, prefix_len, nh, FA7_HD, 1);
  LrProfScope prof(LR_PROF_ATTN_MFMA, pl.work, st);
  LR_RUN(lr_attn_check_grid(pl));
  static bool lds_set[LR_MAX_DEVICES] = {};
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_hd96_prefix_kernel<true>), FA7_LDS_BYTES, lds_set)) return rc;
  hipLaunchKernelGGL(attn_hd96_prefix_kernel<true>, dim3((unsigned)pl.grid), dim3(256), FA7_LDS_BYTES, st, kv, out_last, cu,
                     prefix_len, nh, nkv, 0, (int)pl.n_pairs, q_last);
  LR_CHECK_LAUNCH("attn_hd96_prefix_kernel<last>");
  return LR_OK;
}
