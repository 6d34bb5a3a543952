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
  return lr_attn_launch_tiles<attn_hd64_prefix_kernel<false>, FA5_HD, FA5_QROWS, 256, FA5_LDS_BYTES, true>(
      "attn_hd64_prefix_kernel", "attention variants 5 and 6 need head_dim 64",
      "attention: the head_dim-64 MFMA kernel writes no lse with a shared prefix", nullptr, "attention (head_dim 64)", a, st,
      (const u16*)nullptr);
}

int lr_launch_attention_hd64_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu, const int32_t* cu_host,
                                  int S, int n_tok, int nh, int nkv, int prefix_len, hipStream_t st) {
  return lr_attn_launch_last<attn_hd64_prefix_kernel<true>, FA5_HD, 256, FA5_LDS_BYTES>(
      "attn_hd64_prefix_kernel<last>", "attention (last rows, head_dim 64)", kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv,
      prefix_len, st);
}
