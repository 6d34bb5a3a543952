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
  attn_hd96_body<LASTQ, true, false>(qkv, out, cu, prefix_len, nh, nkv, max_qblocks, n_pairs, nullptr, q_rows_last);
}

// cu / cu_host: segment starts [S + 1]; prefix_len = P > 0: segment 0 is the shared prefix the other segments continue
int lr_launch_attention_hd96_prefix(const LrAttnArgs& a, hipStream_t st) {
  return lr_attn_launch_tiles<attn_hd96_prefix_kernel<false>, FA7_HD, FA7_QROWS, 256, FA7_LDS_BYTES, true>(
      "attn_hd96_prefix_kernel", "attention variant 7 needs head_dim 96", "attention: the head_dim-96 MFMA kernel writes no lse",
      nullptr, "attention (head_dim 96)", a, st, (const u16*)nullptr);
}

int lr_launch_attention_hd96_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu, const int32_t* cu_host,
                                  int S, int n_tok, int nh, int nkv, int prefix_len, hipStream_t st) {
  return lr_attn_launch_last<attn_hd96_prefix_kernel<true>, FA7_HD, 256, FA7_LDS_BYTES>(
      "attn_hd96_prefix_kernel<last>", "attention (last rows, head_dim 96)", kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv,
      prefix_len, st);
}
