// llama_attn_hd256_prefix.hip -- the head_dim-256 MFMA attention (variant 4; its text is attn_hd256_body in
// llama_attn_hd256_body.h: read it first) instantiated in the two modes attn_mfma128_kernel has in llama_attn.hip, as kernels of
// their own in a translation unit of their own, so that variant 4's code object holds variant 4 alone:
//
//   attn_hd256_prefix_kernel<false>  shared prompt prefix (prefix_len = P > 0): the body's PREFIX mode
//   attn_hd256_prefix_kernel<true>   the pruned last layer, one query row per prompt: the body's LASTQ mode
//
// Contract: a row's bits are those variant 4 writes for the same row of the same whole prompt. It holds because the block walk
// and the softmax are the same lines of the body in every mode; only the home of a staged K / V row differs, and the LDS image
// of a block is the same bytes either way (rows past the prompt's end are zero in both: the buffer descriptor's range check).
// The hand-placed `s_waitcnt vmcnt(0)` in front of every barrier covers both staging forms (the DMA is inline asm).
#include "llama_attn_hd256_body.h"

template <bool LASTQ>
__global__ __launch_bounds__(512, 1) void attn_hd256_prefix_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                                   int prefix_len, int nh, int nkv, int max_qblocks, int n_pairs,
                                                                   const u16* __restrict__ q_rows_last) {
  attn_hd256_body<1, LASTQ, true>(qkv, out, cu, prefix_len, nh, nkv, max_qblocks, n_pairs, q_rows_last);
}

// cu / cu_host: segment starts [S + 1]; prefix_len = P > 0: segment 0 is the shared prefix the other segments continue
int lr_launch_attention_hd256_prefix(const LrAttnArgs& a, hipStream_t st) {
  return lr_attn_launch_tiles<attn_hd256_prefix_kernel<false>, FA4_HD, FA4_QR, 512, FA4_LDS_BYTES, true>(
      "attn_hd256_prefix_kernel", "attention variant 4 needs head_dim 256", "attention: the head_dim-256 MFMA kernel writes no lse",
      nullptr, "attention (head_dim 256)", a, st, (const u16*)nullptr);
}

int lr_launch_attention_hd256_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu, const int32_t* cu_host,
                                   int S, int n_tok, int nh, int nkv, int prefix_len, hipStream_t st) {
  return lr_attn_launch_last<attn_hd256_prefix_kernel<true>, FA4_HD, 512, FA4_LDS_BYTES>(
      "attn_hd256_prefix_kernel<last>", "attention (last rows, head_dim 256)", kv, q_last, out_last, cu, cu_host, S, n_tok, nh,
      nkv, prefix_len, st);
}
