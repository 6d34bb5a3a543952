// llama_attn_hd96_lse.hip -- the training forward of attention variant 8: llama_attn_hd96.hip's kernel text instantiated with the
// log-sum-exp store (natural log of the scaled scores' sum, fp32 [token][head], read by llama_attn_bwd_hd96.hip): per row and
// head one store of (m + log2 l) ln 2, m the deferred reference and l the ones-MFMA row sum, by quad 0 of the row's lanes.
// `out` has variant 7's bits. A translation unit and a kernel name of its own: llama_attn_hd96.hip keeps exactly one kernel.
#include "llama_attn_hd96_body.h"

__global__ __launch_bounds__(256, FA7_MIN_WG) void attn_hd96_lse_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                               int nh, int nkv, int max_qblocks, int n_pairs, float* lse) {
  attn_hd96_body<false, false, true>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, lse, nullptr);
}

int lr_launch_attention_hd96_lse(const LrAttnArgs& a, hipStream_t st) {
  return lr_attn_launch_tiles<attn_hd96_lse_kernel, FA7_HD, FA7_QROWS, 256, FA7_LDS_BYTES, false>(
      "attn_hd96_lse_kernel", "attention variants 7 and 8 need head_dim 96", nullptr, nullptr, nullptr, a, st, a.lse);
}
