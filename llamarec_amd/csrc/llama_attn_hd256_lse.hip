// llama_attn_hd256_lse.hip -- the training forward of attention variant 9: llama_attn_hd256.hip's kernel text instantiated with
// the log-sum-exp store (natural log of the scaled scores' sum, fp32 [token][head], read by llama_attn_bwd_hd256.hip): per row
// and head one store of (m + log2 l) ln 2, m the deferred reference and l the ones-MFMA row sum, by quad 0 of the row's lanes.
// `out` has variant 4's bits. A translation unit and a kernel name of its own: llama_attn_hd256.hip keeps its kernels as they are.
#include "llama_attn_hd256_body.h"

__global__ __launch_bounds__(512, 1) void attn_hd256_lse_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu, int nh,
                                                                int nkv, int max_qblocks, int n_pairs, float* lse) {
  attn_hd256_body<1, false, false, false, true>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, nullptr, 0.f, 0.f, lse);
}

int lr_launch_attention_hd256_lse(const LrAttnArgs& a, hipStream_t st) {
  return lr_attn_launch_tiles<attn_hd256_lse_kernel, FA4_HD, FA4_QR, 512, FA4_LDS_BYTES, false>(
      "attn_hd256_lse_kernel", "attention variants 4 and 9 need head_dim 256", nullptr, nullptr, nullptr, a, st, a.lse);
}
