// llama_attn_hd64_lse.hip -- the training forward of attention variant 6: llama_attn_hd64.hip's kernel instantiated with the
// log-sum-exp store (natural log of the scaled scores' sum, fp32 [token][head], read by llama_attn_bwd_hd64.hip). A translation
// unit of its own: llama_attn_hd64.hip keeps exactly one kernel, variant 5's.
#include "llama_attn_hd64_body.h"

int lr_launch_attention_hd64_lse(const LrAttnArgs& a, hipStream_t st) {
  return lr_attn_launch_tiles<attn_hd64_kernel<true>, FA5_HD, FA5_QROWS, 256, FA5_LDS_BYTES, false>(
      "attn_hd64_kernel<lse>", "attention variants 5 and 6 need head_dim 64", nullptr, nullptr, nullptr, a, st, a.lse);
}
