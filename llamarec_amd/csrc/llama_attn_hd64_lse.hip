// llama_attn_hd64_lse.hip -- the training forward of attention variant 6: llama_attn_hd64.hip's kernel instantiated with the
// log-sum-exp store (natural log of the scaled scores' sum, fp32 [token][head], read by llama_attn_bwd_hd64.hip). A translation
// unit of its own: llama_attn_hd64.hip keeps exactly one kernel, variant 5's.
#include "llama_attn_hd64_body.h"

// the launch geometry is lr_launch_attention_hd64's, which validated the shapes
int lr_launch_attention_hd64_lse(const LrAttnArgs& a, unsigned grid, int max_qblocks, int n_pairs, hipStream_t st) {
  static bool lds_set[LR_MAX_DEVICES] = {};
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_hd64_kernel<true>), FA5_LDS_BYTES, lds_set)) return rc;
  hipLaunchKernelGGL(attn_hd64_kernel<true>, dim3(grid), dim3(256), FA5_LDS_BYTES, st, a.qkv, a.out, a.cu, a.nh, a.nkv, max_qblocks,
                     n_pairs, a.lse);
  LR_CHECK_LAUNCH("attn_hd64_kernel<lse>");
  return LR_OK;
}
