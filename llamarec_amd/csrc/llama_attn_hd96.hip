// llama_attn_hd96.hip -- attention variant 7: varlen causal flash attention at head_dim 96 on gfx950 (Phi-3-mini).
//
// Variant 5's transposed formulation (llama_attn_hd64.hip) widened to 96 dimensions:
//   S^T = K Q^T   (A = K rows from LDS, B = Q rows held in registers, 3 k-steps of 32) -> a lane owns ONE query row
//                 (lane & 15) and 16 of the block's 64 keys
//   O^T = V^T P^T (A = V read with ds_read_b64_tr_b16 from the row-major LDS tile, 6 d-tiles of 16, B = P straight from the
//                 S^T accumulators) -> O's column is again the lane's query row: the online-softmax rescale is lane-local.
// Budget. A wave owns 16 FA7_QT query rows; per lane and 16-row tile: O^T 24, Q^T 12, S^T 16, P 8,
// row sums 4 registers, and one K fragment set of 16 per k-step for the wave. A workgroup = 4 waves = 64 FA7_QT query rows
// of one (prompt, head); 64-key blocks, K and V tiles of 64 x 192 B = 12 KiB each, double-buffered: 48 KiB of LDS, three
// workgroups per CU. Per 64-key block and 16-row tile a wave issues 12 + 12 + 2 MFMAs beside the same 16 exponentials per lane.
// Rounding points are variant 5's: fp32 scores and online softmax with the deferred maximum (a row's reference moves only
// when a score exceeds it by more than 2^FA_DEFER), bf16 P into both the numerator and the row sum (an MFMA against a row
// of ones), one bf16 rounding of O / l. A query row's bits depend only on its own prompt: tiles and key blocks are aligned
// to positions inside the prompt, and the rescale decision is per row.
// The kernel's one text is attn_hd96_body in llama_attn_hd96_body.h (the LDS layout and its swizzles are derived there), with
// its modes chosen at compile time. This file instantiates variant 7 (no shared prefix) and holds its launcher;
// llama_attn_hd96_prefix.hip instantiates the shared-prefix mode and the pruned last layer's one-query-row mode. `out` has
// the same bits in every instantiation. llama_attn_hd96_lse.hip instantiates the training forward (attention variant 8), which
// also writes the natural-log log-sum-exp per (token, head); the backward is llama_attn_bwd_hd96.hip.
#include "llama_attn_hd96_body.h"

__global__ __launch_bounds__(256, FA7_MIN_WG) void attn_hd96_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu, int nh,
                                                           int nkv, int max_qblocks, int n_pairs) {
  attn_hd96_body<false, false, false>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, nullptr, nullptr);
}

// cu / cu_host: prompt starts [B + 1] in packed rows (no shared prefix). a.lse reaches this launcher only where the resolver
// allowed it (variant 8, or the LoRA route's auto): lr_resolve_attention refuses variant 7 with lse.
int lr_launch_attention_hd96(const LrAttnArgs& a, hipStream_t st) {
  if (a.lse) return lr_launch_attention_hd96_lse(a, st);   // llama_attn_hd96_lse.hip
  return lr_attn_launch_tiles<attn_hd96_kernel, FA7_HD, FA7_QROWS, 256, FA7_LDS_BYTES, false>(
      "attn_hd96_kernel", "attention variants 7 and 8 need head_dim 96", nullptr, nullptr, nullptr, a, st);
}
