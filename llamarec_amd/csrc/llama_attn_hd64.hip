// llama_attn_hd64.hip -- attention variant 5: varlen causal flash attention at head_dim 64 on gfx950 (Llama-3.2-1B).
//
// Variant 2's transposed formulation (llama_attn.hip) narrowed to 64 dimensions:
//   S^T = K Q^T   (A = K rows from LDS, B = Q rows held in registers) -> a lane owns ONE query row (lane & 15) and
//                 16 of the block's 64 keys
//   O^T = V^T P^T (A = V read with ds_read_b64_tr_b16 from the row-major LDS tile, B = P straight from the S^T
//                 accumulators) -> O's column is again the lane's query row: the online-softmax rescale is lane-local.
// Budget. A wave owns 16 FA5_QT query rows; per lane and 16-row tile: O^T 16, Q^T 8, S^T 16, P 8,
// row sums 4 registers, and two K fragment sets of 16 for the wave. A workgroup = 4 waves = 64 FA5_QT query rows of one
// (prompt, head); 64-key blocks, K and V tiles of 64 x 128 B = 8 KiB each, double-buffered: 32 KiB of LDS.
// Per 64-key block and 16-row tile a wave issues 8 + 8 + 2 MFMAs (variant 2: 16 + 16 + 2) beside the same 16 exponentials
// per lane: the softmax binds, so what counts is how many waves a SIMD holds to overlap one wave's exponentials with
// another's MFMAs.
// Rounding points are variant 2's: fp32 scores and online softmax with the deferred maximum (a row's reference moves only
// when a score exceeds it by more than 2^FA_DEFER), bf16 P into both the numerator and the row sum (an MFMA against a row
// of ones), one bf16 rounding of O / l. A query row's bits depend only on its own prompt: tiles and key blocks are aligned
// to positions inside the prompt, and the rescale decision is per row.
// The kernel's one text is attn_hd64_body in llama_attn_hd64_body.h, with its modes chosen at compile time. This file
// instantiates variant 5 (no shared prefix, no lse) and holds its launcher. llama_attn_hd64_lse.hip instantiates the training
// forward (attention variant 6), which also writes the natural-log log-sum-exp of the scaled scores per (token, head) from the
// deferred reference and the row sum, as variant 2 does. llama_attn_hd64_prefix.hip instantiates the shared-prefix mode and the
// pruned last layer's one-query-row mode. `out` has the same bits in every instantiation. The backward is
// llama_attn_bwd_hd64.hip.
#include "llama_attn_hd64_body.h"

// cu / cu_host: prompt starts [B + 1] in packed rows (no shared prefix at head_dim 64)
int lr_launch_attention_hd64(const LrAttnArgs& a, hipStream_t st) {
  if (a.lse) return lr_launch_attention_hd64_lse(a, st);   // llama_attn_hd64_lse.hip
  return lr_attn_launch_tiles<attn_hd64_kernel<false>, FA5_HD, FA5_QROWS, 256, FA5_LDS_BYTES, false>(
      "attn_hd64_kernel", "attention variants 5 and 6 need head_dim 64", nullptr, nullptr, nullptr, a, st, (float*)nullptr);
}
