// llama_attn_hd256.hip -- attention variant 4: varlen causal flash attention at head_dim 256 on gfx950 (Gemma-2B / 7B).
//
// Variant 2's transposed formulation (llama_attn.hip) widened to 256 dimensions:
//   S^T = K Q^T   (A = K rows from LDS, B = Q rows held in registers) -> a lane owns ONE query row (lane & 15) and
//                 16 of the block's 64 keys
//   O^T = V^T P^T (A = V read with ds_read_b64_tr_b16 from the row-major LDS tile, B = P straight from the S^T
//                 accumulators) -> O's column is again the lane's query row: the online-softmax rescale is lane-local.
// Budget. At hd 256 a wave of variant 2's shape (32 query rows) holds 128 O^T accumulators and 64 Q^T
// registers per lane before any K fragment, score or address: only one such wave fits a SIMD. Here a wave owns 16 query
// rows: O^T 64, Q^T 32, S^T 16, two K fragment sets 32, P 8, row sums 4 -> < 256 registers, two waves per SIMD. A workgroup
// = 8 waves = 128 query rows of one (prompt, head), the same causal tile as variant 2; 64-key blocks, K and V tiles of
// 64 x 512 B = 32 KiB each, double-buffered: 128 KiB of LDS, one workgroup (8 waves) per CU.
// Each K / V fragment read from LDS feeds one MFMA (two in variant 2): 1 KiB per 16x16x32 MFMA, which one CU's LDS
// (256 B/clk) serves for four SIMDs at their full MFMA rate -- the kernel is bound by the softmax and the barriers long
// before that.
// Rounding points are variant 2's: fp32 scores and online softmax with the deferred maximum (a row's reference moves only
// when a score exceeds it by more than 2^FA_DEFER), bf16 P into both the numerator and the row sum (an MFMA against a row
// of ones), one bf16 rounding of O / l. A query row's bits depend only on its own prompt: tiles and key blocks are aligned
// to positions inside the prompt, and the rescale decision is per row.
// The kernel's one text is attn_hd256_body in llama_attn_hd256_body.h, with its modes chosen at compile time. This file
// instantiates variant 4 (no shared prefix, no log-sum-exp output) and holds its launcher; with a shared prefix, and for the
// pruned last layer's one-query-row mode, lr_launch_attention runs the instantiations of llama_attn_hd256_prefix.hip (same
// bits). llama_attn_hd256_lse.hip instantiates the training forward (attention variant 9), which also writes the natural-log
// log-sum-exp per (token, head); the backward is llama_attn_bwd_hd256.hip.
#include "llama_attn_hd256_body.h"

// HPW = heads per workgroup (llama_attn_hd256_body.h): 1 is the product, selected by lr_launch_attention_hd256; 2 is an A/B arm
// (tools/diag/attn_hd256_mqa_ab.py)
template <int HPW>
__global__ __launch_bounds__(512, 1) void attn_hd256_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                            int nh, int nkv, int max_qblocks, int n_pairs) {
  attn_hd256_body<HPW, false, false>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, nullptr);
}

template <int HPW>
static int launch_hd256(const LrAttnArgs& a, hipStream_t st) {
  return lr_attn_launch_tiles<attn_hd256_kernel<HPW>, FA4_HD, FA4_QR, 512, FA4_LDS_BYTES, false, HPW>(
      "attn_hd256_kernel", "attention variant 4 needs head_dim 256", nullptr, nullptr, nullptr, a, st);
}

// cu / cu_host: prompt starts [B + 1] in packed rows (no shared prefix). a.lse reaches this launcher only where the resolver
// allowed it (variant 9, or the LoRA route's auto): lr_resolve_attention refuses variant 4 with lse.
int lr_launch_attention_hd256(const LrAttnArgs& a, hipStream_t st) {
  if (a.lse) return lr_launch_attention_hd256_lse(a, st);   // llama_attn_hd256_lse.hip
  return launch_hd256<1>(a, st);
}
