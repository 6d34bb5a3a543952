// lr_attn_bwd_body.h -- the LoRA step's MFMA attention backward at head_dim 64, 96 and 256 (attention variants 6, 8 and 9:
// llama_attn_bwd_hd64.hip, llama_attn_bwd_hd96.hip, llama_attn_bwd_hd256.hip), once: what the two passes share, and their
// launcher. The text of the passes is lr_attn_bwd_dq_body.h and lr_attn_bwd_dkv_body.h. On v_mfma_f32_16x16x32_bf16, no
// atomics, one writer per element of dqkv.
//
// With P = exp(S - lse), D = rowsum(dO .* O) (lr_launch_rowdot):
//     dV = P^T dO,   dP = dO V^T,   dS = P .* (dP - D),   dQ = scale dS K,   dK = scale dS^T Q.
//  dQ pass      : a workgroup owns 128 query rows of one (prompt, head), a wave 16 DQ_QT of them; 64-key K and V tiles
//                 stream through LDS (LDS-DMA, two stages). Everything transposed: S^T = K Q^T and dP^T = V dO^T put a query
//                 row in a lane's accumulator column, so lse and D are one scalar per lane, and dS^T is, as it stands in the
//                 accumulators, the B operand of dQ^T += K^T dS^T (K^T through ds_read_b64_tr_b16 from the row-major tile).
//                 dP^T is formed whole, or (DPT_WHOLE false) one 16-key tile at a time and turned into dS^T at once: 4 DQ_QT
//                 registers live instead of 16 DQ_QT.
//  dK / dV pass : a workgroup owns 64 keys of one kv head, a wave 16 of them; it walks the query heads of its group
//                 and, for each, the 64-query blocks at or after its keys (Q and dO tiles by LDS-DMA, two stages; the block's
//                 lse / D through LDS): S = Q K^T, dP = dO V^T put a key in the accumulator column; P and dS are the B operands
//                 of dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T through transposed LDS reads).
// Rounding points are those of the head_dim-128 passes (llama_attn_bwd.hip): fp32 scores, P = exp2(fma(s, scale log2 e,
// -lse log2 e)) in fp32 with the scale literal of the geometry, P and dS rounded to bf16 before the second product, fp32
// accumulation, one bf16 rounding of the result; the inverse rotation (rope_cs given) acts on the fp32 accumulators. A prompt's
// gradient rows depend on that prompt only: tiles are aligned to positions inside the prompt, rows past its end are
// range-checked to zero by the tile's buffer descriptor, masked in P and never stored.
//
// A geometry G (a struct of constants and forced-inline static functions in each unit) holds what differs per head size, all
// of it known at compile time; nothing in the passes branches on the head size at run time:
//   HD, KB (rows per streamed block), KSTEPS = HD / 32, DT = HD / 16, ROW_BYTES, TILE_BYTES, STAGE_BYTES, QROWS, and SCALE,
//     the softmax scale as a literal;
//   the LDS swizzle (chunk c of row r at position c ^ swz(r), derived in the unit for both kinds of read) and the address
//     forms on it: row_offsets / row_addr for ds_read_b128 of row 16 t + li at chunk 4 ks + quad, tr_offsets / tr_addr for
//     the transposed read of d-tile dt; NROW and NTR addresses a lane keeps, the rest immediates. row_addr(off, ks) is the
//     lane's offset inside a 16-row sub-tile, row_addr(off, base, ks) that offset added to `base` in the order the unit
//     always added it (the dQ pass uses the first, the dK/dV pass the second: hipcc's instruction order follows it);
//   piece_offsets<NP> (and piece_offsets2 for the dK/dV pass's two tiles): which row and position lane l of piece i of wave w
//     moves by LDS-DMA; DQ_PIECES and DKV_PIECES per wave;
//   the work shape: DQ_WAVES, DKV_WAVES, DQ_QT (16-row query tiles per wave in the dQ pass), the workgroups per CU each kernel
//     is held to (DQ_MIN_WG, DKV_MIN_WG), and DPT_WHOLE.
// A unit's two __global__ kernels name their geometry (`using G = ...;`) and #include the pass's text as their body. The
// text is not a forced-inline template function called from the kernel, because hipcc simplifies a callee on its own before
// it inlines it and then simplifies the kernel again: with such bodies all six kernels came out with other instruction
// streams and attn_bwd_hd256_dkv_kernel with 254 + 132 registers instead of 163 + 148 and 96 more accumulator copies. As
// included text both head_dim-96 kernels and attn_bwd_hd256_dkv_kernel are, instruction for instruction, what they were when
// each unit held its own copy; attn_bwd_hd256_dq_kernel and the two head_dim-64 kernels keep their descriptors and their
// counts of every kind of instruction that matters and differ in the order of their prologues (head_dim 64 computed its
// offsets in the kernel, not through geometry functions; a loop over one query tile lets hipcc hoist the statistics' loads
// above the fragments'). profiles/attn_bwd_shared_code_objects.txt has all of it, with the timings of those three.
#ifndef LR_ATTN_BWD_BODY_H
#define LR_ATTN_BWD_BODY_H

#include "llama_train.h"
#include "lr_attn_body.h"

typedef u16 u16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;

#define AB_LOG2E 1.4426950408889634f
#define AB_DMA_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// Optional epilogue: gradient w.r.t. the UNROTATED q / k. A lane holds dims 16 dt + 4 quad + 0..3 = rotation pairs
// i0 = 8 dt + 2 quad and i0 + 1 of its row (packed layout: pair (x1_i, x2_i) adjacent); HD / 2 pairs per position, so the two
// pairs are one aligned float4 of the table.
template <int HD>
__device__ __forceinline__ void attn_bwd_unrotate(float (&v)[4], const float* rope_cs, int pos, int dt, int quad) {
  if (!rope_cs) return;
  const float4 cs = *reinterpret_cast<const float4*>(rope_cs + ((size_t)pos * (HD / 2) + dt * 8 + 2 * quad) * 2);
  const float a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
  v[0] = a0 * cs.x + a1 * cs.y;
  v[1] = a1 * cs.x - a0 * cs.y;
  v[2] = b0 * cs.z + b1 * cs.w;
  v[3] = b1 * cs.z - b0 * cs.w;
}

// ---- the launch sequence of variants 6, 8 and 9, once --------------------------------------------------------------------
// dsum = rowsum(dO .* O) is already in place (lr_launch_attention_bwd); cu / cu_host: prompt starts [B + 1] in packed rows.
// The kernels are template arguments: the dynamic-LDS flags are per kernel.
template <class G, auto DQ_KERNEL, auto DKV_KERNEL, int VARIANT>
static inline int lr_attn_bwd_launch(const char* dq_name, const char* dkv_name, const u16* qkv, const u16* d_out,
                                     const float* lse, const float* dsum, u16* dqkv, const int32_t* cu, const int32_t* cu_host,
                                     int B, int n_tok, int nh, int nkv, int hd, hipStream_t st, const float* rope_cs) {
  if (hd != G::HD) LR_FAIL(LR_EUNSUPPORTED, "attention backward variant %d needs head_dim %d (got %d)", VARIANT, G::HD, hd);
  int maxT = 0;
  for (int b = 0; b < B; ++b) maxT = max(maxT, cu_host[b + 1] - cu_host[b]);
  // the tiles come through buffer descriptors (32-bit byte offsets from a tile's first element)
  if ((long long)n_tok * (nh + 2 * nkv) * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward: packed qkv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  const int mq = (maxT + G::QROWS - 1) / G::QROWS, mk = (maxT + G::KB - 1) / G::KB;
  if (mq == 0) return LR_OK;
  if (nh > 65535 || nkv > 65535 || B > 65535)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward variant %d: %d heads / %d prompts exceed the grid limit", VARIANT, nh, B);
  static bool lds_set_dq[LR_MAX_DEVICES] = {}, lds_set_dkv[LR_MAX_DEVICES] = {};
  const int dkv_lds = 2 * G::STAGE_BYTES + 2 * 128 * (int)sizeof(float);
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(DQ_KERNEL), 2 * G::STAGE_BYTES, lds_set_dq)) return rc;
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(DKV_KERNEL), dkv_lds, lds_set_dkv)) return rc;
  hipLaunchKernelGGL(DQ_KERNEL, dim3(mq, nh, B), dim3(64 * G::DQ_WAVES), 2 * G::STAGE_BYTES, st, qkv, d_out, lse, dsum, dqkv,
                     cu, nh, nkv, mq, rope_cs);
  LR_CHECK_LAUNCH(dq_name);
  hipLaunchKernelGGL(DKV_KERNEL, dim3(mk, nkv, B), dim3(64 * G::DKV_WAVES), dkv_lds, st, qkv, d_out, lse, dsum, dqkv, cu, nh,
                     nkv, rope_cs);
  LR_CHECK_LAUNCH(dkv_name);
  return LR_OK;
}

#endif
