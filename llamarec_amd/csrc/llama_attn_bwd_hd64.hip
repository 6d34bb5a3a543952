// llama_attn_bwd_hd64.hip -- attention variant 6's backward: the two passes of lr_attn_bwd_body.h (described there, with their
// rounding points) at head_dim 64 (Llama-3.2-1B / 3B LoRA fine-tuning). This file holds their geometry.
//  attn_bwd_hd64_dq_kernel  : a wave owns 32 of the workgroup's 128 query rows; K and V tiles of 8 KiB, rows of 128 B;
//                 S^T = K Q^T over 2 k-steps, dQ^T += K^T dS^T over 4 d-tiles. dP^T is formed whole.
//  attn_bwd_hd64_dkv_kernel : 4 waves of 16 keys; scale = 1/8.
// Budget: dQ pass per lane Q^T 8 + dO^T 8 + dQ^T 32 + S^T 32 + dP^T 32 + dS 8 registers; dK/dV pass
// K 8 + V 8 + dK^T 16 + dV^T 16 + S 16 + dP 16 + P / dS 8. Both are held to 128 registers: four workgroups per CU.
// LDS: two stages of two 8 KiB tiles = 32 KiB (dK/dV: + 1 KiB of row statistics), 128 / 132 KiB of the CU's 160 at four.
#include "lr_attn_bwd_body.h"

// Dual-use swizzle on the 3-bit chunk index of a 128-byte row: chunk c of row r sits at position c ^ ab6_sw(r),
// ab6_sw(r) = ((r >> 1) & 3) << 1. The 16-byte bank slot (of 16) of position p of row r is 8 (r & 1) + p.
//  Row reads (ds_read_b128: lane (li, quad) takes row 16 t + li, chunk 4 ks + quad). The LDS serves 16 lanes per cycle, and
//   not 16 consecutive ones: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32. Such a group holds rows
//   li in {0..3, 12..15} at chunk c and rows li in {4..11} at chunk c ^ 1 (or the other way round). Bit 0 of the swizzle
//   is zero, so bit 0 of the position is bit 0 of the chunk: the two sets never meet. Inside a set, rows of equal parity are
//   {0, 2, 12, 14}, {1, 3, 13, 15}, {4, 6, 8, 10} or {5, 7, 9, 11}: (r >> 1) & 3 takes 0, 1, 2, 3 once in each, so the four
//   rows land on four different positions of their parity's half: all 16 slots, no conflict.
//  Transposed reads (ds_read_b64_tr_b16: 32 lanes per cycle, lane (li, quad) takes 8 bytes of row 4 quad + (li >> 2),
//   chunk 2 dt + ((li & 3) >> 1)). A 32-lane half holds 8 consecutive rows x 32 B, the chunk pair (2 dt, 2 dt + 1); the
//   32-byte slot (of 8) is 4 (r & 1) + ((2 dt ^ sw) >> 1) = 4 (r & 1) + (dt ^ ((r >> 1) & 3)): the four rows of equal parity
//   take four different pairs. The pair itself stays in order (bit 0 untouched).
//  It depends on row bits 1..2 only: sub-tiles 8, 16, 32 rows apart differ by an immediate offset.
// Derived from the bank rules of the microarchitecture notes; NOT confirmed with the LDS bank-conflict counter.
__device__ __forceinline__ int ab6_sw(int row) { return ((row >> 1) & 3) << 1; }

struct AttnBwdHd64 {
  static constexpr int HD = 64;
  static constexpr int KB = 64;                          // keys (dQ pass) / queries (dK/dV pass) per streamed block
  static constexpr int KSTEPS = HD / 32, DT = HD / 16;
  static constexpr int ROW_BYTES = HD * 2;               // 128 B = 8 chunks of 16 B; two rows span the 64 banks
  static constexpr int TILE_BYTES = KB * ROW_BYTES;      // 8 KiB
  static constexpr int STAGE_BYTES = 2 * TILE_BYTES;
  static constexpr int QROWS = 128;                      // query rows per workgroup in the dQ pass
  static constexpr int DQ_WAVES = 4, DQ_QT = 2, DKV_WAVES = 4;
  static constexpr int DQ_PIECES = 2, DKV_PIECES = 2;    // per wave and tile: pieces 2w, 2w + 1
  static constexpr int DQ_MIN_WG = 4;                    // workgroups per CU the dQ pass's registers are held to (<= 128)
  static constexpr int DKV_MIN_WG = 4;                   // ... and the dK/dV pass's (<= 128)
  static constexpr bool DPT_WHOLE = true;
  static constexpr float SCALE = 0.125f;                 // 1 / sqrt(64)
  static constexpr int NROW = 2, NTR = 4;

  // A tile is 8 pieces of 1 KiB (8 rows x 128 B, lane-linear in LDS); wave w moves pieces 2w, 2w + 1. The swizzle is applied
  // to the SOURCE chunk.
  template <int NP>
  static __device__ __forceinline__ void piece_offsets(int wave, int lane, int stride, unsigned (&off)[NP]) {
    const int prow = lane >> 3, ppos = lane & 7;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (wave * NP + i) * 8 + prow;
      off[i] = (unsigned)(row * stride + (ppos ^ ab6_sw(row)) * 8) * 2u;
    }
  }
  // the dK/dV pass's two tiles: rows `stride` (Q) and `ostride` (dO) elements apart, both in one loop as this unit always did
  static __device__ __forceinline__ void piece_offsets2(int wave, int lane, int stride, int ostride,
                                                        unsigned (&qoff)[DKV_PIECES], unsigned (&ooff)[DKV_PIECES]) {
    const int prow = lane >> 3, ppos = lane & 7;
#pragma unroll
    for (int i = 0; i < DKV_PIECES; ++i) {
      const int row = (wave * DKV_PIECES + i) * 8 + prow;
      qoff[i] = (unsigned)(row * stride + (ppos ^ ab6_sw(row)) * 8) * 2u;
      ooff[i] = (unsigned)(row * ostride + (ppos ^ ab6_sw(row)) * 8) * 2u;
    }
  }
  // Row reads: row 16 nt + li, chunk 4 ks + quad: one address per k-step.
  static __device__ __forceinline__ void row_offsets(int quad, int li, int (&off)[NROW]) {
#pragma unroll
    for (int ks = 0; ks < NROW; ++ks) off[ks] = li * ROW_BYTES + (((ks * 4 + quad) ^ ab6_sw(li)) << 4);
  }
  static __device__ __forceinline__ int row_addr(const int (&off)[NROW], int ks) { return off[ks]; }
  static __device__ __forceinline__ int row_addr(const int (&off)[NROW], int base, int ks) { return base + off[ks]; }
  // A operand = X^T fragment of a row-major LDS tile X[row][d] for the 16-dim tile dt and the 32-row step ks2 (fa_read_vt):
  // element e < 4: row 32 ks2 + 4 quad + e, e >= 4: row 32 ks2 + 16 + 4 quad + (e - 4); M index (lane & 15) = dim 16 dt + li.
  // One address per d-tile; rows 16 apart share the swizzle.
  static __device__ __forceinline__ void tr_offsets(int quad, int li, int (&off)[NTR]) {
    const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
    for (int dt = 0; dt < NTR; ++dt) off[dt] = ROW_BYTES * row + 16 * ((dt * 2 + (p4 >> 1)) ^ ab6_sw(row)) + 8 * (p4 & 1);
  }
  static __device__ __forceinline__ int tr_addr(const int (&off)[NTR], int dt) { return off[dt]; }
  static __device__ __forceinline__ int tr_addr(const int (&off)[NTR], int base, int dt) { return base + off[dt]; }
};

__global__ __launch_bounds__(64 * AttnBwdHd64::DQ_WAVES, AttnBwdHd64::DQ_MIN_WG) void attn_bwd_hd64_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, int max_qblocks,
    const float* __restrict__ rope_cs) {
  using G = AttnBwdHd64;
#include "lr_attn_bwd_dq_body.h"
}

__global__ __launch_bounds__(64 * AttnBwdHd64::DKV_WAVES, AttnBwdHd64::DKV_MIN_WG) void attn_bwd_hd64_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, const float* __restrict__ rope_cs) {
  using G = AttnBwdHd64;
#include "lr_attn_bwd_dkv_body.h"
}

int lr_launch_attention_bwd_hd64(const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv,
                                 const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd,
                                 hipStream_t st, const float* rope_cs) {
  return lr_attn_bwd_launch<AttnBwdHd64, attn_bwd_hd64_dq_kernel, attn_bwd_hd64_dkv_kernel, 6>(
      "attn_bwd_hd64_dq_kernel", "attn_bwd_hd64_dkv_kernel", qkv, d_out, lse, dsum, dqkv, cu, cu_host, B, n_tok, nh, nkv, hd,
      st, rope_cs);
}
