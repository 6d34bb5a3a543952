// llama_attn_bwd_hd256.hip -- attention variant 9's backward: the two passes of lr_attn_bwd_body.h (described there, with
// their rounding points) at head_dim 256 (LoRA fine-tuning of a Llama-format model of Gemma's head size). This file holds
// their geometry.
//  attn_bwd_hd256_dq_kernel  : a wave owns 16 of the workgroup's 128 query rows (8 waves, the forward's tile); K and V tiles of
//                 32 KiB, rows of 512 B; S^T = K Q^T over 8 k-steps, dQ^T += K^T dS^T over 16 d-tiles. dP^T is formed one
//                 16-key tile at a time and turned into dS^T at once, as in variant 8.
//  attn_bwd_hd256_dkv_kernel : 4 waves of 16 keys, one per SIMD (see the budget); scale = 1/16.
//
// LDS layout. Every tile here is read both row-wise (ds_read_b128) and transposed (ds_read_b64_tr_b16), so one swizzle has to
// serve both; the forward's two (K: c ^ (r & 15), V: fa4_vswz) each serve one kind. Rows are stored back to back at 512 B = 32
// chunks of 16 B = two bank rows of 256 B, so every row starts at bank 0 and chunk position p of any row sits on the 16-byte
// slot p mod 16: the swizzle alone spreads rows over the banks. Chunk c of row r sits at position c ^ ab9_swz(r),
//     ab9_swz(r) = 2 g(r) | r3,   g(r) = (r & 7) ^ 4 r3,   r3 = (r >> 3) & 1          (bits 0-3 of the chunk index only: a
// chunk stays in its 256-byte half of the row, and sub-tiles 16 rows apart have the same swizzle). Derivation from the bank
// rule (bank = (byte / 4) mod 64 for both instructions; lane groups as measured on this card):
//  transposed: ds_read_b64_tr_b16 is served in two 32-lane halves; lane (li, quad) takes 8 bytes of row 4 quad + (li >> 2)
//    at chunk 2 dt + ((li & 3) >> 1), so a half takes chunks 2 dt, 2 dt + 1 (32 B) of the 8 rows 8 m .. 8 m + 7. The 32-byte
//    slot of a row is bits 1-3 of its position: (dt ^ g(r)) & 7. g is a bijection of r & 7 on each aligned group of 8 rows, so
//    the 8 rows take the 8 slots = all 64 banks once. Bit 0 of the swizzle (r3) swaps the two 16-byte halves inside a row's
//    slot; each lane addresses its own 8 bytes through the same formula, so the read does not care. (Under c ^ (r & 15) rows r
//    and r ^ 1 share a slot: 2-way; under fa4_vswz rows r and r + 4 do.)
//  row-wise: ds_read_b128 is served in four 16-lane groups that are not the quads: a group holds rows {0-3, 12-15} at the
//    chunk of quad q and rows {4-11} at the chunk of quad q ^ 1 (same k-step). The slot is bits 0-3 of c ^ ab9_swz(r). Over
//    rows {0-3, 12-15} ab9_swz takes {0, 2, 4, 6} and {1, 3, 5, 7}: the eight values with bit 3 clear; over rows {4-11} it takes
//    {8, 10, 12, 14} and {9, 11, 13, 15}: the eight with bit 3 set, and that set is closed under ^ 1. XOR with the group's
//    chunk bits keeps the two sets on opposite values of bit 3 and distinct inside: 16 lanes on 16 slots. (The same holds if a
//    group were simply 16 rows at one chunk, since ab9_swz is a bijection of r & 15.)
// Staging: a tile is 32 lane-linear DMA pieces of 1 KiB = 2 rows; lane l of a piece writes position l & 31 of row l >> 5 and
// reads the SOURCE chunk (l & 31) ^ ab9_swz(row). The counters for both passes are in DESIGN.md section 9.
//
// Budget. dQ pass per lane: Q^T 32 + dO^T 32 + dQ^T 64 + S^T 16 + dP^T 4 (per 16-key tile) + dS 8
// registers and 12 read addresses: under the 256 of two waves per SIMD (8 waves, 512 threads, the forward's occupancy). dK/dV
// pass per lane: K 32 + V 32 + dK^T 64 + dV^T 64 + S 16 + dP 16 + P / dS 16 = 240 before any fragment or address: it runs 4
// waves, one per SIMD, on the 512-register budget. LDS: two stages of two 32 KiB tiles = 128 KiB (dK/dV: + 1 KiB of row
// statistics) of the CU's 160: one workgroup per CU in both passes, the forward's situation.
#include "llama_attn_hd256_body.h"
#include "lr_attn_bwd_body.h"

__device__ __forceinline__ int ab9_swz(int row) {
  const int r3 = (row >> 3) & 1;
  return ((((row & 7) ^ (r3 << 2)) << 1) | r3);
}

struct AttnBwdHd256 {
  static constexpr int HD = FA4_HD;
  static constexpr int KB = FA4_KB;                      // keys (dQ pass) / queries (dK/dV pass) per streamed block
  static constexpr int KSTEPS = HD / 32;                 // 8 k-steps of 32 dims in S and dP
  static constexpr int DT = HD / 16;                     // 16 d-tiles of 16 in dQ, dK and dV
  static constexpr int ROW_BYTES = FA4_ROW_BYTES;        // 512 B = 32 chunks of 16 B
  static constexpr int TILE_BYTES = FA4_TILE_BYTES;      // 32 KiB = 32 DMA pieces of 1 KiB
  static constexpr int STAGE_BYTES = FA4_STAGE_BYTES;    // two tiles
  static constexpr int QROWS = 128;                      // query rows per workgroup in the dQ pass: 8 waves of 16
  static constexpr int DQ_WAVES = 8, DQ_QT = 1;
  static constexpr int DQ_PIECES = 4;                    // per wave and tile in the dQ pass: rows 8 w .. 8 w + 7
  static constexpr int DKV_WAVES = 4;
  static constexpr int DKV_PIECES = 8;                   // per wave and tile in the dK/dV pass: rows 16 w .. 16 w + 15
  static constexpr int DQ_MIN_WG = 1, DKV_MIN_WG = 1;
  static constexpr bool DPT_WHOLE = false;
  static constexpr float SCALE = 0.0625f;                // 1 / sqrt(256)
  static constexpr int NROW = 4, NTR = 8;

  // The lane's source byte offsets of its NP DMA pieces inside a 64-row block whose rows are `stride` elements apart: piece i
  // of wave w is rows 2 (NP w + i), 2 (NP w + i) + 1; the swizzle is applied to the SOURCE chunk.
  template <int NP>
  static __device__ __forceinline__ void piece_offsets(int wave, int lane, int stride, unsigned (&off)[NP]) {
    const int prow = lane >> 5, ppos = lane & 31;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (wave * NP + i) * 2 + prow;
      off[i] = (unsigned)(row * stride + (ppos ^ ab9_swz(row)) * 8) * 2u;
    }
  }
  // the dK/dV pass's two tiles: rows `stride` (Q) and `ostride` (dO) elements apart
  static __device__ __forceinline__ void piece_offsets2(int wave, int lane, int stride, int ostride,
                                                        unsigned (&qoff)[DKV_PIECES], unsigned (&ooff)[DKV_PIECES]) {
    piece_offsets<DKV_PIECES>(wave, lane, stride, qoff);
    piece_offsets<DKV_PIECES>(wave, lane, ostride, ooff);
  }
  // Row reads: row 16 t + li, chunk 4 ks + quad. The swizzle touches chunk bits 0-3, so the four k-steps of a 256-byte half
  // are four addresses; k-steps 4-7 are the same + 256 B, sub-tiles differ by 16 rows (immediates).
  static __device__ __forceinline__ void row_offsets(int quad, int li, int (&off)[NROW]) {
#pragma unroll
    for (int ks = 0; ks < NROW; ++ks) off[ks] = li * ROW_BYTES + (((ks * 4 + quad) ^ ab9_swz(li)) << 4);
  }
  static __device__ __forceinline__ int row_addr(const int (&off)[NROW], int ks) { return (ks >> 2) * 256 + off[ks & 3]; }
  static __device__ __forceinline__ int row_addr(const int (&off)[NROW], int base, int ks) { return base + (ks >> 2) * 256 + off[ks & 3]; }
  // A operand = X^T fragment of a row-major LDS tile X[row][d] for the 16-dim tile dt and the 32-row step ks2 (fa_read_vt):
  // element e < 4: row 32 ks2 + 4 quad + e, e >= 4: the same + 16; M index (lane & 15) = dim 16 dt + li. The lane's address
  // for d-tile dt is tr_off[dt & 7] + 256 (dt >> 3): chunk 2 dt + ((li & 3) >> 1) with bits 0-3 swizzled by the row.
  static __device__ __forceinline__ void tr_offsets(int quad, int li, int (&off)[NTR]) {
    const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
    for (int d = 0; d < NTR; ++d) off[d] = ROW_BYTES * row + 16 * ((d * 2 + (p4 >> 1)) ^ ab9_swz(row)) + 8 * (p4 & 1);
  }
  static __device__ __forceinline__ int tr_addr(const int (&off)[NTR], int dt) { return (dt >> 3) * 256 + off[dt & 7]; }
  static __device__ __forceinline__ int tr_addr(const int (&off)[NTR], int base, int dt) { return base + (dt >> 3) * 256 + off[dt & 7]; }
};

__global__ __launch_bounds__(64 * AttnBwdHd256::DQ_WAVES, AttnBwdHd256::DQ_MIN_WG) void attn_bwd_hd256_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, int max_qblocks,
    const float* __restrict__ rope_cs) {
  using G = AttnBwdHd256;
#include "lr_attn_bwd_dq_body.h"
}

__global__ __launch_bounds__(64 * AttnBwdHd256::DKV_WAVES, AttnBwdHd256::DKV_MIN_WG) void attn_bwd_hd256_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, const float* __restrict__ rope_cs) {
  using G = AttnBwdHd256;
#include "lr_attn_bwd_dkv_body.h"
}

int lr_launch_attention_bwd_hd256(const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv,
                                  const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd,
                                  hipStream_t st, const float* rope_cs) {
  return lr_attn_bwd_launch<AttnBwdHd256, attn_bwd_hd256_dq_kernel, attn_bwd_hd256_dkv_kernel, 9>(
      "attn_bwd_hd256_dq_kernel", "attn_bwd_hd256_dkv_kernel", qkv, d_out, lse, dsum, dqkv, cu, cu_host, B, n_tok, nh, nkv, hd,
      st, rope_cs);
}
