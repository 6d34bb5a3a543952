// llama_attn_bwd_hd96.hip -- attention variant 8's backward: the two passes of lr_attn_bwd_body.h (described there, with their
// rounding points) at head_dim 96 (LoRA fine-tuning of a Llama-format Phi-3-mini). This file holds their geometry.
//  attn_bwd_hd96_dq_kernel  : a wave owns 32 of the workgroup's 128 query rows; K and V tiles of 12 KiB, rows of 192 B;
//                 S^T = K Q^T over 3 k-steps, dQ^T += K^T dS^T over 6 d-tiles. dP^T is formed one 16-key tile at a time
//                 and turned into dS^T at once: 8 registers live instead of 32 (see the budget).
//  attn_bwd_hd96_dkv_kernel : 4 waves of 16 keys; scale = 96^-0.5 in fp32.
//
// LDS layout and staging are the head_dim-96 forward's (llama_attn_hd96_body.h, derived there and confirmed with the
// bank-conflict counter): rows back to back at a 192-byte stride, chunk c of row r at position c ^ fa7_swz(r), a tile = 12
// lane-linear DMA pieces of 1 KiB, wave w moving pieces 3w .. 3w + 2 = rows 16w .. 16w + 15. That one swizzle was derived for
// BOTH kinds of read, which is what the backward needs, since each of its tiles is read both ways:
//  K (dQ pass), Q and dO (dK/dV pass), row-wise: ds_read_b128, lane (li, quad) takes row 16 t + li at chunk 4 ks + quad, t the
//    16-row sub-tile and ks the k-step -- the forward's K read, address for address (sub-tiles and k-steps are immediates).
//  K (dQ pass), Q and dO (dK/dV pass), transposed: ds_read_b64_tr_b16, lane (li, quad) takes 8 bytes of row 4 quad + (li >> 2)
//    (+ 16, and + 32 per 32-row step) at chunk 2 dt + ((li & 3) >> 1) -- the forward's V read, address for address.
//  V (dQ pass), row-wise: the forward reads V transposed only, but stages it with K's swizzle, so this is the K read on another
//    tile base (a multiple of 12 KiB = 192 slots of 64 B: the bank of an address is unchanged).
// The derivation speaks of rows and chunks inside a tile only; which tensor the bytes came from does not enter it.
//
// Budget: dQ pass per lane Q^T 12 + dO^T 12 + dQ^T 48 + S^T 32 + dP^T 8 (per 16-key tile) + dS 16
// registers; dK/dV pass K 12 + V 12 + dK^T 24 + dV^T 24 + S 16 + dP 16 + P / dS 8. Both are held to 168 registers: three
// workgroups per CU. LDS: two stages of two 12 KiB tiles = 48 KiB (dK/dV: + 1 KiB of row statistics), 144 / 147 KiB of the
// CU's 160 at three.
#include "llama_attn_hd96_body.h"
#include "lr_attn_bwd_body.h"

struct AttnBwdHd96 {
  static constexpr int HD = FA7_HD;
  static constexpr int KB = FA7_KB;                      // keys (dQ pass) / queries (dK/dV pass) per streamed block
  static constexpr int KSTEPS = FA7_KSTEPS;              // 3 k-steps of 32 dims in S and dP
  static constexpr int DT = FA7_DT;                      // 6 d-tiles of 16 in dQ, dK and dV
  static constexpr int ROW_BYTES = FA7_ROW_BYTES;        // 192 B = 12 chunks of 16 B
  static constexpr int TILE_BYTES = FA7_TILE_BYTES;      // 12 KiB = 12 DMA pieces of 1 KiB
  static constexpr int STAGE_BYTES = FA7_STAGE_BYTES;    // two tiles
  static constexpr int QROWS = 128;                      // query rows per workgroup in the dQ pass
  static constexpr int DQ_WAVES = 4, DQ_QT = 2, DKV_WAVES = 4;
  static constexpr int DQ_PIECES = FA7_WAVE_PIECES, DKV_PIECES = FA7_WAVE_PIECES;   // per wave and tile: exactly 16 rows
  static constexpr int DQ_MIN_WG = 3, DKV_MIN_WG = 3;    // workgroups per CU both passes' registers are held to (<= 168)
  static constexpr bool DPT_WHOLE = false;
  static constexpr float SCALE = 0.10206207261596575f;   // 1 / sqrt(96)
  static constexpr int NROW = 1, NTR = 2;

  // The lane's source byte offsets of its three DMA pieces inside a 64-row block whose rows are `stride` elements apart: lane
  // l of piece i writes linear chunk 64 i + l of the wave's 192, row 16 w + (64 i + l) / 12 at position (64 i + l) % 12; the
  // swizzle is applied to the SOURCE chunk.
  template <int NP>
  static __device__ __forceinline__ void piece_offsets(int wave, int lane, int stride, unsigned (&off)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int g = i * 64 + lane, r16 = g / FA7_ROW_CHUNKS, ppos = g - r16 * FA7_ROW_CHUNKS;
      const int row = wave * 16 + r16;
      off[i] = (unsigned)(row * stride + (ppos ^ fa7_swz(row)) * 8) * 2u;
    }
  }
  // the dK/dV pass's two tiles: rows `stride` (Q) and `ostride` (dO) elements apart
  static __device__ __forceinline__ void piece_offsets2(int wave, int lane, int stride, int ostride,
                                                        unsigned (&qoff)[DKV_PIECES], unsigned (&ooff)[DKV_PIECES]) {
    piece_offsets<DKV_PIECES>(wave, lane, stride, qoff);
    piece_offsets<DKV_PIECES>(wave, lane, ostride, ooff);
  }
  // Row reads: row 16 t + li, chunk 4 ks + quad; the swizzle touches chunk bits 0-1, so k-steps differ by an immediate of
  // 64 B and sub-tiles by 16 rows.
  static __device__ __forceinline__ void row_offsets(int quad, int li, int (&off)[NROW]) {
    off[0] = li * ROW_BYTES + ((quad ^ fa7_swz(li)) << 4);
  }
  static __device__ __forceinline__ int row_addr(const int (&off)[NROW], int ks) { return ks * 64 + off[0]; }
  static __device__ __forceinline__ int row_addr(const int (&off)[NROW], int base, int ks) { return base + ks * 64 + off[0]; }
  // A operand = X^T fragment of a row-major LDS tile X[row][d] for the 16-dim tile dt and the 32-row step ks2 (fa_read_vt):
  // element e < 4: row 32 ks2 + 4 quad + e, e >= 4: the same + 16; M index (lane & 15) = dim 16 dt + li. The lane's address
  // for d-tile dt is tr_off[dt & 1] + 64 (dt >> 1): chunk 2 dt + ((li & 3) >> 1) with bits 0-1 swizzled by the row.
  static __device__ __forceinline__ void tr_offsets(int quad, int li, int (&off)[NTR]) {
    const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
    for (int d = 0; d < NTR; ++d) off[d] = ROW_BYTES * row + 16 * ((d * 2 + (p4 >> 1)) ^ fa7_swz(row)) + 8 * (p4 & 1);
  }
  static __device__ __forceinline__ int tr_addr(const int (&off)[NTR], int dt) { return (dt >> 1) * 64 + off[dt & 1]; }
  static __device__ __forceinline__ int tr_addr(const int (&off)[NTR], int base, int dt) { return base + (dt >> 1) * 64 + off[dt & 1]; }
};

__global__ __launch_bounds__(64 * AttnBwdHd96::DQ_WAVES, AttnBwdHd96::DQ_MIN_WG) void attn_bwd_hd96_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, int max_qblocks,
    const float* __restrict__ rope_cs) {
  using G = AttnBwdHd96;
#include "lr_attn_bwd_dq_body.h"
}

__global__ __launch_bounds__(64 * AttnBwdHd96::DKV_WAVES, AttnBwdHd96::DKV_MIN_WG) void attn_bwd_hd96_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, const float* __restrict__ rope_cs) {
  using G = AttnBwdHd96;
#include "lr_attn_bwd_dkv_body.h"
}

int lr_launch_attention_bwd_hd96(const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv,
                                 const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd,
                                 hipStream_t st, const float* rope_cs) {
  return lr_attn_bwd_launch<AttnBwdHd96, attn_bwd_hd96_dq_kernel, attn_bwd_hd96_dkv_kernel, 8>(
      "attn_bwd_hd96_dq_kernel", "attn_bwd_hd96_dkv_kernel", qkv, d_out, lse, dsum, dqkv, cu, cu_host, B, n_tok, nh, nkv, hd,
      st, rope_cs);
}
