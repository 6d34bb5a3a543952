// lr_attn_body.h -- what the MFMA flash-attention bodies at head_dim 64, 96 and 256 (llama_attn_hd64_body.h,
// llama_attn_hd96_body.h, llama_attn_hd256_body.h) have in common, once: the workgroup-to-(segment, head, tile) prologue, a
// segment's rows and K / V bases, the three-way staging of a key block, and the softmax, row-sum, V-read and store steps on a
// 16-row query tile against a 64-key block. What differs per head size -- the LDS layout and its swizzles, the DMA pieces per
// wave, the schedule of the QK product's K-fragment loads, the mask form -- stays in that head size's body; nothing here
// branches on the head size that calls it. Every helper is forced inline and picks its mode's expression at compile time
// (`if constexpr`, or a condition on the template parameters alone): without PREFIX no shared-prefix length is ever computed,
// compared or added, so the whole-prompt kernels' instructions do not depend on the optimiser folding a zero away. The early
// `return`s of the prologue stand in the bodies, between the helpers: inside a helper they change every kernel's code. So do
// smaller things: the whole-prompt kernels (attention variants 4, 5, 6's forward, 7 and the capped variant 4) are held to the
// instruction stream they had before these helpers existed, which is why a body keeps `pair` in a scope of its own and why
// fa_segment_and_head returns by value.
// A row's bits are the same in every mode of one head size because each mode runs these same lines on the same LDS image.
// The head_dim-128 body (llama_attn_hd128_body.h; llama_attn.hip and llama_attn_cached.hip) takes the softmax, row-sum, V-read
// and store steps and, for the cached kernels, fa_stage_block's form without a prefix; its prologues and variant 2's
// shared-prefix staging (per-lane addresses, not the descriptor forms here) are its kernels' own. The vector typedefs and
// FA_DEFER below are the ones every body uses.
#ifndef LR_ATTN_BODY_H
#define LR_ATTN_BODY_H

#include <type_traits>

#include "llama_kernels.h"
#include "lr_attn_util.h"
#include "lr_profile.h"

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;

#define FA_DEFER 8.0f   // a row's reference maximum moves only when a score exceeds it by more than 2^FA_DEFER

// ---- the modes ---------------------------------------------------------------------------------------------------------
// PREFIX: prefix_len = P > 0 makes segment 0 of the packed rows the P tokens every prompt starts with and segment s >= 1 the
//   rest of prompt s - 1 at positions P.. . Keys and values of positions < P are read from segment 0's rows; query tiles and
//   64-key blocks stay aligned to positions inside the prompt, prefix included; rows of a tile at positions < P belong to
//   segment 0 and are neither computed nor stored for segment s. Without PREFIX prefix_len is not read.
// LASTQ (with PREFIX; prefix_len may be 0): `qkv` is the [rows][2 nkv hd] K | V projection, q_rows_last one rotated query row
//   per prompt. A workgroup = one (prompt, head) walks the prompt's key blocks, every wave staging and wave 0 computing with
//   every lane column holding the query at position T - 1; one output row per prompt.

// The workgroup's (segment, head) pair and query tile, neither known as wave-uniform yet. LASTQ: a workgroup per pair. The body
// returns when pair >= n_pairs.
template <bool LASTQ>
__device__ __forceinline__ void fa_pair_of_workgroup(int n_pairs, int max_qblocks, int& pair, int& qb) {
  if constexpr (LASTQ) {
    pair = blockIdx.x;
    qb = 0;
  } else {
    fa_tile_of_workgroup(n_pairs, max_qblocks, pair, qb);
  }
}
// pair = seg * hg + h with hg heads (or head groups) per segment, both wave-uniform. Returned by value: with `int&` results
// the inlined code of attn_hd64_kernel<true> comes out in another order.
struct FaSegHead {
  int seg, h;
};
__device__ __forceinline__ FaSegHead fa_segment_and_head(int pair, int hg) {
  FaSegHead r;
  r.seg = __builtin_amdgcn_readfirstlane(pair / hg);
  r.h = __builtin_amdgcn_readfirstlane(pair - r.seg * hg);
  return r;
}

// A segment's rows: its first packed row, the shared-prefix keys in front of it, its length with them, and vtok0 such that
// the row of position p >= P is vtok0 + p (tok0 >= P: segment 0 precedes the segment). !PREFIX: P = 0 and vtok0 = tok0 are
// named by no expression of a body.
struct FaSeg {
  int tok0, P, T, vtok0;
};
template <bool PREFIX>
__device__ __forceinline__ FaSeg fa_segment_rows(const int32_t* cu, int seg, int prefix_len) {
  FaSeg s;
  s.tok0 = cu[seg];
  s.P = 0;
  s.vtok0 = s.tok0;
  if constexpr (PREFIX) {
    s.P = (prefix_len > 0 && seg > 0) ? prefix_len : 0;   // keys [0, P) live in segment 0's rows [0, P)
    s.T = s.P + cu[seg + 1] - s.tok0;                     // sequence length, prefix included
    s.vtok0 = s.tok0 - s.P;
  } else {
    s.T = cu[seg + 1] - s.tok0;
  }
  return s;
}

// A position's K / V row of KV head kvh: the segment's own rows (k, v; position p at row p), and with PREFIX packed row 0
// (pk, pv), where segment 0 starts. stride = elements per packed row.
struct FaKV {
  const u16 *k, *v, *pk, *pv;
  int stride;
};
template <bool LASTQ, bool PREFIX, int HD>
__device__ __forceinline__ FaKV fa_kv_bases(const u16* qkv, int nh, int nkv, int kvh, const FaSeg& s) {
  FaKV b;
  b.stride = LASTQ ? 2 * nkv * HD : (nh + 2 * nkv) * HD;
  b.pk = b.pv = nullptr;
  if constexpr (PREFIX) {
    b.pk = qkv + (LASTQ ? kvh * HD : (nh + kvh) * HD);
    b.pv = b.pk + nkv * HD;
    b.k = b.pk + (size_t)s.vtok0 * b.stride;
    b.v = b.pv + (size_t)s.vtok0 * b.stride;
  } else {
    b.k = qkv + (size_t)s.tok0 * b.stride + (nh + kvh) * HD;
    b.v = b.k + nkv * HD;
  }
  return b;
}

// The lane's query row at position qabs, from dimension 8 quad: q_rows_last's row of the prompt (LASTQ), or the packed row,
// clamped into the rows the segment owns (a clamped row is computed and not stored).
template <bool LASTQ, bool PREFIX, int HD>
__device__ __forceinline__ const u16* fa_q_ptr(const u16* qkv, const u16* q_rows_last, const FaSeg& s, int stride, int prompt,
                                               int qabs, int nh, int h, int quad) {
  if constexpr (LASTQ)
    return q_rows_last + (size_t)prompt * nh * HD + h * HD + quad * 8;
  else if constexpr (PREFIX)
    return qkv + (size_t)(s.vtok0 + min(max(qabs, s.P), s.T - 1)) * stride + h * HD + quad * 8;
  else
    return qkv + (size_t)(s.tok0 + min(qabs, s.T - 1)) * stride + h * HD + quad * 8;
}

// ---- staging one 64-key block by LDS-DMA ---------------------------------------------------------------------------------
// A wave moves NP pieces of 1 KiB (64 lanes x 16 B, lane-linear in LDS) of the K tile and of the V tile, TILE_BYTES apart;
// koff / voff = the lane's source byte offset inside the block per piece (row * stride plus the swizzled chunk: the swizzle is
// applied to the SOURCE chunk), row_of_piece(i) = the block row that offset stands in. Rows past the prompt's end are
// range-checked to zero by the per-block buffer descriptor's num_records (those keys are masked for every stored query row).
// Where a block's rows live is what the modes differ in, so each has its staging text. Without PREFIX every block takes a
// per-block descriptor (scalar work only). PREFIX: so does a block that lies wholly in the segment's own rows or wholly in
// segment 0. The one block that straddles position P is gathered from two places: its descriptor spans the packed rows from
// row 0 to the end of the segment's last row, and every lane adds the byte offset of ITS row's home (segment 0 for a key
// < P, the segment's own rows otherwise) to its block-invariant offset: one compare, one select and one add per piece in
// that block only. The LDS image of a block is the same bytes whatever the home of its rows, and the swizzle is a function
// of the row inside the block and the chunk, so the bank behaviour of the reads does not depend on the mode.
template <bool PREFIX, int HD, int KB, int NP, int TILE_BYTES, class RowOfPiece>
__device__ __forceinline__ void fa_stage_block(char* base, const FaKV& b, const FaSeg& s, int kb, const unsigned (&koff)[NP],
                                               const unsigned (&voff)[NP], RowOfPiece row_of_piece) {
  const int stride = b.stride;
  if constexpr (!PREFIX) {
    const size_t blk_off = (size_t)kb * KB * stride * 2;
    const int records = ((s.T - 1 - kb * KB) * stride + HD) * 2;   // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(b.k) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(b.v) + blk_off, records);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      fa_dma16(rk, base + i * 1024, koff[i]);
      fa_dma16(rv, base + TILE_BYTES + i * 1024, voff[i]);
    }
  } else {
    const int k0 = kb * KB, P = s.P;
    if (k0 >= P || k0 + KB <= P) {   // the whole block has one home: the segment's own rows, or segment 0
      const bool own = k0 >= P;
      const size_t blk_off = (size_t)k0 * stride * 2;
      const int records = (((own ? s.T : P) - 1 - k0) * stride + HD) * 2;
      const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(own ? b.k : b.pk) + blk_off, records);
      const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(own ? b.v : b.pv) + blk_off, records);
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        fa_dma16(rk, base + i * 1024, koff[i]);
        fa_dma16(rv, base + TILE_BYTES + i * 1024, voff[i]);
      }
    } else {
      const unsigned records = ((unsigned)(s.vtok0 + s.T - 1) * (unsigned)stride + HD) * 2u;
      const fa_int4 rk = fa_make_rsrc(b.pk, (int)records);
      const fa_int4 rv = fa_make_rsrc(b.pv, (int)records);
      const unsigned home_pre = (unsigned)k0 * (unsigned)stride * 2u, home_own = (unsigned)(s.vtok0 + k0) * (unsigned)stride * 2u;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const unsigned home = (k0 + row_of_piece(i) < P) ? home_pre : home_own;
        fa_dma16(rk, base + i * 1024, koff[i] + home);
        fa_dma16(rv, base + TILE_BYTES + i * 1024, voff[i] + home);
      }
    }
  }
}

// ---- one 16-row query tile against a 64-key block: st[nt][r] = raw score of key 16 nt + 4 quad + r, lane column = query ----
// the maximum of this lane's 16 keys of the row
__device__ __forceinline__ float fa_max16(const floatx4 (&st)[4]) {
  float mx = fa_max3(st[0][0], st[0][1], st[0][2]);
  mx = fa_max3(mx, st[0][3], st[1][0]);
#pragma unroll
  for (int nt = 1; nt < 4; ++nt) {
    mx = fa_max3(mx, st[nt][1], st[nt][2]);
    if (nt < 3) mx = fa_max3(mx, st[nt][3], st[nt + 1][0]);
  }
  return fa_max2(mx, st[3][3]);
}

// Deferred maximum, decided per row (variant 2): a row that keeps its reference multiplies by exactly 1. m_run = the row's
// reference in log2 units, mthr = (m_run + FA_DEFER) / scale in raw-score units, sl2 = scale * log2(e), inv_sl2 = 1 / sl2.
template <int DT>
__device__ __forceinline__ void fa_rescale(float mx, float sl2, float inv_sl2, float& m_run, float& mthr, floatx4& l_acc,
                                           floatx4 (&ot)[DT]) {
  if (__any(mx > mthr)) {
    const float rmx = fa_max_xor16_32(mx);
    const bool grew = rmx > mthr;
    const float m_new = grew ? rmx * sl2 : m_run;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
    for (int r = 0; r < 4; ++r) l_acc[r] *= alpha;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) ot[dt][r] *= alpha;
    m_run = m_new;
    mthr = (m_new + FA_DEFER) * inv_sl2;
  }
}

// P = exp2(score * sl2 - m) in bf16, packed as the B operand of O^T = V^T P^T: k index 8 quad + j of pa[ks2] <-> key
// 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it
__device__ __forceinline__ void fa_pack_p(const floatx4 (&st)[4], float sl2, float m_cur, bf16x8 (&pa)[2]) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      pa[nt >> 1][(nt & 1) * 4 + r] = (__bf16)__builtin_amdgcn_exp2f(__builtin_fmaf(st[nt][r], sl2, -m_cur));
}

// the row sum takes the bf16 P the numerator takes: an MFMA against a row of ones
__device__ __forceinline__ void fa_row_sum(bf16x8 ones_f, bf16x8 p, floatx4& l_acc) {
  l_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, p, l_acc, 0, 0, 0);
}

// The A operand of O^T += V^T P^T from the row-major V tile: two transposed reads (ds_read_b64_tr_b16) at the lane's address
// p (row 4 quad + (li >> 2) of a 32-key half, dims 16 dt + 4 (li & 3)) and 16 rows further
template <int ROW_BYTES>
__device__ __forceinline__ bf16x8 fa_read_vt(lds_char* p) {
  const short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)p);
  const short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(p + 16 * ROW_BYTES));
  bf16x8 vf;
  const bf16x4 b0 = __builtin_bit_cast(bf16x4, t0), b1 = __builtin_bit_cast(bf16x4, t1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    vf[r] = b0[r];
    vf[4 + r] = b1[r];
  }
  return vf;
}

// ---- normalise and store: lane owns query row li, d = 16 dt + 4 quad + r. v_permlane16_swap on the packed tiles (2k, 2k+1)
// gives even quads d = 32 k + 8 (quad / 2) .. +7 and odd quads the same + 16: 16-byte stores, DT / 2 per row and lane. Every
// lane takes part in the swaps; only rows of this segment store. LASTQ: the 16 lane columns of wave 0 hold the same row;
// column 0's four quads store its dims.
template <bool LASTQ, bool PREFIX>
__device__ __forceinline__ bool fa_row_live(const FaSeg& s, int qabs, int wave, int li) {
  return LASTQ ? (wave == 0 && li == 0) : (qabs < s.T && (!PREFIX || qabs >= s.P));
}
// the row of `out` the lane's swaps and stores address: its own if live, else one the segment owns (nothing is stored there)
template <bool LASTQ, bool PREFIX>
__device__ __forceinline__ int fa_out_row(const FaSeg& s, int prompt, bool live, int qabs) {
  if constexpr (LASTQ)
    return prompt;
  else if constexpr (PREFIX)
    return s.vtok0 + (live ? qabs : s.P);
  else
    return s.tok0 + (live ? qabs : 0);
}
template <int DT>
__device__ __forceinline__ void fa_store_row(const floatx4 (&ot)[DT], float inv, bool live, u16* op) {
#pragma unroll
  for (int k = 0; k < DT / 2; ++k) {
    unsigned a[2], b[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      a[w] = (unsigned)f2bf(ot[2 * k][2 * w] * inv) | ((unsigned)f2bf(ot[2 * k][2 * w + 1] * inv) << 16);
      b[w] = (unsigned)f2bf(ot[2 * k + 1][2 * w] * inv) | ((unsigned)f2bf(ot[2 * k + 1][2 * w + 1] * inv) << 16);
      const auto sw = __builtin_amdgcn_permlane16_swap(a[w], b[w], false, false);
      a[w] = sw[0];
      b[w] = sw[1];
    }
    if (live) {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<u32x4*>(op + k * 32) = u32x4{a[0], a[1], b[0], b[1]};
    }
  }
}

#endif
