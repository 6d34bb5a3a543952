// llama_attn_hd64_body.h -- the one text of the head_dim-64 MFMA attention (llama_attn_hd64.hip: read its header first),
// attn_hd64_body<LASTQ, PREFIX, LSE>, inlined into four kernels in three translation units:
//   <false, false, false>  attn_hd64_kernel<false>, attention variant 5                          (llama_attn_hd64.hip)
//   <false, false, true>   attn_hd64_kernel<true>, variant 6's training forward: one lse store per row and head more
//                                                                                                (llama_attn_hd64_lse.hip)
//   <false, true, false>   attn_hd64_prefix_kernel<false>, shared prompt prefix                  (llama_attn_hd64_prefix.hip)
//   <true, true, false>    attn_hd64_prefix_kernel<true>, one query row per prompt               (llama_attn_hd64_prefix.hip)
// The modes differ in where a K / V row and a query row live and in which rows a tile owns. Each such place picks its
// expression at compile time (`if constexpr`, or a condition on the template parameters alone): without PREFIX no shared-prefix
// length is ever computed, compared or added, so variant 5's instructions do not depend on the optimiser folding a zero away.
// The block walk, the masking, the per-row deferred maximum, bf16 P into both products and the ones-MFMA row sum are common to
// all four, which is what makes a row's bits the same in every mode.
#ifndef LLAMA_ATTN_HD64_BODY_H
#define LLAMA_ATTN_HD64_BODY_H

#include <type_traits>

#include "llama_kernels.h"
#include "lr_attn_util.h"
#include "lr_profile.h"

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

#define FA5_HD 64
#ifndef FA5_QT
#define FA5_QT 2                          // 16-row query tiles per wave (the A/B arm of DESIGN 10 builds with 4)
#endif
#ifndef FA5_MIN_WG
#define FA5_MIN_WG 3                      // workgroups per CU = waves per SIMD the register budget is held to (<= 168)
#endif
#define FA5_WAVES 4
#define FA5_QROWS (FA5_WAVES * 16 * FA5_QT)   // query rows per workgroup
#define FA5_KB 64                         // keys per block
#define FA5_ROW_BYTES (FA5_HD * 2)        // one K or V row in LDS: 128 B = 8 chunks of 16 B; two rows span the 64 banks
#define FA5_TILE_BYTES (FA5_KB * FA5_ROW_BYTES)   // 8 KiB
#define FA5_STAGE_BYTES (2 * FA5_TILE_BYTES)      // K tile + V tile
#define FA5_LDS_BYTES (2 * FA5_STAGE_BYTES)       // two stages: 32 KiB
#define FA5_DEFER 8.0f

// Swizzles on the 3-bit chunk index of a 128-byte row; the 16-byte bank slot of chunk position p of row r is 8 (r & 1) + p.
// K tile: position c ^ ((r >> 1) & 7). A ds_read_b128 lane group holds 16 rows distinct mod 16 at one chunk per quad: rows
//   of equal parity differ in (r >> 1) & 7, so the group covers all 16 slots.
// V tile: position c ^ (((r >> 1) & 3) << 1). A 32-lane half of a transposed read takes 8 rows x 32 B (chunks 2 dt, 2 dt + 1):
//   the four rows of equal parity land on four different chunk pairs. Bit 0 is untouched, so a row's 32 bytes stay in order.
// Both depend on row bits 1..3 only: sub-tiles 16 rows apart differ by an immediate.
__device__ __forceinline__ int fa5_kswz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int fa5_vswz(int row) { return ((row >> 1) & 3) << 1; }

// PREFIX: prefix_len = P > 0 makes segment 0 of the packed rows the P tokens every prompt starts with and segment s >= 1 the
//   rest of prompt s - 1 at positions P.. . Keys and values of positions < P are read from segment 0's rows; query tiles and
//   64-key blocks stay aligned to positions inside the prompt, prefix included; rows of a tile at positions < P belong to
//   segment 0 and are neither computed nor stored for segment s. Without PREFIX prefix_len is not read.
// LASTQ (with PREFIX; prefix_len may be 0): `qkv` is the [rows][2 nkv hd] K | V projection, q_rows_last one rotated query row
//   per prompt. A workgroup = one (prompt, head) walks the prompt's key blocks, all four waves staging and wave 0 computing with
//   every lane column holding the query at position T - 1; one output row per prompt.
// LSE (alone): lse[token][head] = natural-log log-sum-exp of the row's scaled scores.
template <bool LASTQ, bool PREFIX, bool LSE>
__device__ __forceinline__ void attn_hd64_body(const u16* qkv, u16* out, const int32_t* cu, int prefix_len, int nh, int nkv,
                                               int max_qblocks, int n_pairs, float* lse, const u16* q_rows_last) {
  static_assert(!LSE || (!PREFIX && !LASTQ), "the lse store exists without a shared prefix and for whole tiles only");
  static_assert(!LASTQ || PREFIX, "the last-row mode reads a shared prefix");
  constexpr int QT = LASTQ ? 1 : FA5_QT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hd = FA5_HD;
  int seg, h, qb;
  {
    int pair;
    if constexpr (LASTQ) {
      pair = blockIdx.x;
      qb = 0;
    } else {
      fa_tile_of_workgroup(n_pairs, max_qblocks, pair, qb);
    }
    if (pair >= n_pairs) return;
    seg = __builtin_amdgcn_readfirstlane(pair / nh);
    h = __builtin_amdgcn_readfirstlane(pair - seg * nh);
    if constexpr (LASTQ) {
      if (prefix_len > 0 && seg == 0) return;   // segment 0 is the shared prefix, not a prompt
    } else {
      qb = __builtin_amdgcn_readfirstlane(qb);
    }
  }
  const int tok0 = cu[seg];
  int P = 0, T, vtok0 = tok0;   // !PREFIX: P and vtok0 are named by no expression below
  if constexpr (PREFIX) {
    P = (prefix_len > 0 && seg > 0) ? prefix_len : 0;   // keys [0, P) live in segment 0's rows [0, P)
    T = P + cu[seg + 1] - tok0;                         // sequence length, prefix included
    vtok0 = tok0 - P;   // the row of position p >= P is vtok0 + p (tok0 >= P: segment 0 precedes the segment)
  } else {
    T = cu[seg + 1] - tok0;
  }
  // no query row of this segment in the tile
  if (!LASTQ && (qb * FA5_QROWS >= T || (PREFIX && (qb + 1) * FA5_QROWS <= P))) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const int stride = LASTQ ? 2 * nkv * hd : (nh + 2 * nkv) * hd;
  const u16 *kbase, *vbase, *pkbase = nullptr, *pvbase = nullptr;   // a position's K / V row: own rows, and (PREFIX) packed row 0
  if constexpr (PREFIX) {
    pkbase = qkv + (LASTQ ? kvh * hd : (nh + kvh) * hd);
    pvbase = pkbase + nkv * hd;
    kbase = pkbase + (size_t)vtok0 * stride;
    vbase = pvbase + (size_t)vtok0 * stride;
  } else {
    kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
    vbase = kbase + nkv * hd;
  }
  const int prompt = prefix_len > 0 ? seg - 1 : seg;         // LASTQ: row of q_rows_last / out

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32 ks + 8 quad + 0..7
  const int wave_q0 = LASTQ ? T - 1 : qb * FA5_QROWS + wave * (16 * QT);
  bf16x8 qf[QT][2];
  int qabs[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qabs[qt] = LASTQ ? T - 1 : wave_q0 + qt * 16 + li;
    const u16* qp;
    if constexpr (LASTQ)
      qp = q_rows_last + (size_t)prompt * nh * hd + h * hd + quad * 8;
    else if constexpr (PREFIX)
      qp = qkv + (size_t)(vtok0 + min(max(qabs[qt], P), T - 1)) * stride + h * hd + quad * 8;
    else
      qp = qkv + (size_t)(tok0 + min(qabs[qt], T - 1)) * stride + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }
  floatx4 ot[QT][4];
  floatx4 l_acc[QT];
  float m_run[QT], mthr[QT];   // mthr = (m + FA5_DEFER) / scale of the lane's row, in raw-score units
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ot[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    l_acc[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
    m_run[qt] = -__builtin_inff();
    mthr[qt] = -__builtin_inff();
  }
  bf16x8 ones_f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = LASTQ ? T - 1 : min(qb * FA5_QROWS + FA5_QROWS - 1, T - 1);
  const int kb_last = q_last / FA5_KB;
  const int wave_q_last = LASTQ ? T - 1 : wave_q0 + 16 * QT - 1;
  // the wave owns at least one row of this segment (LASTQ: wave 0 computes, every wave stages)
  const bool wave_live = LASTQ ? wave == 0 : (wave_q0 < T && (!PREFIX || wave_q_last >= P));
  const float sl2 = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging: a tile is 8 pieces of 1 KiB (8 rows x 128 B, lane-linear in LDS); wave w moves pieces 2w, 2w + 1 of
  // K and of V. The swizzle is applied to the SOURCE chunk. Rows past the prompt's end are range-checked to zero by the
  // per-block buffer descriptor (those keys are masked for every stored query row).
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned koff[2], voff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wave * 2 + i) * 8 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ fa5_kswz(row)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ fa5_vswz(row)) * 8) * 2u;
  }
  // Where a block's rows live is what the modes differ in, so each has its staging text. Without PREFIX every block takes a
  // per-block descriptor (scalar work only). PREFIX: so does a block that lies wholly in the segment's own rows or wholly in
  // segment 0. The one block that straddles position P is gathered from two places: its descriptor spans the packed rows from
  // row 0 to the end of the segment's last row, and every lane adds the byte offset of ITS row's home (segment 0 for a key
  // < P, the segment's own rows otherwise) to its block-invariant offset: one compare, one select and one add per piece in
  // that block only. The LDS image of a block is the same bytes whatever the home of its rows, and the swizzle is a function
  // of the row inside the block and the chunk, so the bank behaviour of the reads does not depend on the mode.
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * FA5_STAGE_BYTES + wave * 2048;
    if constexpr (!PREFIX) {
      const size_t blk_off = (size_t)kb * FA5_KB * stride * 2;
      const int records = ((T - 1 - kb * FA5_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
      const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
      const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa_dma16(rk, base + i * 1024, koff[i]);
        fa_dma16(rv, base + FA5_TILE_BYTES + i * 1024, voff[i]);
      }
    } else {
      const int k0 = kb * FA5_KB;
      if (k0 >= P || k0 + FA5_KB <= P) {   // the whole block has one home: the segment's own rows, or segment 0
        const bool own = k0 >= P;
        const size_t blk_off = (size_t)k0 * stride * 2;
        const int records = (((own ? T : P) - 1 - k0) * stride + hd) * 2;
        const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(own ? kbase : pkbase) + blk_off, records);
        const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(own ? vbase : pvbase) + blk_off, records);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa_dma16(rk, base + i * 1024, koff[i]);
          fa_dma16(rv, base + FA5_TILE_BYTES + i * 1024, voff[i]);
        }
      } else {
        const unsigned records = ((unsigned)(vtok0 + T - 1) * (unsigned)stride + hd) * 2u;
        const fa_int4 rk = fa_make_rsrc(pkbase, (int)records);
        const fa_int4 rv = fa_make_rsrc(pvbase, (int)records);
        const unsigned home_pre = (unsigned)k0 * (unsigned)stride * 2u, home_own = (unsigned)(vtok0 + k0) * (unsigned)stride * 2u;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = (wave * 2 + i) * 8 + prow;
          const unsigned home = (k0 + row < P) ? home_pre : home_own;
          fa_dma16(rk, base + i * 1024, koff[i] + home);
          fa_dma16(rv, base + FA5_TILE_BYTES + i * 1024, voff[i] + home);
        }
      }
    }
  };

  // LDS read addresses, lane-dependent part computed once. K: row nt*16 + li, chunk 4 ks + quad. V^T (transposed reads):
  // row quad*4 + (li >> 2) (+16, +32, +48 per key sub-block), dims 16 dt + 4 (li & 3).
  typedef __attribute__((address_space(3))) char lds_char;
  lds_char* const lds = (lds_char*)smem;
  lds_char *kb_off[2], *vb_off[4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) kb_off[ks] = lds + (li * FA5_ROW_BYTES + (((ks * 4 + quad) ^ fa5_kswz(li)) << 4));
  {
    const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      vb_off[dt] = lds + (FA5_ROW_BYTES * row + 16 * ((dt * 2 + (p4 >> 1)) ^ fa5_vswz(row)) + 8 * (p4 & 1));
  }

  stage(0, 0);
  // Q must be resident before the loop (llama_attn.hip): otherwise its pending loads are waited for behind the in-loop DMA
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) asm volatile("" ::"v"(qf[qt][ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMAs of block 0 (hipcc does not count them)
  __syncthreads();

  auto block = [&](const int kb, auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    constexpr int KS = BUF * FA5_STAGE_BYTES, VS = KS + FA5_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, BUF ^ 1);
    if (wave_live && kb * FA5_KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T : st[qt][nt] rows = keys nt*16 + 4*quad + r, col = query li
      floatx4 st[QT][4];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
      typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
      bf16x8 kf[2][4];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          kf[ks][nt] = *reinterpret_cast<lds_bf16x8*>(kb_off[ks] + (KS + nt * 16 * FA5_ROW_BYTES));
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            st[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks][nt], qf[qt][ks], st[qt][nt], 0, 0, 0);

      // ---- online softmax (lane-local row), P packed as the B operand of O^T = V^T P^T
      bf16x8 pa[QT][2];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const bool diag = (kb * FA5_KB + FA5_KB - 1) > wave_q0 + qt * 16;   // the block needs masking (wave-uniform)
        if (diag) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kb * FA5_KB + nt * 16 + quad * 4 + r;
              st[qt][nt][r] = (key <= qabs[qt]) ? st[qt][nt][r] : -__builtin_inff();
            }
          __builtin_amdgcn_sched_barrier(0);
        }
        float mx = fa_max3(st[qt][0][0], st[qt][0][1], st[qt][0][2]);
        mx = fa_max3(mx, st[qt][0][3], st[qt][1][0]);
#pragma unroll
        for (int nt = 1; nt < 4; ++nt) {
          mx = fa_max3(mx, st[qt][nt][1], st[qt][nt][2]);
          if (nt < 3) mx = fa_max3(mx, st[qt][nt][3], st[qt][nt + 1][0]);
        }
        mx = fa_max2(mx, st[qt][3][3]);      // this lane's 16 keys of the row
        // deferred maximum, decided per row (variant 2): a row that keeps its reference multiplies by exactly 1
        if (__any(mx > mthr[qt])) {
          const float rmx = fa_max_xor16_32(mx);
          const bool grew = rmx > mthr[qt];
          const float m_new = grew ? rmx * sl2 : m_run[qt];
          const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);
#pragma unroll
          for (int r = 0; r < 4; ++r) l_acc[qt][r] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[qt][dt][r] *= alpha;
          m_run[qt] = m_new;
          mthr[qt] = (m_new + FA5_DEFER) * inv_sl2;
        }
        const float m_cur = m_run[qt];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            pa[qt][nt >> 1][(nt & 1) * 4 + r] = (__bf16)__builtin_amdgcn_exp2f(__builtin_fmaf(st[qt][nt][r], sl2, -m_cur));
      }
      // ---- O^T += V^T P^T (k index 8 quad + j <-> key 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) l_acc[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pa[qt][ks2], l_acc[qt], 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int o = VS + ks2 * 32 * FA5_ROW_BYTES;
          const short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt] + o));
          const short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt] + (o + 16 * FA5_ROW_BYTES)));
          bf16x8 vf;
          const bf16x4 b0 = __builtin_bit_cast(bf16x4, t0), b1 = __builtin_bit_cast(bf16x4, t1);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            vf[r] = b0[r];
            vf[4 + r] = b1[r];
          }
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            ot[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa[qt][ks2], ot[qt][dt], 0, 0, 0);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of block kb + 1 have landed
    __syncthreads();                                   // ... and every wave is done with block kb
  };
  for (int kb = 0; kb <= kb_last; kb += 2) {
    block(kb, std::integral_constant<int, 0>{});
    if (kb + 1 <= kb_last) block(kb + 1, std::integral_constant<int, 1>{});
  }

  // ---- normalise and store: lane owns query row li, d = 16 dt + 4 quad + r. v_permlane16_swap on the packed tiles
  // (2k, 2k+1) gives even quads d = 32 k + 8 (quad / 2) .. +7 and odd quads the same + 16: 16-byte stores. Every lane
  // takes part in the swaps; only rows of this segment store. LASTQ: the 16 lane columns of wave 0 hold the same row;
  // column 0's four quads store its 64 dims.
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float inv = 1.0f / l_acc[qt][0];
    const bool live = LASTQ ? (wave == 0 && li == 0) : (qabs[qt] < T && (!PREFIX || qabs[qt] >= P));
    if (LSE && live && quad == 0)   // the lane's row: m (log2 units) + log2 l, as natural log
      lse[(size_t)(tok0 + qabs[qt]) * nh + h] = (m_run[qt] + __builtin_amdgcn_logf(l_acc[qt][0])) * 0.6931471805599453f;
    int orow;
    if constexpr (LASTQ)
      orow = prompt;
    else if constexpr (PREFIX)
      orow = vtok0 + (live ? qabs[qt] : P);
    else
      orow = tok0 + (live ? qabs[qt] : 0);
    u16* op = out + (size_t)orow * nh * hd + h * hd + (quad & 1) * 16 + (quad >> 1) * 8;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      unsigned a[2], b[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        a[w] = (unsigned)f2bf(ot[qt][2 * k][2 * w] * inv) | ((unsigned)f2bf(ot[qt][2 * k][2 * w + 1] * inv) << 16);
        b[w] = (unsigned)f2bf(ot[qt][2 * k + 1][2 * w] * inv) | ((unsigned)f2bf(ot[qt][2 * k + 1][2 * w + 1] * inv) << 16);
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
}

template <bool LSE>
__global__ __launch_bounds__(256, FA5_MIN_WG) void attn_hd64_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu, int nh,
                                                           int nkv, int max_qblocks, int n_pairs, float* lse) {
  attn_hd64_body<false, false, LSE>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, lse, nullptr);
}

#endif
