// llama_attn_hd96_body.h -- the one text of the head_dim-96 MFMA attention (llama_attn_hd96.hip: read its header first),
// attn_hd96_body<LASTQ, PREFIX>, inlined into three kernels in two translation units:
//   <false, false>  attn_hd96_kernel, attention variant 7                        (llama_attn_hd96.hip)
//   <false, true>   attn_hd96_prefix_kernel<false>, shared prompt prefix          (llama_attn_hd96_prefix.hip)
//   <true, true>    attn_hd96_prefix_kernel<true>, one query row per prompt       (llama_attn_hd96_prefix.hip)
// The structure is that of llama_attn_hd64_body.h (four waves, S^T = K Q^T, P from registers into O^T = V^T P^T, per-row
// deferred maximum, bf16 P into both products and the ones-MFMA row sum, two-stage LDS ring by inline-asm LDS-DMA with the
// hand-written vmcnt wait in front of the block barrier). The modes differ in where a K / V row and a query row live and in
// which rows a tile owns; each such place picks its expression at compile time, so a row's bits are the same in every mode.
// No lse and no backward exist at this head size.
//
// What differs at 96: a K or V row is 192 B = 12 chunks of 16 B (not a power of two), the QK product has 3 k-steps of 32 and
// O has 6 d-tiles of 16.
//
// LDS layout: derived from the bank rule -- bank = (byte / 4) mod 64, i.e. 16 slots of 16 B -- and then CONFIRMED with the LDS
// bank-conflict counter for both kinds of read at once: SQ_LDS_BANK_CONFLICT = 0 of 33.6 M SQ_LDS_IDX_ACTIVE cycles over two
// launches of variant 7 on 16 prompts of 1125 tokens at (32, 32) heads, a counter-only run. Rows are stored back to back at a 192-byte stride, so the slot of chunk position p of row r is
// (12 r + p) mod 16 = (4 (3 (r & 3) mod 4) + p) mod 16: the stride alone rotates rows over the slots with period 4, and the
// four rows r & 3 = 0..3 of a position start at slots 0, 12, 8, 4. A swizzle may XOR bits 0-1 of the chunk index only: then a
// chunk stays inside its aligned group of four and below 12.
// K tile: position c ^ fa7_swz(r), fa7_swz(r) = (-(r >> 2)) & 3 = {0, 3, 2, 1}[(r >> 2) & 3]. A ds_read_b128 is served in
//   four 16-lane groups that are not the quads: a group holds rows {0-3, 12-15} at the chunk of quad q and rows {4-11} at the
//   chunk of quad q ^ 1 (same k-step). Bits 2-3 of the slot are (3 (r & 3) + ks) mod 4: distinct over r & 3. Bits 0-1 are
//   q ^ f(j) for row group j = r >> 2 in {0, 3} and q ^ 1 ^ f(j) for j in {1, 2}: with f = {0, 3, 2, 1} these are q ^ {0, 1}
//   and q ^ {2, 3}: four different values. So the 16 lanes of a group sit on 16 different slots. (The identity f(j) = j gives
//   q ^ {0, 3, 0, 3}: two-way conflicts under this grouping. Any bijection f is conflict-free if a group were one quad.)
// V tile: the same swizzle, so one set of per-lane source offsets stages both tiles. A 32-lane half of a ds_read_b64_tr_b16
//   takes 8 rows x 32 B (chunks 2 dt, 2 dt + 1 of rows 8 m .. 8 m + 7): in 32-byte units the slot of row r is
//   (6 r + c / 2) mod 8, and 6 r mod 8 = {0, 6, 4, 2} for r & 3 = 0..3: all even, so rows r and r + 4 would meet. What
//   separates them is chunk bit 1 (bit 0 of the 32-byte index) differing between row groups j = 2 m and 2 m + 1: bit 1 of
//   f is {0, 1, 1, 0}, which does. 8 rows then sit on 8 different 32-byte slots = all 64 banks once. f's bit 0 swaps the two
//   16-byte halves of a row's 32 bytes inside their slot; every lane addresses its own 8 bytes, so the read does not care.
// The swizzle depends on row bits 2..3 only: sub-tiles 16 rows apart differ by an immediate.
#ifndef LLAMA_ATTN_HD96_BODY_H
#define LLAMA_ATTN_HD96_BODY_H

#include <type_traits>

#include "llama_kernels.h"
#include "lr_attn_util.h"
#include "lr_profile.h"

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

#define FA7_HD 96
#define FA7_QT 2                          // 16-row query tiles per wave
#define FA7_MIN_WG 3                      // workgroups per CU = waves per SIMD the register budget is held to (<= 168)
#define FA7_WAVES 4
#define FA7_QROWS (FA7_WAVES * 16 * FA7_QT)   // query rows per workgroup
#define FA7_KB 64                         // keys per block
#define FA7_KSTEPS (FA7_HD / 32)          // 3 k-steps of the QK product
#define FA7_DT (FA7_HD / 16)              // 6 d-tiles of O
#define FA7_ROW_BYTES (FA7_HD * 2)        // one K or V row in LDS: 192 B = 12 chunks of 16 B
#define FA7_ROW_CHUNKS 12
#define FA7_TILE_BYTES (FA7_KB * FA7_ROW_BYTES)   // 12 KiB = 12 DMA pieces of 1 KiB
#define FA7_WAVE_PIECES 3                 // per wave, of K and of V: three pieces = exactly 16 rows
#define FA7_STAGE_BYTES (2 * FA7_TILE_BYTES)      // K tile + V tile
#define FA7_LDS_BYTES (2 * FA7_STAGE_BYTES)       // two stages: 48 KiB
#define FA7_DEFER 8.0f                    // FA5_DEFER's rule

__device__ __forceinline__ int fa7_swz(int row) { return (0 - (row >> 2)) & 3; }

// PREFIX, LASTQ: as in llama_attn_hd64_body.h. prefix_len = P > 0 makes segment 0 of the packed rows the P tokens every prompt
//   starts with and segment s >= 1 the rest of prompt s - 1 at positions P.. ; LASTQ (with PREFIX; prefix_len may be 0): `qkv`
//   is the [rows][2 nkv hd] K | V projection, q_rows_last one rotated query row per prompt, a workgroup = one (prompt, head)
//   with all four waves staging and wave 0 computing, every lane column holding the query at position T - 1.
template <bool LASTQ, bool PREFIX>
__device__ __forceinline__ void attn_hd96_body(const u16* qkv, u16* out, const int32_t* cu, int prefix_len, int nh, int nkv,
                                               int max_qblocks, int n_pairs, const u16* q_rows_last) {
  static_assert(!LASTQ || PREFIX, "the last-row mode reads a shared prefix");
  constexpr int QT = LASTQ ? 1 : FA7_QT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hd = FA7_HD;
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
  if (!LASTQ && (qb * FA7_QROWS >= T || (PREFIX && (qb + 1) * FA7_QROWS <= P))) return;
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
  const int wave_q0 = LASTQ ? T - 1 : qb * FA7_QROWS + wave * (16 * QT);
  // the lane's query position in tile qt (not kept in a register across the block loop: the loop masks by `dq` below)
  auto qabs_of = [&](int qt) { return LASTQ ? T - 1 : wave_q0 + qt * 16 + li; };
  // key kb*64 + nt*16 + 4 quad + r <= qabs  <=>  kb*64 + nt*16 + r - wave_q0 - 16 qt (wave-uniform) <= dq
  const int dq = (LASTQ ? 0 : li) - quad * 4;
  bf16x8 qf[QT][FA7_KSTEPS];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qabs = qabs_of(qt);
    const u16* qp;
    if constexpr (LASTQ)
      qp = q_rows_last + (size_t)prompt * nh * hd + h * hd + quad * 8;
    else if constexpr (PREFIX)
      qp = qkv + (size_t)(vtok0 + min(max(qabs, P), T - 1)) * stride + h * hd + quad * 8;
    else
      qp = qkv + (size_t)(tok0 + min(qabs, T - 1)) * stride + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < FA7_KSTEPS; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }
  floatx4 ot[QT][FA7_DT];
  floatx4 l_acc[QT];
  float m_run[QT], mthr[QT];   // mthr = (m + FA7_DEFER) / scale of the lane's row, in raw-score units
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < FA7_DT; ++dt) ot[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    l_acc[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
    m_run[qt] = -__builtin_inff();
    mthr[qt] = -__builtin_inff();
  }
  bf16x8 ones_f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = LASTQ ? T - 1 : min(qb * FA7_QROWS + FA7_QROWS - 1, T - 1);
  const int kb_last = q_last / FA7_KB;
  const int wave_q_last = LASTQ ? T - 1 : wave_q0 + 16 * QT - 1;
  // the wave owns at least one row of this segment (LASTQ: wave 0 computes, every wave stages)
  const bool wave_live = LASTQ ? wave == 0 : (wave_q0 < T && (!PREFIX || wave_q_last >= P));
  const float sl2 = 0.10206207261596575f * 1.4426950408889634f;  // 1/sqrt(96) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging: a tile is 12 pieces of 1 KiB (lane-linear in LDS: 64 chunks = 5 1/3 rows); wave w moves pieces 3w .. 3w + 2
  // of K and of V, which are exactly rows 16 w .. 16 w + 15. Lane l of piece i writes linear chunk 64 i + l of the wave's 192:
  // row 16 w + (64 i + l) / 12 at position (64 i + l) % 12. The swizzle is applied to the SOURCE chunk. Rows past the prompt's
  // end are range-checked to zero by the per-block buffer descriptor's num_records (and those keys are masked in P for every
  // stored query row: a key past T - 1 is past every query position).
  unsigned soff[FA7_WAVE_PIECES];   // K and V alike: V's rows stand nkv hd elements behind K's, which the descriptors' bases carry
#pragma unroll
  for (int i = 0; i < FA7_WAVE_PIECES; ++i) {
    const int g = i * 64 + lane, r16 = g / FA7_ROW_CHUNKS, ppos = g - r16 * FA7_ROW_CHUNKS;
    const int row = wave * 16 + r16;
    soff[i] = (unsigned)(row * stride + (ppos ^ fa7_swz(row)) * 8) * 2u;
  }
  // Where a block's rows live is what the modes differ in, so each has its staging text (llama_attn_hd64_body.h): a per-block
  // descriptor where the block has one home, and for the one block that straddles position P a descriptor over the packed
  // rows from row 0 with every lane adding the byte offset of its row's home.
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * FA7_STAGE_BYTES + wave * (FA7_WAVE_PIECES * 1024);
    if constexpr (!PREFIX) {
      const size_t blk_off = (size_t)kb * FA7_KB * stride * 2;
      const int records = ((T - 1 - kb * FA7_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
      const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
      const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
      for (int i = 0; i < FA7_WAVE_PIECES; ++i) {
        fa_dma16(rk, base + i * 1024, soff[i]);
        fa_dma16(rv, base + FA7_TILE_BYTES + i * 1024, soff[i]);
      }
    } else {
      const int k0 = kb * FA7_KB;
      if (k0 >= P || k0 + FA7_KB <= P) {   // the whole block has one home: the segment's own rows, or segment 0
        const bool own = k0 >= P;
        const size_t blk_off = (size_t)k0 * stride * 2;
        const int records = (((own ? T : P) - 1 - k0) * stride + hd) * 2;
        const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(own ? kbase : pkbase) + blk_off, records);
        const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(own ? vbase : pvbase) + blk_off, records);
#pragma unroll
        for (int i = 0; i < FA7_WAVE_PIECES; ++i) {
          fa_dma16(rk, base + i * 1024, soff[i]);
          fa_dma16(rv, base + FA7_TILE_BYTES + i * 1024, soff[i]);
        }
      } else {
        const unsigned records = ((unsigned)(vtok0 + T - 1) * (unsigned)stride + hd) * 2u;
        const fa_int4 rk = fa_make_rsrc(pkbase, (int)records);
        const fa_int4 rv = fa_make_rsrc(pvbase, (int)records);
        const unsigned home_pre = (unsigned)k0 * (unsigned)stride * 2u, home_own = (unsigned)(vtok0 + k0) * (unsigned)stride * 2u;
#pragma unroll
        for (int i = 0; i < FA7_WAVE_PIECES; ++i) {
          const int row = wave * 16 + (i * 64 + lane) / FA7_ROW_CHUNKS;
          const unsigned home = (k0 + row < P) ? home_pre : home_own;
          fa_dma16(rk, base + i * 1024, soff[i] + home);
          fa_dma16(rv, base + FA7_TILE_BYTES + i * 1024, soff[i] + home);
        }
      }
    }
  };

  // LDS read addresses, lane-dependent part computed once. K: row nt*16 + li, chunk 4 ks + quad: the swizzle touches bits 0-1,
  // so k-steps differ by an immediate of 64 B. V^T (transposed reads): row quad*4 + (li >> 2) (+16, +32, +48 per key
  // sub-block), dims 16 dt + 4 (li & 3): chunk 2 dt + ((li & 3) >> 1) with bits 0-1 swizzled by the row, so the d-tiles are
  // two addresses (dt even, dt odd) plus immediates of 64 B.
  typedef __attribute__((address_space(3))) char lds_char;
  lds_char* const lds = (lds_char*)smem;
  lds_char* const kb_off = lds + (li * FA7_ROW_BYTES + ((quad ^ fa7_swz(li)) << 4));
  lds_char* vb_off[2];
  {
    const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
    for (int d = 0; d < 2; ++d)
      vb_off[d] = lds + (FA7_ROW_BYTES * row + 16 * ((d * 2 + (p4 >> 1)) ^ fa7_swz(row)) + 8 * (p4 & 1));
  }

  stage(0, 0);
  // Q must be resident before the loop (llama_attn.hip): otherwise its pending loads are waited for behind the in-loop DMA
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int ks = 0; ks < FA7_KSTEPS; ++ks) asm volatile("" ::"v"(qf[qt][ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMAs of block 0 (hipcc does not count them)
  __syncthreads();

  auto block = [&](const int kb, auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    constexpr int KS = BUF * FA7_STAGE_BYTES, VS = KS + FA7_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, BUF ^ 1);
    if (wave_live && kb * FA7_KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T : st[qt][nt] rows = keys nt*16 + 4*quad + r, col = query li
      floatx4 st[QT][4];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
      typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
#pragma unroll
      for (int ks = 0; ks < FA7_KSTEPS; ++ks) {
        bf16x8 kf[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          kf[nt] = *reinterpret_cast<lds_bf16x8*>(kb_off + (KS + nt * 16 * FA7_ROW_BYTES + ks * 64));
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            st[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[nt], qf[qt][ks], st[qt][nt], 0, 0, 0);
      }

      // ---- online softmax (lane-local row), P packed as the B operand of O^T = V^T P^T
      bf16x8 pa[QT][2];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const bool diag = (kb * FA7_KB + FA7_KB - 1) > wave_q0 + qt * 16;   // the block needs masking (wave-uniform)
        if (diag) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key_u = kb * FA7_KB + nt * 16 + r - wave_q0 - qt * 16;
              st[qt][nt][r] = (key_u <= dq) ? st[qt][nt][r] : -__builtin_inff();
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
        // deferred maximum, decided per row: a row that keeps its reference multiplies by exactly 1
        if (__any(mx > mthr[qt])) {
          const float rmx = fa_max_xor16_32(mx);
          const bool grew = rmx > mthr[qt];
          const float m_new = grew ? rmx * sl2 : m_run[qt];
          const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);
#pragma unroll
          for (int r = 0; r < 4; ++r) l_acc[qt][r] *= alpha;
#pragma unroll
          for (int dt = 0; dt < FA7_DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[qt][dt][r] *= alpha;
          m_run[qt] = m_new;
          mthr[qt] = (m_new + FA7_DEFER) * inv_sl2;
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
        for (int dt = 0; dt < FA7_DT; ++dt) {
          const int o = VS + ks2 * 32 * FA7_ROW_BYTES + (dt >> 1) * 64;
          const short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt & 1] + o));
          const short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt & 1] + (o + 16 * FA7_ROW_BYTES)));
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
  // (2k, 2k+1) gives even quads d = 32 k + 8 (quad / 2) .. +7 and odd quads the same + 16: 16-byte stores, three per row and
  // lane. Every lane takes part in the swaps; only rows of this segment store. LASTQ: the 16 lane columns of wave 0 hold the
  // same row; column 0's four quads store its 96 dims.
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float inv = 1.0f / l_acc[qt][0];
    const int qabs = qabs_of(qt);
    const bool live = LASTQ ? (wave == 0 && li == 0) : (qabs < T && (!PREFIX || qabs >= P));
    int orow;
    if constexpr (LASTQ)
      orow = prompt;
    else if constexpr (PREFIX)
      orow = vtok0 + (live ? qabs : P);
    else
      orow = tok0 + (live ? qabs : 0);
    u16* op = out + (size_t)orow * nh * hd + h * hd + (quad & 1) * 16 + (quad >> 1) * 8;
#pragma unroll
    for (int k = 0; k < FA7_DT / 2; ++k) {
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

#endif
