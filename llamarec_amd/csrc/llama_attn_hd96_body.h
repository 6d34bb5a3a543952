// llama_attn_hd96_body.h -- the one text of the head_dim-96 MFMA attention (llama_attn_hd96.hip: read its header first),
// attn_hd96_body<LASTQ, PREFIX, LSE>, inlined into four kernels in three translation units:
//   <false, false, false>  attn_hd96_kernel, attention variant 7                        (llama_attn_hd96.hip)
//   <false, false, true>   attn_hd96_lse_kernel, variant 8's training forward: one lse store per row and head more
//                                                                                       (llama_attn_hd96_lse.hip)
//   <false, true, false>   attn_hd96_prefix_kernel<false>, shared prompt prefix          (llama_attn_hd96_prefix.hip)
//   <true, true, false>    attn_hd96_prefix_kernel<true>, one query row per prompt       (llama_attn_hd96_prefix.hip)
// Here stand the constants, the LDS layout with its swizzle and staging offsets, the QK product and the mask. The prologue,
// the staging of a block, the softmax steps and the store are lr_attn_body.h's, shared with head_dim 64 and 256; the PREFIX and
// LASTQ modes are described there. The backward is llama_attn_bwd_hd96.hip, which stages and reads its tiles by this layout.
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

#include "lr_attn_body.h"

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

__device__ __forceinline__ int fa7_swz(int row) { return (0 - (row >> 2)) & 3; }

// LSE (alone): lse[token][head] = natural-log log-sum-exp of the row's scaled scores.
template <bool LASTQ, bool PREFIX, bool LSE>
__device__ __forceinline__ void attn_hd96_body(const u16* qkv, u16* out, const int32_t* cu, int prefix_len, int nh, int nkv,
                                               int max_qblocks, int n_pairs, float* lse, const u16* q_rows_last) {
  static_assert(!LSE || (!PREFIX && !LASTQ), "the lse store exists without a shared prefix and for whole tiles only");
  static_assert(!LASTQ || PREFIX, "the last-row mode reads a shared prefix");
  constexpr int QT = LASTQ ? 1 : FA7_QT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int seg, h, qb;
  {   // (`pair` in a scope of its own, seg and h assigned: lr_attn_body.h on what keeps the whole-prompt kernels' code)
    int pair;
    fa_pair_of_workgroup<LASTQ>(n_pairs, max_qblocks, pair, qb);
    if (pair >= n_pairs) return;
    const FaSegHead sh = fa_segment_and_head(pair, nh);
    seg = sh.seg;
    h = sh.h;
    if constexpr (LASTQ) {
      if (prefix_len > 0 && seg == 0) return;   // segment 0 is the shared prefix, not a prompt
    } else {
      qb = __builtin_amdgcn_readfirstlane(qb);
    }
  }
  const FaSeg sg = fa_segment_rows<PREFIX>(cu, seg, prefix_len);
  const int P = sg.P, T = sg.T;
  // no query row of this segment in the tile
  if (!LASTQ && (qb * FA7_QROWS >= T || (PREFIX && (qb + 1) * FA7_QROWS <= P))) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const FaKV kv = fa_kv_bases<LASTQ, PREFIX, FA7_HD>(qkv, nh, nkv, kvh, sg);
  const int stride = kv.stride;
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
    const u16* qp = fa_q_ptr<LASTQ, PREFIX, FA7_HD>(qkv, q_rows_last, sg, stride, prompt, qabs_of(qt), nh, h, quad);
#pragma unroll
    for (int ks = 0; ks < FA7_KSTEPS; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }
  floatx4 ot[QT][FA7_DT];
  floatx4 l_acc[QT];
  float m_run[QT], mthr[QT];   // mthr = (m + FA_DEFER) / scale of the lane's row, in raw-score units
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < FA7_DT; ++dt) ot[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    l_acc[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
    m_run[qt] = -__builtin_inff();
    mthr[qt] = -__builtin_inff();
  }
  bf16x8 ones_f;   // (built here, not in a helper: attn_hd256_kernel<1> schedules one instruction elsewhere otherwise)
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = LASTQ ? T - 1 : min(qb * FA7_QROWS + FA7_QROWS - 1, T - 1);
  const int kb_last = q_last / FA7_KB;
  const int wave_q_last = LASTQ ? T - 1 : wave_q0 + 16 * QT - 1;
  // the wave owns at least one row of this segment (LASTQ: wave 0 computes, every wave stages)
  const bool wave_live = LASTQ ? wave == 0 : (wave_q0 < T && (!PREFIX || wave_q_last >= P));
  const float sl2 = 0.10206207261596575f * 1.4426950408889634f;  // 1/sqrt(96) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging (fa_stage_block): a tile is 12 pieces of 1 KiB (lane-linear in LDS: 64 chunks = 5 1/3 rows); wave w moves
  // pieces 3w .. 3w + 2 of K and of V, which are exactly rows 16 w .. 16 w + 15. Lane l of piece i writes linear chunk 64 i + l
  // of the wave's 192: row 16 w + (64 i + l) / 12 at position (64 i + l) % 12.
  unsigned soff[FA7_WAVE_PIECES];   // K and V alike: V's rows stand nkv hd elements behind K's, which the descriptors' bases carry
#pragma unroll
  for (int i = 0; i < FA7_WAVE_PIECES; ++i) {
    const int g = i * 64 + lane, r16 = g / FA7_ROW_CHUNKS, ppos = g - r16 * FA7_ROW_CHUNKS;
    const int row = wave * 16 + r16;
    soff[i] = (unsigned)(row * stride + (ppos ^ fa7_swz(row)) * 8) * 2u;
  }
  auto stage = [&](int kb, int buf) {
    fa_stage_block<PREFIX, FA7_HD, FA7_KB, FA7_WAVE_PIECES, FA7_TILE_BYTES>(
        smem + buf * FA7_STAGE_BYTES + wave * (FA7_WAVE_PIECES * 1024), kv, sg, kb, soff, soff,
        [=](int i) { return wave * 16 + (i * 64 + lane) / FA7_ROW_CHUNKS; });
  };

  // LDS read addresses, lane-dependent part computed once. K: row nt*16 + li, chunk 4 ks + quad: the swizzle touches bits 0-1,
  // so k-steps differ by an immediate of 64 B. V^T (transposed reads): row quad*4 + (li >> 2) (+16, +32, +48 per key
  // sub-block), dims 16 dt + 4 (li & 3): chunk 2 dt + ((li & 3) >> 1) with bits 0-1 swizzled by the row, so the d-tiles are
  // two addresses (dt even, dt odd) plus immediates of 64 B.
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
      // ---- S^T = K Q^T : st[qt][nt] rows = keys nt*16 + 4*quad + r, col = query li. The K fragments are loaded per k-step.
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

      // ---- online softmax (lane-local row)
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
        fa_rescale<FA7_DT>(fa_max16(st[qt]), sl2, inv_sl2, m_run[qt], mthr[qt], l_acc[qt], ot[qt]);
        fa_pack_p(st[qt], sl2, m_run[qt], pa[qt]);
      }
      // ---- O^T += V^T P^T
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) fa_row_sum(ones_f, pa[qt][ks2], l_acc[qt]);
#pragma unroll
        for (int dt = 0; dt < FA7_DT; ++dt) {
          const bf16x8 vf = fa_read_vt<FA7_ROW_BYTES>(vb_off[dt & 1] + (VS + ks2 * 32 * FA7_ROW_BYTES + (dt >> 1) * 64));
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

  // ---- normalise and store (fa_store_row): three 16-byte stores per row and lane
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float inv = 1.0f / l_acc[qt][0];
    const int qabs = qabs_of(qt);
    const bool live = fa_row_live<LASTQ, PREFIX>(sg, qabs, wave, li);
    if constexpr (LSE) {   // the lane's row: m (log2 units) + log2 l, as natural log; quad 0 of the row's lanes writes it
      if (live && quad == 0)
        lse[(size_t)(sg.tok0 + qabs) * nh + h] = (m_run[qt] + __builtin_amdgcn_logf(l_acc[qt][0])) * 0.6931471805599453f;
    }
    const int orow = fa_out_row<LASTQ, PREFIX>(sg, prompt, live, qabs);
    fa_store_row<FA7_DT>(ot[qt], inv, live, out + (size_t)orow * nh * FA7_HD + h * FA7_HD + (quad & 1) * 16 + (quad >> 1) * 8);
  }
}

#endif
