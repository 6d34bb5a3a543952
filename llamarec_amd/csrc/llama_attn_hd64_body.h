// llama_attn_hd64_body.h -- the one text of the head_dim-64 MFMA attention (llama_attn_hd64.hip: read its header first),
// attn_hd64_body<LASTQ, PREFIX, LSE>, inlined into four kernels in three translation units:
//   <false, false, false>  attn_hd64_kernel<false>, attention variant 5                          (llama_attn_hd64.hip)
//   <false, false, true>   attn_hd64_kernel<true>, variant 6's training forward: one lse store per row and head more
//                                                                                                (llama_attn_hd64_lse.hip)
//   <false, true, false>   attn_hd64_prefix_kernel<false>, shared prompt prefix                  (llama_attn_hd64_prefix.hip)
//   <true, true, false>    attn_hd64_prefix_kernel<true>, one query row per prompt               (llama_attn_hd64_prefix.hip)
// Here stand the constants, the LDS layout with its swizzles and staging offsets, the QK product and the mask. The prologue,
// the staging of a block, the softmax steps and the store are lr_attn_body.h's, shared with head_dim 96 and 256; the PREFIX and
// LASTQ modes are described there.
#ifndef LLAMA_ATTN_HD64_BODY_H
#define LLAMA_ATTN_HD64_BODY_H

#include "lr_attn_body.h"

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

// Swizzles on the 3-bit chunk index of a 128-byte row; the 16-byte bank slot of chunk position p of row r is 8 (r & 1) + p.
// K tile: position c ^ ((r >> 1) & 7). A ds_read_b128 lane group holds 16 rows distinct mod 16 at one chunk per quad: rows
//   of equal parity differ in (r >> 1) & 7, so the group covers all 16 slots.
// V tile: position c ^ (((r >> 1) & 3) << 1). A 32-lane half of a transposed read takes 8 rows x 32 B (chunks 2 dt, 2 dt + 1):
//   the four rows of equal parity land on four different chunk pairs. Bit 0 is untouched, so a row's 32 bytes stay in order.
// Both depend on row bits 1..3 only: sub-tiles 16 rows apart differ by an immediate.
__device__ __forceinline__ int fa5_kswz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int fa5_vswz(int row) { return ((row >> 1) & 3) << 1; }

// LSE (alone): lse[token][head] = natural-log log-sum-exp of the row's scaled scores.
template <bool LASTQ, bool PREFIX, bool LSE>
__device__ __forceinline__ void attn_hd64_body(const u16* qkv, u16* out, const int32_t* cu, int prefix_len, int nh, int nkv,
                                               int max_qblocks, int n_pairs, float* lse, const u16* q_rows_last) {
  static_assert(!LSE || (!PREFIX && !LASTQ), "the lse store exists without a shared prefix and for whole tiles only");
  static_assert(!LASTQ || PREFIX, "the last-row mode reads a shared prefix");
  constexpr int QT = LASTQ ? 1 : FA5_QT;
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
  if (!LASTQ && (qb * FA5_QROWS >= T || (PREFIX && (qb + 1) * FA5_QROWS <= P))) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const FaKV kv = fa_kv_bases<LASTQ, PREFIX, FA5_HD>(qkv, nh, nkv, kvh, sg);
  const int stride = kv.stride;
  const int prompt = prefix_len > 0 ? seg - 1 : seg;         // LASTQ: row of q_rows_last / out

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32 ks + 8 quad + 0..7
  const int wave_q0 = LASTQ ? T - 1 : qb * FA5_QROWS + wave * (16 * QT);
  bf16x8 qf[QT][2];
  int qabs[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qabs[qt] = LASTQ ? T - 1 : wave_q0 + qt * 16 + li;
    const u16* qp = fa_q_ptr<LASTQ, PREFIX, FA5_HD>(qkv, q_rows_last, sg, stride, prompt, qabs[qt], nh, h, quad);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }
  floatx4 ot[QT][4];
  floatx4 l_acc[QT];
  float m_run[QT], mthr[QT];   // mthr = (m + FA_DEFER) / scale of the lane's row, in raw-score units
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ot[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    l_acc[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
    m_run[qt] = -__builtin_inff();
    mthr[qt] = -__builtin_inff();
  }
  bf16x8 ones_f;   // (built here, not in a helper: attn_hd256_kernel<1> schedules one instruction elsewhere otherwise)
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = LASTQ ? T - 1 : min(qb * FA5_QROWS + FA5_QROWS - 1, T - 1);
  const int kb_last = q_last / FA5_KB;
  const int wave_q_last = LASTQ ? T - 1 : wave_q0 + 16 * QT - 1;
  // the wave owns at least one row of this segment (LASTQ: wave 0 computes, every wave stages)
  const bool wave_live = LASTQ ? wave == 0 : (wave_q0 < T && (!PREFIX || wave_q_last >= P));
  const float sl2 = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging (fa_stage_block): a tile is 8 pieces of 1 KiB (8 rows x 128 B); wave w moves pieces 2w, 2w + 1 of K and
  // of V.
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned koff[2], voff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wave * 2 + i) * 8 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ fa5_kswz(row)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ fa5_vswz(row)) * 8) * 2u;
  }
  auto stage = [&](int kb, int buf) {
    fa_stage_block<PREFIX, FA5_HD, FA5_KB, 2, FA5_TILE_BYTES>(smem + buf * FA5_STAGE_BYTES + wave * 2048, kv, sg, kb, koff, voff,
                                                              [=](int i) { return (wave * 2 + i) * 8 + prow; });
  };

  // LDS read addresses, lane-dependent part computed once. K: row nt*16 + li, chunk 4 ks + quad. V^T (transposed reads):
  // row quad*4 + (li >> 2) (+16, +32, +48 per key sub-block), dims 16 dt + 4 (li & 3).
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
      // ---- S^T = K Q^T : st[qt][nt] rows = keys nt*16 + 4*quad + r, col = query li. Every K fragment is loaded up front.
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

      // ---- online softmax (lane-local row)
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
        fa_rescale<4>(fa_max16(st[qt]), sl2, inv_sl2, m_run[qt], mthr[qt], l_acc[qt], ot[qt]);
        fa_pack_p(st[qt], sl2, m_run[qt], pa[qt]);
      }
      // ---- O^T += V^T P^T
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) fa_row_sum(ones_f, pa[qt][ks2], l_acc[qt]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 vf = fa_read_vt<FA5_ROW_BYTES>(vb_off[dt] + (VS + ks2 * 32 * FA5_ROW_BYTES));
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

  // ---- normalise and store (fa_store_row)
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float inv = 1.0f / l_acc[qt][0];
    const bool live = fa_row_live<LASTQ, PREFIX>(sg, qabs[qt], wave, li);
    if (LSE && live && quad == 0)   // the lane's row: m (log2 units) + log2 l, as natural log
      lse[(size_t)(sg.tok0 + qabs[qt]) * nh + h] = (m_run[qt] + __builtin_amdgcn_logf(l_acc[qt][0])) * 0.6931471805599453f;
    const int orow = fa_out_row<LASTQ, PREFIX>(sg, prompt, live, qabs[qt]);
    fa_store_row<4>(ot[qt], inv, live, out + (size_t)orow * nh * FA5_HD + h * FA5_HD + (quad & 1) * 16 + (quad >> 1) * 8);
  }
}

template <bool LSE>
__global__ __launch_bounds__(256, FA5_MIN_WG) void attn_hd64_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu, int nh,
                                                           int nkv, int max_qblocks, int n_pairs, float* lse) {
  attn_hd64_body<false, false, LSE>(qkv, out, cu, 0, nh, nkv, max_qblocks, n_pairs, lse, nullptr);
}

#endif
