// llama_attn_hd128_body.h -- the one text of the head_dim-128 MFMA attention, attn_hd128_body<STAMP, LASTQ>, inlined into
// four kernels in two translation units:
//   <STAMP, false>  attn_mfma128_kernel<STAMP, false>, attention variant 2: whole prompts or a shared prefix   (llama_attn.hip)
//   <STAMP, true>   attn_mfma128_kernel<STAMP, true>, one query row per prompt                                  (llama_attn.hip)
//   <false, false>  attn_cached128_kernel<false>, query tiles over a user's K / V cache slot                    (llama_attn_cached.hip)
//   <false, true>   attn_cached128_kernel<true>, one query row per prompt over the slot                         (llama_attn_cached.hip)
// Here stands everything from the Q fragments to the store: the constants, the LDS layout with its swizzles, staging offsets
// and read addresses, the key-block loop unrolled by two, the QK product, the mask, the softmax, the PV product, normalise and
// store, lse, and the STAMP hooks. The softmax, row-sum, V-read and store steps are lr_attn_body.h's, shared with head_dim 64,
// 96 and 256. A kernel keeps what its source of rows decides: the prologue (workgroup -> segment, head, query tile, with its
// early returns), where the Q and output rows are (Fa128Src) and how a key block is staged (the `stage` it hands in).
// A row's bits are the same in all four because each runs these same lines on the same LDS image of a key block.
#ifndef LLAMA_ATTN_HD128_BODY_H
#define LLAMA_ATTN_HD128_BODY_H

#include "lr_attn_body.h"

#define FA_HD 128
#define FA_QROWS 128  // query rows per workgroup
#define FA_KB 64      // keys per block
#define FA_TILE_BYTES (FA_KB * 256)         // one K or V tile: 64 keys x 128 dims bf16
#define FA_STAGE_BYTES (2 * FA_TILE_BYTES)  // K tile + V tile
#define FA_LDS_BYTES (2 * FA_STAGE_BYTES)   // two stages: 64 KiB

__device__ __forceinline__ int v_off(int row, int ch) {  // dual-use swizzle, 256-byte rows
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// What a kernel's prologue hands the body. Positions count from the prompt's start; the segment owns positions P .. T - 1
// (keys [0, P) are the shared prefix's, or rows the cache held before this call), and the row of q, out and lse for position
// p >= P is row0 + p. LASTQ: row0 is the prompt's one row of q and out, the query is the one at position T - 1, qb is not read.
struct Fa128Src {
  int T, P, qb;        // sequence length, first owned position, query tile
  int h, nh;           // head, heads per row of out
  int kv_stride;       // elements per K / V row
  const u16* q;        // query rows, q_ld elements apart, head h at column h * 128
  int q_ld;
  u16* out;            // [rows][nh * 128]
  float* lse;          // optional [rows][nh] (whole tiles only)
  int row0;
};

// Diagnostic stamps: STAMP = true is instantiated only in a -DLR_EXPERIMENTS build (make EXPERIMENTS=1, then
// LR_ATTN_STAMPS=1 at run time; tools/attn_stamps.py); the product library holds no stamping code. s_memtime deltas
// of the key-block loop's segments summed over the loop, wave 0 of the first 64 workgroups (acc_out), and a per-workgroup
// timeline of the launch (wg_out; s_memrealtime, 100 MHz; tools/attn_wg_trace.py):
// entry | prologue done | key-block loop done | exit | HW_ID | XCC_ID | key blocks | blockIdx
// The kernel takes rt_entry and t_prev at its entry, in front of its prologue.
#define FA_WG_TRACE 8192
struct Fa128Stamps {
  unsigned long long rt_entry = 0, t_prev = 0;
  unsigned long long *acc_out = nullptr, *wg_out = nullptr;
};
#define FA_RT(dst)                                                                \
  if (STAMP) {                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                            \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(dst)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                            \
  }
#define FA_STAMP(slot)                                                         \
  if (STAMP) {                                                                 \
    unsigned long long t_;                                                     \
    __builtin_amdgcn_sched_barrier(0);                                         \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                         \
    stamp_acc[(slot)] += t_ - t_prev;                                          \
    t_prev = t_;                                                               \
  }

// Everything is computed transposed so that no cross-lane data movement is needed:
//   S^T = K Q^T   (A = K rows from LDS, B = Q rows held in registers)  -> lane owns ONE query
//                  row (lane&15) and 16 of the block's 64 keys: row max/sum = 2 shuffles
//   O^T = V^T P^T (A = V read with ds_read_b64_tr_b16 from the row-major LDS tile,
//                  B = P straight from the S^T accumulators, packed to bf16 in-lane)
//                  -> the O accumulator's column is again the lane's query row, so the
//                  online-softmax rescale is lane-local.
// A workgroup = 4 wave64 = 128 query rows of one (prompt, head); each wave 32 rows, so every K/V
// fragment read from LDS feeds two MFMA column tiles. K tile XOR-swizzled by (row&15) for
// ds_read_b128; V tile by the dual-use swizzle (row reads + transposed reads).
// LASTQ: wave 0 computes (every lane of the wave holds the same query row, so the tile arithmetic -- and with it the bits
// of that row -- is that of the tile mode) and all four waves stage.
// stage(kb, base, koff, voff): this wave's four K and four V pieces of key block kb to base + i * 1024 and
// base + FA_TILE_BYTES + i * 1024, by LDS-DMA.
template <bool STAMP, bool LASTQ, class Stage>
__device__ __forceinline__ void attn_hd128_body(const Fa128Src& src, Stage stage, const Fa128Stamps& sp) {
  unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_prev = sp.t_prev;
  unsigned long long rt_pro = 0, rt_loop = 0, rt_exit = 0;
  // [2 stages][K 16 KiB | V 16 KiB]; filled by LDS-DMA (lane-linear 1 KiB pieces = 4 rows x 256 B),
  // the XOR swizzles are applied to the SOURCE chunk: position p of row r holds chunk p ^ s(r).
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T = src.T, P = src.P, qb = src.qb, h = src.h, nh = src.nh, stride = src.kv_stride;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32*ks + 8*quad + 0..7
  bf16x8 qf[2][4];
  int qabs[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    qabs[qt] = LASTQ ? T - 1 : qb * FA_QROWS + wave * 32 + qt * 16 + li;
    const int qr = min(max(qabs[qt], P), T - 1);   // a clamped row is computed and not stored
    const u16* qp = src.q + (size_t)(LASTQ ? src.row0 : src.row0 + qr) * src.q_ld + h * FA_HD + quad * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }

  floatx4 ot[2][8];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) ot[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-__builtin_inff(), -__builtin_inff()};
  float mthr[2] = {-__builtin_inff(), -__builtin_inff()};   // (m + FA_DEFER) / scale of the lane's row, in raw-score units
  // Row sums of P through the matrix pipe (round 5): one more A row of ones beside V^T gives l = sum_k P[k][row] as an MFMA
  // accumulator -- every lane of a row's column holds the complete sum of the bf16 P the numerator uses -- instead of 16
  // v_add_f32 per half and block plus two cross-lane exchanges at the end (the block loop is bound by what a SIMD ISSUES: an
  // MFMA costs it ~8 cycles, 16 adds ~70).
  floatx4 l_acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
  bf16x8 ones_f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = min(qb * FA_QROWS + FA_QROWS - 1, T - 1);   // (LASTQ: qb is the tile of row T - 1, so this is T - 1)
  const int kb_last = q_last / FA_KB;
  const int wave_q_last = LASTQ ? T - 1 : qb * FA_QROWS + wave * 32 + 31;  // last query row this wave owns
  const float sl2 = 0.08838834764831845f * 1.4426950408889634f;  // 1/sqrt(128) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging: 16 pieces per tile (4 rows each); wave w moves pieces 4w..4w+3 of K and of V
  const int prow = lane >> 4, ppos = lane & 15;
  // per-lane byte offsets of this wave's 4 K pieces and 4 V pieces inside a key block (row and swizzled chunk are
  // block-invariant)
  unsigned koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 4 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ (row & 15)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ (((row & 3) << 2) | ((row >> 2) & 3))) * 8) * 2u;
  }
  auto stage_buf = [&](int kb, int buf) { stage(kb, smem + buf * FA_STAGE_BYTES + wave * 4096, koff, voff); };

  // LDS read addresses: everything lane-dependent is computed ONCE (4 K bases, 8 V bases); stage buffer, key sub-tile
  // and k-step are compile-time immediates of the ds_read (the key-block loop is unrolled by two so that the stage
  // buffer is one of them): no vector ALU between the MFMAs for addressing (was ~38 v_add / v_add3 per key block).
  lds_char* const lds = (lds_char*)smem;
  lds_char *kb_off[4], *vb_off[8];   // pointers, so that the LDS base is added here and not at every read
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kb_off[ks] = lds + (li * 256 + (((ks * 4 + quad) ^ li) << 4));   // row nt*16 + li: (row & 15) = li
  {
    const int qp = li >> 2, p4 = li & 3;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) vb_off[dt] = lds + (v_off(quad * 4 + qp, dt * 2 + (p4 >> 1)) + 8 * (p4 & 1));   // + 8192 ks2 + 4096 half
  }

  stage_buf(0, 0);
  // Q must be resident before the loop: otherwise hipcc carries its pending-load state into the loop
  // and waits for the in-loop DMA prefetch (vmcnt is in-order) in front of the first MFMAs.
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" ::"v"(qf[qt][ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMAs of block 0 (hipcc does not count them)
  __syncthreads();
  FA_STAMP(0)  // prologue: Q fragments + first K/V tile landed
  FA_RT(rt_pro)

  auto block = [&](const int kb, auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    constexpr int KS = BUF * FA_STAGE_BYTES, VS = KS + FA_TILE_BYTES;   // LDS byte offsets of this block's K and V tiles
    if (kb < kb_last) stage_buf(kb + 1, BUF ^ 1);
    FA_STAMP(1)  // DMA issue

    if (kb * FA_KB <= wave_q_last && wave_q_last >= P && (!LASTQ || wave == 0)) {  // otherwise every key of the block is masked for this wave
                                                          // (or none of its rows is the segment's own)
      // ---- S^T = K Q^T : st[qt][nt] rows = keys nt*16 + 4*quad + r, col = query li
      floatx4 st[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
      typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
      bf16x8 kf[2][4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) kf[0][nt] = *reinterpret_cast<lds_bf16x8*>(kb_off[0] + (KS + nt * 4096));
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < 3) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            kf[(ks + 1) & 1][nt] = *reinterpret_cast<lds_bf16x8*>(kb_off[ks + 1] + (KS + nt * 4096));
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            st[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks & 1][nt], qf[qt][ks], st[qt][nt], 0, 0, 0);
      }

      if (STAMP) asm volatile("" ::"v"(st[0][0]), "v"(st[1][3]));
      FA_STAMP(2)  // S^T = K Q^T
      // ---- online softmax (lane-local row), P packed as the B operand of O^T = V^T P^T
      bf16x8 pa[2][2];
      const bool diag = (kb * FA_KB + FA_KB - 1) > (LASTQ ? T - 1 : qb * FA_QROWS + wave * 32);  // block needs masking
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        if (diag) {  // a real (wave-uniform) branch: written as a select inside the loop below, hipcc predicates
                     // all 32 scores of every block -- ~100 wasted VALU instructions on the off-diagonal blocks
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kb * FA_KB + nt * 16 + quad * 4 + r;
              st[qt][nt][r] = (key <= qabs[qt]) ? st[qt][nt][r] : -__builtin_inff();
            }
          __builtin_amdgcn_sched_barrier(0);
        }
        // Raw-score row maximum (the scale is positive, so max commutes with it), then the deferred maximum (round 5, as in
        // llama_attn256.hip): a row's reference value m moves only when a score exceeds it by more than FA_DEFER in the exp2
        // domain, so P stays below 2^FA_DEFER (exact in fp32 sums, 8 significant bits in bf16 whatever its scale) and O / l are
        // rescaled in a tile's first block and then almost never -- with the running maximum some row of the 16 moved in most
        // blocks of a 600-1 100-token prompt (32 multiplies + an exp2 per half and block).
        // The decision is per row: a row's bits do not depend on its tile mates (alpha is exactly 1 for a row that keeps m).
        // Common path (fa_rescale): no lane of this half sees a score above its row's cached RAW threshold (m + FA_DEFER) / scale
        // -- one compare and a wave-uniform branch; the row maximum across the four lanes of a row, the new reference, alpha and
        // the rescale run only behind it (a row's own decision is the same either way: its maximum exceeds the threshold iff one
        // of its lanes' does -- the SAME predicate as the lanes' test, on the row maximum: a row moves iff one of its own lanes
        // asked for it, whatever the other rows of the wave do -- and a row that keeps m multiplies by exactly 1).
        fa_rescale<8>(fa_max16(st[qt]), sl2, inv_sl2, m_run[qt], mthr[qt], l_acc[qt], ot[qt]);
        fa_pack_p(st[qt], sl2, m_run[qt], pa[qt]);   // exp2(s*scale*log2e - m): one fma + one exp per score
      }

      if (STAMP) asm volatile("" ::"v"(pa[0][0]), "v"(pa[1][1]));
      FA_STAMP(3)  // softmax
      // ---- O^T += V^T P^T : A = V^T fragment via transposed LDS reads
      // V^T fragment rows: keys ks2*32 + quad*4 + qp (+16); their swizzle term ((row & 3) << 2 | (row >> 2) & 3) does not
      // depend on ks2 or the +16, so row0's address differs from vb_off[dt] by the immediate 8192 ks2 (+ 4096)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) fa_row_sum(ones_f, pa[qt][ks2], l_acc[qt]);
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
          const bf16x8 vf = fa_read_vt<256>(vb_off[dt] + (VS + ks2 * 8192));
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            ot[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa[qt][ks2], ot[qt][dt], 0, 0, 0);
        }
      }
    }
    if (STAMP) asm volatile("" ::"v"(ot[0][0]), "v"(ot[1][7]));
    FA_STAMP(4)  // O^T += V^T P^T
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of block kb + 1 have landed
    __syncthreads();  // ... and every wave is done with block kb
    FA_STAMP(5)  // barrier + DMA wait
  };
  for (int kb = 0; kb <= kb_last; kb += 2) {
    block(kb, std::integral_constant<int, 0>{});
    if (kb + 1 <= kb_last) block(kb + 1, std::integral_constant<int, 1>{});
  }

  FA_RT(rt_loop)
  // ---- normalise and store: lane owns query row li, d = dt*16 + 4*quad + r
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float l = l_acc[qt][0];   // (every register of the tile, in every lane of the row's column, holds the row's sum)
    const float inv = 1.0f / l;
    if (!LASTQ && qabs[qt] < T && qabs[qt] >= P && src.lse && quad == 0)  // natural-log log-sum-exp of the scaled scores (backward pass)
      src.lse[(size_t)(src.row0 + qabs[qt]) * nh + h] = (m_run[qt] + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
    // A lane holds d = 16 dt + 4 quad + r of its row: 8 bytes per tile. v_permlane16_swap (vdst rows 1 / 3 <-> src rows
    // 0 / 2 of 16 lanes) on the packed tiles (2k, 2k+1) leaves even quads with d = 8 (quad/2) .. +7 of tile 2k and odd
    // quads with the same of tile 2k + 1: 4 x 16-byte stores per row instead of 8 x 8 bytes (the tail is store-ISSUE
    // bound). Every lane takes part in the swaps (fa_store_row); only rows the segment owns store.
    const bool live = LASTQ ? (wave == 0 && qt == 0 && li == 0) : (qabs[qt] < T && qabs[qt] >= P);
    u16* op = src.out + (size_t)(LASTQ ? src.row0 : src.row0 + (live ? qabs[qt] : P)) * nh * FA_HD + h * FA_HD + (quad & 1) * 16 +
              (quad >> 1) * 8;
    fa_store_row<8>(ot[qt], inv, live, op);
  }
  if (STAMP) {
    FA_STAMP(6)  // epilogue
    const int wg = blockIdx.x;
    if (wg < 64 && tid == 0) {
      stamp_acc[7] = kb_last + 1;
#pragma unroll
      for (int i = 0; i < 8; ++i) sp.acc_out[wg * 8 + i] = stamp_acc[i];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the output stores have left
    FA_RT(rt_exit)
    if (wg < FA_WG_TRACE && tid == 0) {
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      unsigned long long* w = sp.wg_out + (size_t)wg * 8;
      w[0] = sp.rt_entry; w[1] = rt_pro; w[2] = rt_loop; w[3] = rt_exit; w[4] = hw; w[5] = xcc; w[6] = kb_last + 1; w[7] = wg;
    }
  }
}

#endif
