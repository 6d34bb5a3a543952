// llama_attn_hd256_body.h -- the one text of the head_dim-256 MFMA attention (llama_attn_hd256.hip: read its header first),
// attn_hd256_body<HPW, LASTQ, PREFIX, SOFTCAP, LSE>, inlined into eight kernels in four translation units and one diagnostic
// build:
//   <1, false, false>  attn_hd256_kernel<1>, attention variant 4                                 (llama_attn_hd256.hip)
//   <1, false, false, false, true>  attn_hd256_lse_kernel, variant 9's training forward: one lse store per row and head more
//                                                                                                (llama_attn_hd256_lse.hip)
//   <2, false, false>  attn_hd256_kernel<2>, two heads of one KV head per workgroup: an A/B arm  (tools/diag/attn_hd256_mqa_ab.hip)
//   <1, false, true>   attn_hd256_prefix_kernel<false>, shared prompt prefix                     (llama_attn_hd256_prefix.hip)
//   <1, true, true>    attn_hd256_prefix_kernel<true>, one query row per prompt                  (llama_attn_hd256_prefix.hip)
//   the same three <1, ., ., true> with soft-capped scores (Gemma-2)                             (llama_attn_hd256_softcap.hip)
// Here stand the constants, the LDS layout with its swizzles and staging offsets, the QK product and the mask. The prologue,
// the staging of a block, the softmax steps and the store are lr_attn_body.h's, shared with head_dim 64 and 96; the PREFIX and
// LASTQ modes are described there, HPW and SOFTCAP below. A row's bits are the same in every mode of one SOFTCAP setting.
// The backward is llama_attn_bwd_hd256.hip, which has an LDS layout of its own (one swizzle for both kinds of read).
#ifndef LLAMA_ATTN_HD256_BODY_H
#define LLAMA_ATTN_HD256_BODY_H

#include "lr_attn_body.h"

#define FA4_HD 256
#define FA4_WAVES 8                       // 16 query rows each
#define FA4_QR (16 * FA4_WAVES)           // query rows per workgroup with one head per workgroup
#define FA4_KB 64                         // keys per block
#define FA4_ROW_BYTES (FA4_HD * 2)        // one K or V row in LDS: 512 B = 32 chunks of 16 B
#define FA4_TILE_BYTES (FA4_KB * FA4_ROW_BYTES)   // 32 KiB
#define FA4_STAGE_BYTES (2 * FA4_TILE_BYTES)      // K tile + V tile
#define FA4_LDS_BYTES (2 * FA4_STAGE_BYTES)       // two stages: 128 KiB

// K tile: chunk c of row r sits at position c ^ (r & 15) (conflict-free ds_read_b128 of 16 rows at one chunk).
// V tile: the dual-use swizzle of variant 2, c ^ (((r & 3) << 2) | ((r >> 2) & 3)) (conflict-free transposed reads).
// Both flip the low 4 bits of the chunk index only, so a chunk stays in its 256-byte half of the row; both depend on the row
// inside the block and the chunk only. Derived, and since measured with the conflict counter ("Training at
// head_dim 256"): SQ_LDS_BANK_CONFLICT is a third of SQ_LDS_IDX_ACTIVE in variant 4, which is the transposed V read being 2-way
// (a 32-lane half takes rows 8 m .. 8 m + 7, and rows r and r + 4 share a 32-byte slot under fa4_vswz); the K read is
// conflict-free. The backward's one swizzle ab9_swz (llama_attn_bwd_hd256.hip) measures 0 for both kinds of read; moving this
// V tile to it would change variant 4's instruction stream and has not been done.
__device__ __forceinline__ int fa4_vswz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// HPW = heads per workgroup. 1: the 8 waves are 128 query rows of one head. 2 (MQA / GQA, two heads of one KV head): waves
//   0-3 are 64 rows of head 2p, waves 4-7 the same rows of head 2p + 1, both fed by one staged K/V tile (same reuse of the LDS
//   tile per stage, half-height causal tiles). A row's arithmetic is the same in both.
// SOFTCAP (Gemma-2): the fp32 score s out of the MFMA becomes cap * tanh(s * scale / cap) before masking and the row maximum,
//   with scale and cap run-time values (without SOFTCAP neither is read: the scale is the compile-time 1/16). The capped score
//   is kept in the exp2 domain, y = cap log2(e) (1 - 2 / (1 + exp2(2 s scale log2(e) / cap))): a multiply, v_exp_f32, an add,
//   v_rcp_f32 and an fma per score. exp2 overflowing to +inf gives rcp = 0 and y = +cap log2(e), underflowing to 0 gives
//   -cap log2(e): no NaN at any finite s. The absolute error of the quotient form is ~1e-7 (one ulp of 1), times cap log2(e)
//   <= 1e-5 for cap 50, against a bf16 step of P of 2^-8. The running maximum stays (|y| <= cap log2(e) would allow a fixed
//   reference, but exp2(-2 cap log2(e)) is a denormal at cap 50 and can zero a row's sum). Scores in the exp2 domain take no
//   scale, so the capped rescale and P packing are fa_rescale and fa_pack_p without sl2, written out in the block loop: through
//   the helpers (with a SOFTCAP parameter, or with a scale of 1) attn_hd256_softcap_kernel orders two register moves in the
//   loop's preheader the other way round, and the whole-prompt kernels are held to the instruction stream they had.
// LSE (alone): lse[token][head] = natural-log log-sum-exp of the row's scaled scores; `lse` is read by no other mode.
template <int HPW, bool LASTQ, bool PREFIX, bool SOFTCAP = false, bool LSE = false>
__device__ __forceinline__ void attn_hd256_body(const u16* qkv, u16* out, const int32_t* cu, int prefix_len, int nh, int nkv,
                                                int max_qblocks, int n_pairs, const u16* q_rows_last, float scale = 0.f,
                                                float cap = 0.f, float* lse = nullptr) {
  static_assert(!LSE || (HPW == 1 && !PREFIX && !LASTQ && !SOFTCAP),
                "the lse store exists for whole tiles of one head without a shared prefix and without a soft cap only");
  static_assert(!SOFTCAP || HPW == 1, "soft-capped scores: one head per workgroup");
  static_assert(HPW == 1 || (HPW == 2 && !PREFIX && !LASTQ), "two heads per workgroup: whole tiles without a shared prefix only");
  static_assert(!LASTQ || PREFIX, "the last-row mode reads a shared prefix");
  constexpr int WPH = FA4_WAVES / HPW;   // waves per head
  constexpr int QR = 16 * WPH;           // query rows per head and workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int seg, h, qb;
  {   // (`pair` in a scope of its own, seg and h assigned: lr_attn_body.h on what keeps the whole-prompt kernels' code)
    int pair;
    fa_pair_of_workgroup<LASTQ>(n_pairs, max_qblocks, pair, qb);
    if (pair >= n_pairs) return;
    const FaSegHead sh = fa_segment_and_head(pair, nh / HPW);   // head groups per prompt
    seg = sh.seg;
    h = sh.h * HPW;   // first head of the group
    if constexpr (LASTQ) {
      if (prefix_len > 0 && seg == 0) return;   // segment 0 is the shared prefix, not a prompt
    } else {
      qb = __builtin_amdgcn_readfirstlane(qb);
    }
  }
  const FaSeg sg = fa_segment_rows<PREFIX>(cu, seg, prefix_len);
  const int P = sg.P, T = sg.T;
  // no query row of this segment in the tile
  if (!LASTQ && (qb * QR >= T || (PREFIX && (qb + 1) * QR <= P))) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));   // (HPW = 2: both heads' KV head)
  h += wave / WPH;                                                      // this wave's head
  const FaKV kv = fa_kv_bases<LASTQ, PREFIX, FA4_HD>(qkv, nh, nkv, kvh, sg);
  const int stride = kv.stride;
  const int prompt = prefix_len > 0 ? seg - 1 : seg;         // LASTQ: row of q_rows_last / out

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32 ks + 8 quad + 0..7
  const int wave_q0 = LASTQ ? T - 1 : qb * QR + (wave % WPH) * 16;
  const int qabs = LASTQ ? T - 1 : wave_q0 + li;
  bf16x8 qf[8];
  {
    const u16* qp = fa_q_ptr<LASTQ, PREFIX, FA4_HD>(qkv, q_rows_last, sg, stride, prompt, qabs, nh, h, quad);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }
  floatx4 ot[16];
#pragma unroll
  for (int dt = 0; dt < 16; ++dt) ot[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -__builtin_inff(), mthr = -__builtin_inff();
  floatx4 l_acc = floatx4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones_f;   // (built here, not in a helper: attn_hd256_kernel<1> schedules one instruction elsewhere otherwise)
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = LASTQ ? T - 1 : min(qb * QR + QR - 1, T - 1);
  const int kb_last = q_last / FA4_KB;
  const int wave_q_last = LASTQ ? T - 1 : wave_q0 + 15;
  // the wave owns at least one row of this segment (LASTQ: wave 0 computes, every wave stages)
  const bool wave_live = LASTQ ? wave == 0 : (wave_q0 < T && (!PREFIX || wave_q_last >= P));
  const float sl2 = 0.0625f * 1.4426950408889634f;  // 1/sqrt(256) * log2(e)
  const float inv_sl2 = 1.0f / sl2;
  // SOFTCAP: exp2 argument per raw score, and cap in the exp2 domain (wave-uniform; named by SOFTCAP expressions only)
  const float cap_a = SOFTCAP ? 2.0f * 1.4426950408889634f * scale / cap : 0.f;
  const float cap_l2 = SOFTCAP ? cap * 1.4426950408889634f : 0.f;

  // ---- DMA staging (fa_stage_block): a tile is 32 pieces of 1 KiB (2 rows x 512 B); wave w moves pieces 4w..4w+3 of K and
  // of V.
  const int prow = lane >> 5, ppos = lane & 31;
  unsigned koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 2 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ (row & 15)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ fa4_vswz(row)) * 8) * 2u;
  }
  auto stage = [&](int kb, int buf) {
    fa_stage_block<PREFIX, FA4_HD, FA4_KB, 4, FA4_TILE_BYTES>(smem + buf * FA4_STAGE_BYTES + wave * 4096, kv, sg, kb, koff, voff,
                                                              [=](int i) { return (wave * 4 + i) * 2 + prow; });
  };

  // LDS read addresses. K: row nt*16 + li, chunk 4 ks + quad (ks >= 4: the same position + 256 B). V^T (transposed reads):
  // row quad*4 + (li >> 2) (+16, +32, +48 per key sub-block), dims 16 dt + 4 (li & 3) (dt >= 8: + 256 B).
  lds_char* const lds = (lds_char*)smem;
  lds_char *kb_off[4], *vb_off[8];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kb_off[ks] = lds + (li * FA4_ROW_BYTES + (((ks * 4 + quad) ^ li) << 4));
  {
    const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      vb_off[dt] = lds + (FA4_ROW_BYTES * row + 16 * ((dt * 2 + (p4 >> 1)) ^ fa4_vswz(row)) + 8 * (p4 & 1));
  }

  stage(0, 0);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) asm volatile("" ::"v"(qf[ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMAs of block 0 (hipcc does not count them)
  __syncthreads();

  auto block = [&](const int kb, auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    constexpr int KS = BUF * FA4_STAGE_BYTES, VS = KS + FA4_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, BUF ^ 1);
    if (wave_live && kb * FA4_KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T : st[nt] rows = keys nt*16 + 4*quad + r, col = query li. The K fragments are double-buffered.
      floatx4 st[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) st[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
      typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
      bf16x8 kf[2][4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) kf[0][nt] = *reinterpret_cast<lds_bf16x8*>(kb_off[0] + (KS + nt * 16 * FA4_ROW_BYTES));
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks < 7) {
          const int kn = ks + 1;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            kf[kn & 1][nt] = *reinterpret_cast<lds_bf16x8*>(kb_off[kn & 3] + (KS + (kn >> 2) * 256 + nt * 16 * FA4_ROW_BYTES));
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks & 1][nt], qf[ks], st[nt], 0, 0, 0);
      }
      if constexpr (SOFTCAP) {   // st <- cap log2(e) tanh(st scale / cap), every key of the block (masking follows)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(st[nt][r] * cap_a);
            st[nt][r] = __builtin_fmaf(__builtin_amdgcn_rcpf(1.0f + e), -2.0f * cap_l2, cap_l2);
          }
      }
      // ---- online softmax (lane-local row)
      bf16x8 pa[2];
      const bool diag = (kb * FA4_KB + FA4_KB - 1) > wave_q0;   // the block needs masking (wave-uniform)
      if (diag) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kb * FA4_KB + nt * 16 + quad * 4 + r;
            st[nt][r] = (key <= qabs) ? st[nt][r] : -__builtin_inff();
          }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (!SOFTCAP) {
        fa_rescale<16>(fa_max16(st), sl2, inv_sl2, m_run, mthr, l_acc, ot);
        fa_pack_p(st, sl2, m_run, pa);
      } else {
        const float mx = fa_max16(st);
        if (__any(mx > mthr)) {
          const float rmx = fa_max_xor16_32(mx);
          const float m_new = rmx > mthr ? rmx : m_run;
          const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
          for (int r = 0; r < 4; ++r) l_acc[r] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 16; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[dt][r] *= alpha;
          m_run = m_new;
          mthr = m_new + FA_DEFER;
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) pa[nt >> 1][(nt & 1) * 4 + r] = (__bf16)__builtin_amdgcn_exp2f(st[nt][r] - m_run);
      }
      // ---- O^T += V^T P^T
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        fa_row_sum(ones_f, pa[ks2], l_acc);
#pragma unroll
        for (int dt = 0; dt < 16; ++dt) {
          const bf16x8 vf = fa_read_vt<FA4_ROW_BYTES>(vb_off[dt & 7] + (VS + ks2 * 32 * FA4_ROW_BYTES + (dt >> 3) * 256));
          ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa[ks2], ot[dt], 0, 0, 0);
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
  const float inv = 1.0f / l_acc[0];
  const bool live = fa_row_live<LASTQ, PREFIX>(sg, qabs, wave, li);
  if constexpr (LSE) {   // the lane's row: m (log2 units) + log2 l, as natural log; quad 0 of the row's lanes writes it
    if (live && quad == 0) lse[(size_t)(sg.tok0 + qabs) * nh + h] = (m_run + __builtin_amdgcn_logf(l_acc[0])) * 0.6931471805599453f;
  }
  const int orow = fa_out_row<LASTQ, PREFIX>(sg, prompt, live, qabs);
  fa_store_row<16>(ot, inv, live, out + (size_t)orow * nh * FA4_HD + h * FA4_HD + (quad & 1) * 16 + (quad >> 1) * 8);
}

#endif
