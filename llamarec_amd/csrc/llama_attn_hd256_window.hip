// llama_attn_hd256_window.hip -- the head_dim-256 MFMA attention with a sliding window (Gemma-3's local layers): query i sees
// keys j with i - W < j <= i, W a run-time value >= 1. A body of its own beside attn_hd256_body (llama_attn_hd256_body.h: read
// it first; constants, LDS layout, swizzles, staging offsets and the QK / PV products are the same lines), in a translation unit
// of its own, so that no existing instantiation of that body changes by an instruction. Two kernels:
//
//   attn_hd256_window_kernel        whole prompts, 128-row query tiles
//   attn_hd256_window_last_kernel   the pruned last layer, one query row per prompt (the LASTQ layout of lr_attn_body.h)
//
// What the window changes, against the causal walk:
//   first block   a tile whose first row is q0 starts at key block kb0 = max(0, q0 - W + 1) / 64 (last-row mode: the row is
//                 T - 1). The blocks in front of it are neither staged nor computed.
//   parity        the block loop alternates the two LDS stages by kb & 1 at compile time. Block kb0 is staged into stage
//                 kb0 & 1 and the loop starts at the even block kb0 & ~1, whose turn is skipped when it is kb0 - 1.
//   wave skip     a wave computes block kb only if it holds a key some row of the wave sees: kb * 64 <= wave_q_last (the causal
//                 test) and kb * 64 + 63 > wave_q0 - W (its last key is not in front of the first row's window).
//   lower edge    key > qabs - W per score, in the blocks that contain such a key (kb * 64 <= wave_q_last - W), in the same
//                 select as the causal edge.
//   masked rows   the rows of a 16-row wave tile start their windows in different blocks, so a row can meet blocks in which
//                 every one of its keys is masked BEFORE its first visible key (the causal kernel never does: key 0 is visible
//                 to every row). Such a row has m_run = -inf and scores of -inf only, and two expressions of the causal body
//                 then produce NaN: the rescale factor exp2(m_run - m_new) of a row that keeps its reference while a wave mate
//                 moves (-inf - -inf), and P = exp2(s * sl2 - m_run) (-inf + inf). Here a row that keeps its reference
//                 multiplies by the constant 1 (exactly what exp2(0) gives the causal kernel's rows), and P is formed against
//                 0 while the reference is -inf, which gives exp2(-inf) = 0: a wholly masked block adds +0 to the row's sum and
//                 to its output and leaves m_run at -inf, so it is an exact no-op for the row. The row's first visible key
//                 then moves the reference with a factor exp2(-inf) = 0 on accumulators that are still 0.
// Because a wholly masked block is an exact no-op for a row, a row's bits depend on its own window only, not on the tile it
// sits in: the last-row kernel (which starts at the last row's own first block) writes the bits the whole-prompt kernel writes
// for that row. Every stored row sees at least its own key, so l > 0 at the end. No lse, no shared prefix, no soft cap.
#include "llama_attn_hd256_body.h"

template <bool LASTQ>
__device__ __forceinline__ void attn_hd256_window_body(const u16* qkv, u16* out, const int32_t* cu, int nh, int nkv,
                                                       int max_qblocks, int n_pairs, const u16* q_rows_last, int window) {
  constexpr int QR = FA4_QR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int seg, h, qb;
  {
    int pair;
    fa_pair_of_workgroup<LASTQ>(n_pairs, max_qblocks, pair, qb);
    if (pair >= n_pairs) return;
    const FaSegHead sh = fa_segment_and_head(pair, nh);
    seg = sh.seg;
    h = sh.h;
    if constexpr (!LASTQ) qb = __builtin_amdgcn_readfirstlane(qb);
  }
  // LASTQ reads the K | V layout, which the helpers know under PREFIX (here with a prefix of 0 rows)
  const FaSeg sg = fa_segment_rows<LASTQ>(cu, seg, 0);
  const int T = sg.T, W = window;
  if (!LASTQ && qb * QR >= T) return;   // no query row of this segment in the tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const FaKV kv = fa_kv_bases<LASTQ, LASTQ, FA4_HD>(qkv, nh, nkv, kvh, sg);
  const int stride = kv.stride;

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32 ks + 8 quad + 0..7
  const int wave_q0 = LASTQ ? T - 1 : qb * QR + wave * 16;
  const int qabs = LASTQ ? T - 1 : wave_q0 + li;
  bf16x8 qf[8];
  {
    const u16* qp = fa_q_ptr<LASTQ, LASTQ, FA4_HD>(qkv, q_rows_last, sg, stride, seg, qabs, nh, h, quad);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }
  floatx4 ot[16];
#pragma unroll
  for (int dt = 0; dt < 16; ++dt) ot[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -__builtin_inff(), mthr = -__builtin_inff();
  floatx4 l_acc = floatx4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones_f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int tile_q0 = LASTQ ? T - 1 : qb * QR;
  const int q_last = LASTQ ? T - 1 : min(qb * QR + QR - 1, T - 1);
  const int kb_first = max(0, tile_q0 - W + 1) / FA4_KB;   // the block of the first key the tile's first row sees
  const int kb_last = q_last / FA4_KB;                     // kb_first <= tile_q0 / 64 <= kb_last
  const int wave_q_last = LASTQ ? T - 1 : wave_q0 + 15;
  const bool wave_live = LASTQ ? wave == 0 : wave_q0 < T;
  const float sl2 = 0.0625f * 1.4426950408889634f;  // 1/sqrt(256) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging (fa_stage_block), as attn_hd256_body
  const int prow = lane >> 5, ppos = lane & 31;
  unsigned koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 2 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ (row & 15)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ fa4_vswz(row)) * 8) * 2u;
  }
  auto stage = [&](int kb, int buf) {
    fa_stage_block<LASTQ, FA4_HD, FA4_KB, 4, FA4_TILE_BYTES>(smem + buf * FA4_STAGE_BYTES + wave * 4096, kv, sg, kb, koff, voff,
                                                             [=](int i) { return (wave * 4 + i) * 2 + prow; });
  };

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

  stage(kb_first, kb_first & 1);   // the stage block() reads block kb_first from
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) asm volatile("" ::"v"(qf[ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMAs of the first block (hipcc does not count them)
  __syncthreads();

  auto block = [&](const int kb, auto buf_c) {   // kb & 1 == BUF
    constexpr int BUF = decltype(buf_c)::value;
    constexpr int KS = BUF * FA4_STAGE_BYTES, VS = KS + FA4_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, BUF ^ 1);
    // some row of the wave sees a key of the block: not every key behind the last row, nor every key in front of the first
    // row's window
    if (wave_live && kb * FA4_KB <= wave_q_last && kb * FA4_KB + FA4_KB - 1 > wave_q0 - W) {
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
      // ---- both edges of the window, in the blocks that contain one (wave-uniform)
      const bool upper = (kb * FA4_KB + FA4_KB - 1) > wave_q0;    // a key behind some row
      const bool lower = kb * FA4_KB <= wave_q_last - W;          // a key in front of some row's window
      if (upper || lower) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kb * FA4_KB + nt * 16 + quad * 4 + r;
            st[nt][r] = (key <= qabs && key > qabs - W) ? st[nt][r] : -__builtin_inff();
          }
        __builtin_amdgcn_sched_barrier(0);
      }
      // ---- online softmax with the deferred maximum (fa_rescale), a row that keeps its reference multiplying by the constant 1
      const float mx = fa_max16(st);
      if (__any(mx > mthr)) {
        const float rmx = fa_max_xor16_32(mx);
        const bool grew = rmx > mthr;   // then rmx is finite: m_new is, and alpha = exp2(-inf) = 0 for a row's first key
        const float m_new = grew ? rmx * sl2 : m_run;
        const float alpha = grew ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) l_acc[r] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 16; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) ot[dt][r] *= alpha;
        m_run = m_new;
        mthr = (m_new + FA_DEFER) * inv_sl2;
      }
      // a row without a visible key so far (m_run = -inf, every score -inf): P = exp2(-inf - 0) = 0
      bf16x8 pa[2];
      fa_pack_p(st, sl2, m_run == -__builtin_inff() ? 0.f : m_run, pa);
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
  for (int kb = kb_first & ~1; kb <= kb_last; kb += 2) {
    if (kb >= kb_first) block(kb, std::integral_constant<int, 0>{});   // (false only in the first turn of an odd kb_first)
    if (kb + 1 <= kb_last) block(kb + 1, std::integral_constant<int, 1>{});
  }

  // ---- normalise and store (fa_store_row)
  const float inv = 1.0f / l_acc[0];
  const bool live = fa_row_live<LASTQ, LASTQ>(sg, qabs, wave, li);
  const int orow = fa_out_row<LASTQ, LASTQ>(sg, seg, live, qabs);
  fa_store_row<16>(ot, inv, live, out + (size_t)orow * nh * FA4_HD + h * FA4_HD + (quad & 1) * 16 + (quad >> 1) * 8);
}

__global__ __launch_bounds__(512, 1) void attn_hd256_window_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                                   int nh, int nkv, int max_qblocks, int n_pairs, int window) {
  attn_hd256_window_body<false>(qkv, out, cu, nh, nkv, max_qblocks, n_pairs, nullptr, window);
}

// (prefix_len: lr_attn_launch_last's argument list; always 0 here)
__global__ __launch_bounds__(512, 1) void attn_hd256_window_last_kernel(const u16* __restrict__ kv, u16* out, const int32_t* cu,
                                                                        int prefix_len, int nh, int nkv, int max_qblocks,
                                                                        int n_pairs, const u16* __restrict__ q_rows_last,
                                                                        int window) {
  attn_hd256_window_body<true>(kv, out, cu, nh, nkv, max_qblocks, n_pairs, q_rows_last, window);
}

// a.window >= 1, a.prefix_len == 0
int lr_launch_attention_hd256_window(const LrAttnArgs& a, hipStream_t st) {
  if (a.window < 1 || a.prefix_len != 0)
    LR_FAIL(a.window < 1 ? LR_EINVAL : LR_EUNSUPPORTED, "attention (window, head_dim 256): window %d, shared prefix %d (a window "
            ">= 1 and no shared prefix)", a.window, a.prefix_len);
  return lr_attn_launch_tiles<attn_hd256_window_kernel, FA4_HD, FA4_QR, 512, FA4_LDS_BYTES, false>(
      "attn_hd256_window_kernel", "windowed MFMA attention needs head_dim 256",
      "attention: the windowed head_dim-256 MFMA kernel writes no lse", nullptr, nullptr, a, st, a.window);
}

int lr_launch_attention_hd256_window_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu,
                                          const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int window, hipStream_t st) {
  if (window < 1) LR_FAIL(LR_EINVAL, "attention (window, last rows, head_dim 256): window %d", window);
  return lr_attn_launch_last<attn_hd256_window_last_kernel, FA4_HD, 512, FA4_LDS_BYTES>(
      "attn_hd256_window_last_kernel", "attention (window, last rows, head_dim 256)", kv, q_last, out_last, cu, cu_host, S, n_tok,
      nh, nkv, 0, st, window);
}
