// llama_attn_hd256_body.h -- the one text of the head_dim-256 MFMA attention (llama_attn_hd256.hip: read its header first),
// attn_hd256_body<HPW, LASTQ, PREFIX, SOFTCAP>, inlined into seven kernels in three translation units and one diagnostic build:
//   <1, false, false>  attn_hd256_kernel<1>, attention variant 4                                 (llama_attn_hd256.hip)
//   <2, false, false>  attn_hd256_kernel<2>, two heads of one KV head per workgroup: an A/B arm  (tools/diag/attn_hd256_mqa_ab.hip)
//   <1, false, true>   attn_hd256_prefix_kernel<false>, shared prompt prefix                     (llama_attn_hd256_prefix.hip)
//   <1, true, true>    attn_hd256_prefix_kernel<true>, one query row per prompt                  (llama_attn_hd256_prefix.hip)
//   the same three <1, ., ., true> with soft-capped scores (Gemma-2)                             (llama_attn_hd256_softcap.hip)
// The modes differ in where a K / V row and a query row live and in which rows a tile owns. Each such place picks its
// expression at compile time (`if constexpr`, or a condition on the template parameters alone): without PREFIX no shared-prefix
// length is ever computed, compared or added, so variant 4's instructions do not depend on the optimiser folding a zero away.
// The block walk, the masking, the per-row deferred maximum, bf16 P into both products and the ones-MFMA row sum are common to
// all of them, which is what makes a row's bits the same in every mode of one SOFTCAP setting.
#ifndef LLAMA_ATTN_HD256_BODY_H
#define LLAMA_ATTN_HD256_BODY_H

#include <type_traits>

#include "llama_kernels.h"
#include "lr_attn_util.h"
#include "lr_profile.h"

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

#define FA4_HD 256
#define FA4_WAVES 8                       // 16 query rows each
#define FA4_QR (16 * FA4_WAVES)           // query rows per workgroup with one head per workgroup
#define FA4_KB 64                         // keys per block
#define FA4_ROW_BYTES (FA4_HD * 2)        // one K or V row in LDS: 512 B = 32 chunks of 16 B
#define FA4_TILE_BYTES (FA4_KB * FA4_ROW_BYTES)   // 32 KiB
#define FA4_STAGE_BYTES (2 * FA4_TILE_BYTES)      // K tile + V tile
#define FA4_LDS_BYTES (2 * FA4_STAGE_BYTES)       // two stages: 128 KiB
#define FA4_DEFER 8.0f

// K tile: chunk c of row r sits at position c ^ (r & 15) (conflict-free ds_read_b128 of 16 rows at one chunk).
// V tile: the dual-use swizzle of variant 2, c ^ (((r & 3) << 2) | ((r >> 2) & 3)) (conflict-free transposed reads).
// Both flip the low 4 bits of the chunk index only, so a chunk stays in its 256-byte half of the row.
__device__ __forceinline__ int fa4_vswz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// HPW = heads per workgroup. 1: the 8 waves are 128 query rows of one head. 2 (MQA / GQA, two heads of one KV head): waves
//   0-3 are 64 rows of head 2p, waves 4-7 the same rows of head 2p + 1, both fed by one staged K/V tile (same reuse of the LDS
//   tile per stage, half-height causal tiles). A row's arithmetic is the same in both.
// PREFIX: prefix_len = P > 0 makes segment 0 of the packed rows the P tokens every prompt starts with and segment s >= 1 the
//   rest of prompt s - 1 at positions P.. . Keys and values of positions < P are read from segment 0's rows; query tiles and
//   64-key blocks stay aligned to positions inside the prompt, prefix included; rows of a tile at positions < P belong to
//   segment 0 and are neither computed nor stored for segment s. Without PREFIX prefix_len is not read.
// LASTQ (with PREFIX; prefix_len may be 0): `qkv` is the [rows][2 nkv hd] K | V projection, q_rows_last one rotated query row
//   per prompt. A workgroup = one (prompt, head) walks the prompt's key blocks, all eight waves staging and wave 0 computing
//   with every lane column holding the query at position T - 1; one output row per prompt.
// SOFTCAP (Gemma-2): the fp32 score s out of the MFMA becomes cap * tanh(s * scale / cap) before masking and the row maximum,
//   with scale and cap run-time values (without SOFTCAP neither is read: the scale is the compile-time 1/16). The capped score
//   is kept in the exp2 domain, y = cap log2(e) (1 - 2 / (1 + exp2(2 s scale log2(e) / cap))): a multiply, v_exp_f32, an add,
//   v_rcp_f32 and an fma per score. exp2 overflowing to +inf gives rcp = 0 and y = +cap log2(e), underflowing to 0 gives
//   -cap log2(e): no NaN at any finite s. The absolute error of the quotient form is ~1e-7 (one ulp of 1), times cap log2(e)
//   <= 1e-5 for cap 50, against a bf16 step of P of 2^-8. The running maximum stays (|y| <= cap log2(e) would allow a fixed
//   reference, but exp2(-2 cap log2(e)) is a denormal at cap 50 and can zero a row's sum).
template <int HPW, bool LASTQ, bool PREFIX, bool SOFTCAP = false>
__device__ __forceinline__ void attn_hd256_body(const u16* qkv, u16* out, const int32_t* cu, int prefix_len, int nh, int nkv,
                                                int max_qblocks, int n_pairs, const u16* q_rows_last, float scale = 0.f,
                                                float cap = 0.f) {
  static_assert(!SOFTCAP || HPW == 1, "soft-capped scores: one head per workgroup");
  static_assert(HPW == 1 || (HPW == 2 && !PREFIX && !LASTQ), "two heads per workgroup: whole tiles without a shared prefix only");
  static_assert(!LASTQ || PREFIX, "the last-row mode reads a shared prefix");
  constexpr int WPH = FA4_WAVES / HPW;   // waves per head
  constexpr int QR = 16 * WPH;           // query rows per head and workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hd = FA4_HD;
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
    const int hg = nh / HPW;   // head groups per prompt
    seg = __builtin_amdgcn_readfirstlane(pair / hg);
    h = __builtin_amdgcn_readfirstlane((pair - seg * hg) * HPW);   // first head of the group
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
  if (!LASTQ && (qb * QR >= T || (PREFIX && (qb + 1) * QR <= P))) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));   // (HPW = 2: both heads' KV head)
  h += wave / WPH;                                                      // this wave's head
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
  const int wave_q0 = LASTQ ? T - 1 : qb * QR + (wave % WPH) * 16;
  const int qabs = LASTQ ? T - 1 : wave_q0 + li;
  bf16x8 qf[8];
  {
    const u16* qp;
    if constexpr (LASTQ)
      qp = q_rows_last + (size_t)prompt * nh * hd + h * hd + quad * 8;
    else if constexpr (PREFIX)
      qp = qkv + (size_t)(vtok0 + min(max(qabs, P), T - 1)) * stride + h * hd + quad * 8;
    else
      qp = qkv + (size_t)(tok0 + min(qabs, T - 1)) * stride + h * hd + quad * 8;
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

  // ---- DMA staging: a tile is 32 pieces of 1 KiB (2 rows x 512 B, lane-linear in LDS); wave w moves pieces 4w..4w+3 of
  // K and of V. Rows past the prompt's end are range-checked to zero by the per-block buffer descriptor (those keys are
  // masked for every stored query row).
  const int prow = lane >> 5, ppos = lane & 31;
  unsigned koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 2 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ (row & 15)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ fa4_vswz(row)) * 8) * 2u;
  }
  // Where a block's rows live is what the modes differ in, so each has its staging text (as llama_attn_hd64_body.h). Without
  // PREFIX every block takes a per-block descriptor (scalar work only). PREFIX: so does a block that lies wholly in the
  // segment's own rows or wholly in segment 0; the one block that straddles position P takes one descriptor over the packed
  // rows [0, end of this segment] and a per-lane home offset (a compare, a select and an add per piece). The LDS image of a
  // block is the same bytes whatever the home of its rows, and the swizzles depend on the row inside the block and the chunk
  // only (derived, not measured with the conflict counter).
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * FA4_STAGE_BYTES + wave * 4096;
    if constexpr (!PREFIX) {
      const size_t blk_off = (size_t)kb * FA4_KB * stride * 2;
      const int records = ((T - 1 - kb * FA4_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
      const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
      const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa_dma16(rk, base + i * 1024, koff[i]);
        fa_dma16(rv, base + FA4_TILE_BYTES + i * 1024, voff[i]);
      }
    } else {
      const int k0 = kb * FA4_KB;
      if (k0 >= P || k0 + FA4_KB <= P) {   // the whole block has one home: the segment's own rows, or segment 0
        const bool own = k0 >= P;
        const size_t blk_off = (size_t)k0 * stride * 2;
        const int records = (((own ? T : P) - 1 - k0) * stride + hd) * 2;
        const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(own ? kbase : pkbase) + blk_off, records);
        const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(own ? vbase : pvbase) + blk_off, records);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fa_dma16(rk, base + i * 1024, koff[i]);
          fa_dma16(rv, base + FA4_TILE_BYTES + i * 1024, voff[i]);
        }
      } else {
        const unsigned records = ((unsigned)(vtok0 + T - 1) * (unsigned)stride + hd) * 2u;
        const fa_int4 rk = fa_make_rsrc(pkbase, (int)records);
        const fa_int4 rv = fa_make_rsrc(pvbase, (int)records);
        const unsigned home_pre = (unsigned)k0 * (unsigned)stride * 2u, home_own = (unsigned)(vtok0 + k0) * (unsigned)stride * 2u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = (wave * 4 + i) * 2 + prow;
          const unsigned home = (k0 + row < P) ? home_pre : home_own;
          fa_dma16(rk, base + i * 1024, koff[i] + home);
          fa_dma16(rv, base + FA4_TILE_BYTES + i * 1024, voff[i] + home);
        }
      }
    }
  };

  // LDS read addresses. K: row nt*16 + li, chunk 4 ks + quad (ks >= 4: the same position + 256 B). V^T (transposed reads):
  // row quad*4 + (li >> 2) (+16, +32, +48 per key sub-block), dims 16 dt + 4 (li & 3) (dt >= 8: + 256 B).
  typedef __attribute__((address_space(3))) char lds_char;
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
      // ---- S^T = K Q^T : st[nt] rows = keys nt*16 + 4*quad + r, col = query li
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
      // ---- online softmax (lane-local row), P packed as the B operand of O^T = V^T P^T
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
      float mx = fa_max3(st[0][0], st[0][1], st[0][2]);
      mx = fa_max3(mx, st[0][3], st[1][0]);
#pragma unroll
      for (int nt = 1; nt < 4; ++nt) {
        mx = fa_max3(mx, st[nt][1], st[nt][2]);
        if (nt < 3) mx = fa_max3(mx, st[nt][3], st[nt + 1][0]);
      }
      mx = fa_max2(mx, st[3][3]);
      // deferred maximum, decided per row (variant 2): a row that keeps its reference multiplies by exactly 1
      if (__any(mx > mthr)) {
        const float rmx = fa_max_xor16_32(mx);
        const bool grew = rmx > mthr;
        float m_new;   // SOFTCAP: the scores are in the exp2 domain already
        if constexpr (SOFTCAP) m_new = grew ? rmx : m_run;
        else m_new = grew ? rmx * sl2 : m_run;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
        for (int r = 0; r < 4; ++r) l_acc[r] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 16; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) ot[dt][r] *= alpha;
        m_run = m_new;
        if constexpr (SOFTCAP) mthr = m_new + FA4_DEFER;
        else mthr = (m_new + FA4_DEFER) * inv_sl2;
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (SOFTCAP) pa[nt >> 1][(nt & 1) * 4 + r] = (__bf16)__builtin_amdgcn_exp2f(st[nt][r] - m_run);
          else pa[nt >> 1][(nt & 1) * 4 + r] = (__bf16)__builtin_amdgcn_exp2f(__builtin_fmaf(st[nt][r], sl2, -m_run));
        }
      // ---- O^T += V^T P^T (k index 8 quad + j <-> key 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        l_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pa[ks2], l_acc, 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < 16; ++dt) {
          const int o = VS + ks2 * 32 * FA4_ROW_BYTES + (dt >> 3) * 256;
          const short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt & 7] + o));
          const short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt & 7] + (o + 16 * FA4_ROW_BYTES)));
          bf16x8 vf;
          const bf16x4 b0 = __builtin_bit_cast(bf16x4, t0), b1 = __builtin_bit_cast(bf16x4, t1);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            vf[r] = b0[r];
            vf[4 + r] = b1[r];
          }
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

  // ---- normalise and store: lane owns query row li, d = 16 dt + 4 quad + r. v_permlane16_swap on the packed tiles
  // (2k, 2k+1) gives even quads d = 32 k + 8 (quad / 2) .. +7 and odd quads the same + 16: 16-byte stores. Every lane
  // takes part in the swaps; only rows of this segment store. LASTQ: the 16 lane columns of wave 0 hold the same row;
  // column 0's four quads store its 256 dims.
  const float inv = 1.0f / l_acc[0];
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
  for (int k = 0; k < 8; ++k) {
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
