// llama_attn_hd64_body.h -- the kernel of llama_attn_hd64.hip (read its header first), as a template over LSE so that the
// two instantiations live in two translation units: <false> = attention variant 5 in llama_attn_hd64.hip, the code it was
// before the template; <true> = the training forward of variant 6 in llama_attn_hd64_lse.hip, the same code plus one lse
// store per row and head.
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

template <bool LSE>
__global__ __launch_bounds__(256, FA5_MIN_WG) void attn_hd64_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu, int nh,
                                                           int nkv, int max_qblocks, int n_pairs, float* lse) {
  constexpr int QT = FA5_QT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hd = FA5_HD;
  // workgroup -> (prompt, head, query tile): variant 2's order (a (prompt, head) pair per dispatch stream, heavy tiles first,
  // the two lightest tiles of every pair at the end of the launch)
  int seg, h, qb;
  {
    const int id = blockIdx.x, stream = id & 7, j = id >> 3;
    const int ppx = (n_pairs + 7) >> 3;
    const int n_light = min(max_qblocks, 2), n_heavy = max_qblocks - n_light;
    int pl;
    if (j < ppx * n_heavy) {
      pl = j / n_heavy;
      qb = max_qblocks - 1 - j % n_heavy;
    } else {
      const int j2 = j - ppx * n_heavy;
      pl = j2 / n_light;
      qb = n_light - 1 - j2 % n_light;
    }
    const int pair = pl * 8 + stream;
    if (pair >= n_pairs) return;
    seg = __builtin_amdgcn_readfirstlane(pair / nh);
    h = __builtin_amdgcn_readfirstlane(pair - seg * nh);
    qb = __builtin_amdgcn_readfirstlane(qb);
  }
  const int tok0 = cu[seg];
  const int T = cu[seg + 1] - tok0;
  if (qb * FA5_QROWS >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const int stride = (nh + 2 * nkv) * hd;
  const u16* kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
  const u16* vbase = kbase + nkv * hd;

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32 ks + 8 quad + 0..7
  const int wave_q0 = qb * FA5_QROWS + wave * (16 * QT);
  bf16x8 qf[QT][2];
  int qabs[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qabs[qt] = wave_q0 + qt * 16 + li;
    const u16* qp = qkv + (size_t)(tok0 + min(qabs[qt], T - 1)) * stride + h * hd + quad * 8;
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

  const int q_last = min(qb * FA5_QROWS + FA5_QROWS - 1, T - 1);
  const int kb_last = q_last / FA5_KB;
  const int wave_q_last = wave_q0 + 16 * QT - 1;
  const bool wave_live = wave_q0 < T;              // the wave owns at least one row of the prompt
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
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * FA5_STAGE_BYTES + wave * 2048;
    const size_t blk_off = (size_t)kb * FA5_KB * stride * 2;
    const int records = ((T - 1 - kb * FA5_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa_dma16(rk, base + i * 1024, koff[i]);
      fa_dma16(rv, base + FA5_TILE_BYTES + i * 1024, voff[i]);
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
  // takes part in the swaps; only rows of this prompt store.
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float inv = 1.0f / l_acc[qt][0];
    const bool live = qabs[qt] < T;
    if (LSE && live && quad == 0)   // the lane's row: m (log2 units) + log2 l, as natural log
      lse[(size_t)(tok0 + qabs[qt]) * nh + h] = (m_run[qt] + __builtin_amdgcn_logf(l_acc[qt][0])) * 0.6931471805599453f;
    u16* op = out + (size_t)(tok0 + (live ? qabs[qt] : 0)) * nh * hd + h * hd + (quad & 1) * 16 + (quad >> 1) * 8;
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

#endif
