// llama_attn_bwd_hd64.hip -- attention variant 6's backward: the two head_dim-128 passes of llama_attn_bwd.hip narrowed to
// head_dim 64 (Llama-3.2-1B / 3B LoRA fine-tuning), on v_mfma_f32_16x16x32_bf16, no atomics, one writer per element of dqkv.
//
// With P = exp(S - lse), D = rowsum(dO .* O) (lr_launch_rowdot):
//     dV = P^T dO,   dP = dO V^T,   dS = P .* (dP - D),   dQ = scale dS K,   dK = scale dS^T Q.
//  attn_bwd_hd64_dq_kernel  : a workgroup owns 128 query rows of one (prompt, head), a wave 32 of them; 64-key K and V tiles
//                 stream through LDS (LDS-DMA, two stages). Everything transposed: S^T = K Q^T and dP^T = V dO^T put a query
//                 row in a lane's accumulator column, so lse and D are one scalar per lane, and dS^T is, as it stands in the
//                 accumulators, the B operand of dQ^T += K^T dS^T (K^T through ds_read_b64_tr_b16 from the row-major tile).
//  attn_bwd_hd64_dkv_kernel : a workgroup owns 64 keys of one kv head, a wave 16 of them; it walks the query heads of its group
//                 and, for each, the 64-query blocks at or after its keys (Q and dO tiles by LDS-DMA, two stages):
//                 S = Q K^T, dP = dO V^T put a key in the accumulator column; P and dS are the B operands of
//                 dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T through transposed LDS reads).
// Rounding points are those of the head_dim-128 passes: fp32 scores, P = exp2(fma(s, scale log2 e, -lse log2 e)) in fp32,
// P and dS rounded to bf16 before the second product, fp32 accumulation, one bf16 rounding of the result; the inverse rotation
// (rope_cs given) acts on the fp32 accumulators. A prompt's gradient rows depend on that prompt only: tiles are aligned to
// positions inside the prompt, rows past its end are range-checked to zero by the tile's buffer descriptor, masked in P and
// never stored.
// Budget: dQ pass per lane Q^T 8 + dO^T 8 + dQ^T 32 + S^T 32 + dP^T 32 + dS 8 registers; dK/dV pass
// K 8 + V 8 + dK^T 16 + dV^T 16 + S 16 + dP 16 + P / dS 8. Both are held to 128 registers: four workgroups per CU.
// LDS: two stages of two 8 KiB tiles = 32 KiB (dK/dV: + 1 KiB of row statistics), 128 / 132 KiB of the CU's 160 at four.
#include "llama_train.h"
#include "lr_attn_util.h"
#include "lr_profile.h"

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef u16 u16x4 __attribute__((ext_vector_type(4)));

#define AB6_HD 64
#define AB6_KB 64                          // keys (dQ pass) / queries (dK/dV pass) per streamed block
#define AB6_ROW_BYTES (AB6_HD * 2)         // 128 B = 8 chunks of 16 B; two rows span the 64 banks
#define AB6_TILE_BYTES (AB6_KB * AB6_ROW_BYTES)   // 8 KiB
#define AB6_STAGE_BYTES (2 * AB6_TILE_BYTES)
#define AB6_QROWS 128                      // query rows per workgroup in the dQ pass
#define AB6_DQ_MIN_WG 4                    // workgroups per CU the dQ pass's registers are held to (<= 128)
#define AB6_DKV_MIN_WG 4                   // ... and the dK/dV pass's (<= 128)
#define AB6_SCALE 0.125f                   // 1 / sqrt(64)
#define AB6_LOG2E 1.4426950408889634f

// Dual-use swizzle on the 3-bit chunk index of a 128-byte row: chunk c of row r sits at position c ^ ab6_sw(r),
// ab6_sw(r) = ((r >> 1) & 3) << 1. The 16-byte bank slot (of 16) of position p of row r is 8 (r & 1) + p.
//  Row reads (ds_read_b128: lane (li, quad) takes row 16 t + li, chunk 4 ks + quad). The LDS serves 16 lanes per cycle, and
//   not 16 consecutive ones: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32. Such a group holds rows
//   li in {0..3, 12..15} at chunk c and rows li in {4..11} at chunk c ^ 1 (or the other way round). Bit 0 of the swizzle
//   is zero, so bit 0 of the position is bit 0 of the chunk: the two sets never meet. Inside a set, rows of equal parity are
//   {0, 2, 12, 14}, {1, 3, 13, 15}, {4, 6, 8, 10} or {5, 7, 9, 11}: (r >> 1) & 3 takes 0, 1, 2, 3 once in each, so the four
//   rows land on four different positions of their parity's half: all 16 slots, no conflict.
//  Transposed reads (ds_read_b64_tr_b16: 32 lanes per cycle, lane (li, quad) takes 8 bytes of row 4 quad + (li >> 2),
//   chunk 2 dt + ((li & 3) >> 1)). A 32-lane half holds 8 consecutive rows x 32 B, the chunk pair (2 dt, 2 dt + 1); the
//   32-byte slot (of 8) is 4 (r & 1) + ((2 dt ^ sw) >> 1) = 4 (r & 1) + (dt ^ ((r >> 1) & 3)): the four rows of equal parity
//   take four different pairs. The pair itself stays in order (bit 0 untouched).
//  It depends on row bits 1..2 only: sub-tiles 8, 16, 32 rows apart differ by an immediate offset.
// Derived from the bank rules of the microarchitecture notes; NOT confirmed with the LDS bank-conflict counter.
__device__ __forceinline__ int ab6_sw(int row) { return ((row >> 1) & 3) << 1; }

#define AB6_DMA_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

typedef __attribute__((address_space(3))) char ab6_lds_char;

// A operand = X^T fragment of a row-major LDS tile X[row][d] for the 16-dim tile dt and the 32-row step ks2:
// element e < 4: row 32 ks2 + 4 quad + e, e >= 4: row 32 ks2 + 16 + 4 quad + (e - 4); M index (lane & 15) = dim 16 dt + li.
// `p` = tile base + the lane's part (ab6_tr_off) + the dt part; rows 16 apart share the swizzle.
__device__ __forceinline__ int ab6_tr_off(int dt, int quad, int li) {
  const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
  return AB6_ROW_BYTES * row + 16 * ((dt * 2 + (p4 >> 1)) ^ ab6_sw(row)) + 8 * (p4 & 1);
}
__device__ __forceinline__ bf16x8 ab6_read_tr(const ab6_lds_char* p) {
  const short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(p));
  const short4v t1 =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(p + 16 * AB6_ROW_BYTES));
  const bf16x4 b0 = __builtin_bit_cast(bf16x4, t0), b1 = __builtin_bit_cast(bf16x4, t1);
  bf16x8 f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    f[r] = b0[r];
    f[4 + r] = b1[r];
  }
  return f;
}

// Optional epilogue: gradient w.r.t. the UNROTATED q / k. A lane holds dims 16 dt + 4 quad + 0..3 = rotation pairs
// i0 = 8 dt + 2 quad and i0 + 1 of its row (packed layout: pair (x1_i, x2_i) adjacent); 32 pairs per position.
__device__ __forceinline__ void ab6_unrotate(float (&v)[4], const float* rope_cs, int pos, int dt, int quad) {
  if (!rope_cs) return;
  const float4 cs = *reinterpret_cast<const float4*>(rope_cs + ((size_t)pos * (AB6_HD / 2) + dt * 8 + 2 * quad) * 2);
  const float a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
  v[0] = a0 * cs.x + a1 * cs.y;
  v[1] = a1 * cs.x - a0 * cs.y;
  v[2] = b0 * cs.z + b1 * cs.w;
  v[3] = b1 * cs.z - b0 * cs.w;
}

// ---------------------------------------------------------------------------------------------
// dQ pass
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, AB6_DQ_MIN_WG) void attn_bwd_hd64_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, int max_qblocks,
    const float* __restrict__ rope_cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][K tile | V tile]
  const int hd = AB6_HD;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qb = max_qblocks - 1 - (int)blockIdx.x;   // heavy tiles first
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (qb * AB6_QROWS >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = h / (nh / nkv);
  const int stride = (nh + 2 * nkv) * hd;
  const u16* kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
  const u16* vbase = kbase + nkv * hd;

  // ---- Q and dO fragments (B operands): row q, d = 32 ks + 8 quad + 0..7; lse and D of the lane's rows
  bf16x8 qf[2][2], dof[2][2];
  int qabs[2];
  float lse2[2], dq_row[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    qabs[qt] = qb * AB6_QROWS + wave * 32 + qt * 16 + li;
    const int qr = min(qabs[qt], T - 1);
    const u16* qp = qkv + (size_t)(tok0 + qr) * stride + h * hd + quad * 8;
    const u16* dp = d_out + (size_t)(tok0 + qr) * nh * hd + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
      dof[qt][ks] = *reinterpret_cast<const bf16x8*>(dp + ks * 32);
    }
    lse2[qt] = lse[(size_t)(tok0 + qr) * nh + h] * AB6_LOG2E;
    dq_row[qt] = dsum[(size_t)(tok0 + qr) * nh + h];
  }
  floatx4 dqt[2][4];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dqt[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int q_last = min(qb * AB6_QROWS + AB6_QROWS - 1, T - 1);
  const int kb_last = q_last / AB6_KB;
  const int wave_q0 = qb * AB6_QROWS + wave * 32;
  const int wave_q_last = wave_q0 + 31;
  const bool wave_live = wave_q0 < T;
  const float sl2 = AB6_SCALE * AB6_LOG2E;

  // ---- DMA staging: a tile is 8 pieces of 1 KiB (8 rows x 128 B, lane-linear in LDS); wave w moves pieces 2w, 2w + 1 of
  // K and of V. The swizzle is applied to the SOURCE chunk. Rows past the prompt's end are range-checked to zero by the
  // per-block buffer descriptor (those keys are masked for every query row of the prompt).
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned soff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wave * 2 + i) * 8 + prow;
    soff[i] = (unsigned)(row * stride + (ppos ^ ab6_sw(row)) * 8) * 2u;
  }
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * AB6_STAGE_BYTES + wave * 2048;
    const size_t blk_off = (size_t)kb * AB6_KB * stride * 2;
    const int records = ((T - 1 - kb * AB6_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa_dma16(rk, base + i * 1024, soff[i]);
      fa_dma16(rv, base + AB6_TILE_BYTES + i * 1024, soff[i]);
    }
  };
  // LDS read addresses, the lane's part computed once. Row reads: row 16 nt + li, chunk 4 ks + quad.
  ab6_lds_char* const lds = (ab6_lds_char*)smem;
  int row_off[2], tr_off[4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) row_off[ks] = li * AB6_ROW_BYTES + (((ks * 4 + quad) ^ ab6_sw(li)) << 4);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) tr_off[dt] = ab6_tr_off(dt, quad, li);

  stage(0, 0);
  // Q, dO and the statistics must be resident before the loop: otherwise their loads are waited for behind the in-loop DMA
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) asm volatile("" ::"v"(qf[qt][ks]), "v"(dof[qt][ks]));
    asm volatile("" ::"v"(lse2[qt]), "v"(dq_row[qt]));
  }
  AB6_DMA_LANDED();
  __syncthreads();

  typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
  for (int kb = 0; kb <= kb_last; ++kb) {
    const int KS = (kb & 1) * AB6_STAGE_BYTES, VS = KS + AB6_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, (kb + 1) & 1);
    if (wave_live && kb * AB6_KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T (rows = keys 16 nt + 4 quad + r, column = query li), then P^T in place
      floatx4 st[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 kf = *reinterpret_cast<lds_bf16x8*>(lds + (KS + nt * 16 * AB6_ROW_BYTES + row_off[ks]));
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            st[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][ks], st[qt][nt], 0, 0, 0);
        }
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kb * AB6_KB + nt * 16 + quad * 4 + r;
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qt][nt][r], sl2, -lse2[qt]));
            st[qt][nt][r] = (key <= qabs[qt] && qabs[qt] < T) ? p : 0.f;
          }
      // ---- dP^T = V dO^T
      floatx4 dpt[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) dpt[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 vf = *reinterpret_cast<lds_bf16x8*>(lds + (VS + nt * 16 * AB6_ROW_BYTES + row_off[ks]));
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            dpt[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[qt][ks], dpt[qt][nt], 0, 0, 0);
        }
      // ---- dS^T = P^T .* (dP^T - D), packed as the B operand of dQ^T += K^T dS^T
      // (k index 8 quad + j <-> key 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it)
      bf16x8 dsb[2][2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dsb[qt][nt >> 1][(nt & 1) * 4 + r] = (__bf16)(st[qt][nt][r] * (dpt[qt][nt][r] - dq_row[qt]));
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 kt = ab6_read_tr(lds + (KS + ks2 * 32 * AB6_ROW_BYTES + tr_off[dt]));
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            dqt[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, dsb[qt][ks2], dqt[qt][dt], 0, 0, 0);
        }
    }
    AB6_DMA_LANDED();   // this wave's pieces of block kb + 1
    __syncthreads();
  }
  // ---- store scale * dQ: lane owns query row li, d = 16 dt + 4 quad + r
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    if (qabs[qt] < T) {
      u16* op = dqkv + (size_t)(tok0 + qabs[qt]) * stride + h * hd + quad * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = dqt[qt][dt][r] * AB6_SCALE;
        ab6_unrotate(v, rope_cs, qabs[qt], dt, quad);
        u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(v[r]);
        *reinterpret_cast<u16x4*>(op + dt * 16) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// dK / dV pass
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, AB6_DKV_MIN_WG) void attn_bwd_hd64_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, const float* __restrict__ rope_cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][Q tile | dO tile], then the statistics
  float* stats = reinterpret_cast<float*>(smem + 2 * AB6_STAGE_BYTES);  // [2 stages][lse2[64] | D[64]]
  const int hd = AB6_HD;
  const int b = blockIdx.z, kvh = blockIdx.y, kb = blockIdx.x;
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (kb * AB6_KB >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int rep = nh / nkv;
  const int stride = (nh + 2 * nkv) * hd;
  const int ostride = nh * hd;

  // ---- this lane's key: K and V fragments (B operands), d = 32 ks + 8 quad + 0..7
  const int kabs = kb * AB6_KB + wave * 16 + li;
  const int kr = min(kabs, T - 1);
  bf16x8 kf[2], vf[2];
  {
    const u16* kp = qkv + (size_t)(tok0 + kr) * stride + (nh + kvh) * hd + quad * 8;
    const u16* vp = kp + nkv * hd;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8*>(kp + ks * 32);
      vf[ks] = *reinterpret_cast<const bf16x8*>(vp + ks * 32);
    }
  }
  floatx4 dkt[4], dvt[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dkt[dt] = dvt[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = AB6_SCALE * AB6_LOG2E;

  const int qb_first = kb, qb_last = (T - 1) / AB6_KB;
  const int nqb = qb_last - qb_first + 1;
  const int steps = nqb * rep;  // (query head of the group, query block) pairs, head-major
  // DMA staging as in the dQ pass: wave w moves pieces 2w, 2w + 1 of the Q tile (row stride of qkv) and of the dO tile
  // (row stride of d_out); rows past the prompt's end come back as zeros and are masked in P.
  const int prow = lane >> 3, ppos = lane & 7;
  unsigned qoff[2], ooff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wave * 2 + i) * 8 + prow;
    qoff[i] = (unsigned)(row * stride + (ppos ^ ab6_sw(row)) * 8) * 2u;
    ooff[i] = (unsigned)(row * ostride + (ppos ^ ab6_sw(row)) * 8) * 2u;
  }
  // a step's tiles are requested at the top of the step before (LDS-DMA) together with its 64 query rows' statistics
  // (ordinary loads into two registers of wave 0); the statistics are written to LDS at the END of that step, so that the
  // wait hipcc puts in front of the write coincides with the hand-written one for the DMA
  float st_l = 0.f, st_dd = 0.f;
  auto stage = [&](int step, int buf) {
    const int h = kvh * rep + step / nqb, qb = qb_first + step % nqb;
    char* base = smem + buf * AB6_STAGE_BYTES + wave * 2048;
    const int rows_left = T - 1 - qb * AB6_KB;
    const fa_int4 rq = fa_make_rsrc(
        reinterpret_cast<const char*>(qkv + (size_t)tok0 * stride + h * hd) + (size_t)qb * AB6_KB * stride * 2,
        (rows_left * stride + hd) * 2);
    const fa_int4 ro = fa_make_rsrc(
        reinterpret_cast<const char*>(d_out + (size_t)tok0 * ostride + h * hd) + (size_t)qb * AB6_KB * ostride * 2,
        (rows_left * ostride + hd) * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa_dma16(rq, base + i * 1024, qoff[i]);
      fa_dma16(ro, base + AB6_TILE_BYTES + i * 1024, ooff[i]);
    }
    if (tid < 64) {
      const int q = min(qb * AB6_KB + tid, T - 1);
      st_l = lse[(size_t)(tok0 + q) * nh + h];   // (first use of either value: commit_stats)
      st_dd = dsum[(size_t)(tok0 + q) * nh + h];
    }
  };
  auto commit_stats = [&](int buf) {
    __builtin_amdgcn_sched_barrier(0);
    if (tid < 64) {
      stats[buf * 128 + tid] = st_l * AB6_LOG2E;
      stats[buf * 128 + 64 + tid] = st_dd;
    }
  };
  ab6_lds_char* const lds = (ab6_lds_char*)smem;
  int row_off[2], tr_off[4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) row_off[ks] = li * AB6_ROW_BYTES + (((ks * 4 + quad) ^ ab6_sw(li)) << 4);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) tr_off[dt] = ab6_tr_off(dt, quad, li);

  stage(0, 0);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) asm volatile("" ::"v"(kf[ks]), "v"(vf[ks]));
  commit_stats(0);
  AB6_DMA_LANDED();
  __syncthreads();

  typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
  for (int step = 0; step < steps; ++step) {
    const int qb = qb_first + step % nqb;
    const int QS = (step & 1) * AB6_STAGE_BYTES, OS = QS + AB6_TILE_BYTES;
    const float* st_lse = stats + (step & 1) * 128;
    const float* st_d = st_lse + 64;
    if (step + 1 < steps) stage(step + 1, (step + 1) & 1);
    // ---- S = Q K^T and dP = dO V^T : rows = queries 16 mt + 4 quad + r, column = this lane's key
    floatx4 s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) s[mt] = dp[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 qa = *reinterpret_cast<lds_bf16x8*>(lds + (QS + mt * 16 * AB6_ROW_BYTES + row_off[ks]));
        const bf16x8 oa = *reinterpret_cast<lds_bf16x8*>(lds + (OS + mt * 16 * AB6_ROW_BYTES + row_off[ks]));
        s[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kf[ks], s[mt], 0, 0, 0);
        dp[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa, vf[ks], dp[mt], 0, 0, 0);
      }
    // ---- P and dS, packed as B operands (k index = query row)
    bf16x8 pb[2], dsb[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const floatx4 l4 = *reinterpret_cast<const floatx4*>(st_lse + mt * 16 + quad * 4);
      const floatx4 d4 = *reinterpret_cast<const floatx4*>(st_d + mt * 16 + quad * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = qb * AB6_KB + mt * 16 + quad * 4 + r;
        float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[mt][r], sl2, -l4[r]));
        p = (kabs <= q && q < T) ? p : 0.f;
        pb[mt >> 1][(mt & 1) * 4 + r] = (__bf16)p;
        dsb[mt >> 1][(mt & 1) * 4 + r] = (__bf16)(p * (dp[mt][r] - d4[r]));
      }
    }
    // ---- dV^T += dO^T P,  dK^T += Q^T dS
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8 ot = ab6_read_tr(lds + (OS + ks2 * 32 * AB6_ROW_BYTES + tr_off[dt]));
        const bf16x8 qt = ab6_read_tr(lds + (QS + ks2 * 32 * AB6_ROW_BYTES + tr_off[dt]));
        dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ot, pb[ks2], dvt[dt], 0, 0, 0);
        dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, dsb[ks2], dkt[dt], 0, 0, 0);
      }
    if (step + 1 < steps) commit_stats((step + 1) & 1);
    AB6_DMA_LANDED();   // this wave's pieces of step + 1
    __syncthreads();
  }
  if (kabs < T) {
    u16* kp = dqkv + (size_t)(tok0 + kabs) * stride + (nh + kvh) * hd + quad * 4;
    u16* vp = kp + nkv * hd;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      u16x4 ok, ov;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = dkt[dt][r] * AB6_SCALE;
      ab6_unrotate(v, rope_cs, kabs, dt, quad);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[r] = f2bf(v[r]);
        ov[r] = f2bf(dvt[dt][r]);
      }
      *reinterpret_cast<u16x4*>(kp + dt * 16) = ok;
      *reinterpret_cast<u16x4*>(vp + dt * 16) = ov;
    }
  }
}

// =============================================================================================
// dsum = rowsum(dO .* O) is already in place (lr_launch_attention_bwd); cu / cu_host: prompt starts [B + 1] in packed rows
int lr_launch_attention_bwd_hd64(const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv,
                                 const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd,
                                 hipStream_t st, const float* rope_cs) {
  if (hd != AB6_HD) LR_FAIL(LR_EUNSUPPORTED, "attention backward variant 6 needs head_dim 64 (got %d)", hd);
  int maxT = 0;
  for (int b = 0; b < B; ++b) maxT = max(maxT, cu_host[b + 1] - cu_host[b]);
  // the tiles come through buffer descriptors (32-bit byte offsets from a tile's first element)
  if ((long long)n_tok * (nh + 2 * nkv) * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward: packed qkv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  const int mq = (maxT + AB6_QROWS - 1) / AB6_QROWS, mk = (maxT + AB6_KB - 1) / AB6_KB;
  if (mq == 0) return LR_OK;
  if (nh > 65535 || nkv > 65535 || B > 65535)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward variant 6: %d heads / %d prompts exceed the grid limit", nh, B);
  static bool lds_set_dq[LR_MAX_DEVICES] = {}, lds_set_dkv[LR_MAX_DEVICES] = {};
  const int dkv_lds = 2 * AB6_STAGE_BYTES + 2 * 128 * (int)sizeof(float);
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_bwd_hd64_dq_kernel), 2 * AB6_STAGE_BYTES, lds_set_dq))
    return rc;
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_bwd_hd64_dkv_kernel), dkv_lds, lds_set_dkv))
    return rc;
  hipLaunchKernelGGL(attn_bwd_hd64_dq_kernel, dim3(mq, nh, B), dim3(256), 2 * AB6_STAGE_BYTES, st, qkv, d_out, lse, dsum,
                     dqkv, cu, nh, nkv, mq, rope_cs);
  LR_CHECK_LAUNCH("attn_bwd_hd64_dq_kernel");
  hipLaunchKernelGGL(attn_bwd_hd64_dkv_kernel, dim3(mk, nkv, B), dim3(256), dkv_lds, st, qkv, d_out, lse, dsum, dqkv, cu, nh,
                     nkv, rope_cs);
  LR_CHECK_LAUNCH("attn_bwd_hd64_dkv_kernel");
  return LR_OK;
}
