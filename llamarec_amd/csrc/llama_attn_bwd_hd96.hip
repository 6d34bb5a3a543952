// llama_attn_bwd_hd96.hip -- attention variant 8's backward: the two passes of llama_attn_bwd_hd64.hip widened to head_dim 96
// (LoRA fine-tuning of a Llama-format Phi-3-mini), on v_mfma_f32_16x16x32_bf16, no atomics, one writer per element of dqkv.
//
// With P = exp(S - lse), D = rowsum(dO .* O) (lr_launch_rowdot):
//     dV = P^T dO,   dP = dO V^T,   dS = P .* (dP - D),   dQ = scale dS K,   dK = scale dS^T Q.
//  attn_bwd_hd96_dq_kernel  : a workgroup owns 128 query rows of one (prompt, head), a wave 32 of them; 64-key K and V tiles
//                 (12 KiB each, rows of 192 B) stream through LDS (LDS-DMA, two stages). Everything transposed:
//                 S^T = K Q^T (3 k-steps) and dP^T = V dO^T put a query row in a lane's accumulator column, so lse and D are one
//                 scalar per lane, and dS^T is, as it stands in the accumulators, the B operand of dQ^T += K^T dS^T over 6
//                 d-tiles (K^T through ds_read_b64_tr_b16 from the row-major tile). dP^T is formed one 16-key tile at a time
//                 and turned into dS^T at once: 8 registers live instead of 32 (see the budget).
//  attn_bwd_hd96_dkv_kernel : a workgroup owns 64 keys of one kv head, a wave 16 of them; it walks the query heads of its group
//                 and, for each, the 64-query blocks at or after its keys (Q and dO tiles by LDS-DMA, two stages; the block's
//                 lse / D through LDS): S = Q K^T, dP = dO V^T put a key in the accumulator column; P and dS are the B operands
//                 of dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T through transposed LDS reads).
// Rounding points are those of the head_dim-64 / -128 passes: fp32 scores, P = exp2(fma(s, scale log2 e, -lse log2 e)) in fp32
// with scale = 96^-0.5 in fp32, P and dS rounded to bf16 before the second product, fp32 accumulation, one bf16 rounding of the
// result; the inverse rotation (rope_cs given) acts on the fp32 accumulators. A prompt's gradient rows depend on that prompt
// only: tiles are aligned to positions inside the prompt, rows past its end are range-checked to zero by the tile's buffer
// descriptor, masked in P and never stored.
//
// LDS layout and staging are the head_dim-96 forward's (llama_attn_hd96_body.h, derived there and confirmed with the
// bank-conflict counter): rows back to back at a 192-byte stride, chunk c of row r at position c ^ fa7_swz(r), a tile = 12
// lane-linear DMA pieces of 1 KiB, wave w moving pieces 3w .. 3w + 2 = rows 16w .. 16w + 15. That one swizzle was derived for
// BOTH kinds of read, which is what the backward needs, since each of its tiles is read both ways:
//  K (dQ pass), Q and dO (dK/dV pass), row-wise: ds_read_b128, lane (li, quad) takes row 16 t + li at chunk 4 ks + quad, t the
//    16-row sub-tile and ks the k-step -- the forward's K read, address for address (sub-tiles and k-steps are immediates).
//  K (dQ pass), Q and dO (dK/dV pass), transposed: ds_read_b64_tr_b16, lane (li, quad) takes 8 bytes of row 4 quad + (li >> 2)
//    (+ 16, and + 32 per 32-row step) at chunk 2 dt + ((li & 3) >> 1) -- the forward's V read, address for address.
//  V (dQ pass), row-wise: the forward reads V transposed only, but stages it with K's swizzle, so this is the K read on another
//    tile base (a multiple of 12 KiB = 192 slots of 64 B: the bank of an address is unchanged).
// The derivation speaks of rows and chunks inside a tile only; which tensor the bytes came from does not enter it.
//
// Budget: dQ pass per lane Q^T 12 + dO^T 12 + dQ^T 48 + S^T 32 + dP^T 8 (per 16-key tile) + dS 16
// registers; dK/dV pass K 12 + V 12 + dK^T 24 + dV^T 24 + S 16 + dP 16 + P / dS 8. Both are held to 168 registers: three
// workgroups per CU. LDS: two stages of two 12 KiB tiles = 48 KiB (dK/dV: + 1 KiB of row statistics), 144 / 147 KiB of the
// CU's 160 at three.
#include "llama_attn_hd96_body.h"
#include "llama_train.h"

typedef u16 u16x4 __attribute__((ext_vector_type(4)));

#define AB8_HD FA7_HD
#define AB8_KB FA7_KB                      // keys (dQ pass) / queries (dK/dV pass) per streamed block
#define AB8_KSTEPS FA7_KSTEPS              // 3 k-steps of 32 dims in S and dP
#define AB8_DT FA7_DT                      // 6 d-tiles of 16 in dQ, dK and dV
#define AB8_ROW_BYTES FA7_ROW_BYTES        // 192 B = 12 chunks of 16 B
#define AB8_TILE_BYTES FA7_TILE_BYTES      // 12 KiB = 12 DMA pieces of 1 KiB
#define AB8_STAGE_BYTES FA7_STAGE_BYTES    // two tiles
#define AB8_WAVE_PIECES FA7_WAVE_PIECES    // per wave and tile: three pieces = exactly 16 rows
#define AB8_QROWS 128                      // query rows per workgroup in the dQ pass
#define AB8_MIN_WG 3                       // workgroups per CU both passes' registers are held to (<= 168)
#define AB8_SCALE 0.10206207261596575f     // 1 / sqrt(96)
#define AB8_LOG2E 1.4426950408889634f

#define AB8_DMA_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

typedef __attribute__((address_space(3))) const bf16x8 ab8_lds_bf16x8;

// The lane's source byte offsets of its three DMA pieces inside a 64-row block whose rows are `stride` elements apart: lane l
// of piece i writes linear chunk 64 i + l of the wave's 192, row 16 w + (64 i + l) / 12 at position (64 i + l) % 12; the
// swizzle is applied to the SOURCE chunk.
__device__ __forceinline__ void ab8_piece_offsets(int wave, int lane, int stride, unsigned (&off)[AB8_WAVE_PIECES]) {
#pragma unroll
  for (int i = 0; i < AB8_WAVE_PIECES; ++i) {
    const int g = i * 64 + lane, r16 = g / FA7_ROW_CHUNKS, ppos = g - r16 * FA7_ROW_CHUNKS;
    const int row = wave * 16 + r16;
    off[i] = (unsigned)(row * stride + (ppos ^ fa7_swz(row)) * 8) * 2u;
  }
}
// Row reads: row 16 t + li, chunk 4 ks + quad; the swizzle touches chunk bits 0-1, so k-steps differ by an immediate of 64 B
// and sub-tiles by 16 rows.
__device__ __forceinline__ int ab8_row_off(int quad, int li) { return li * AB8_ROW_BYTES + ((quad ^ fa7_swz(li)) << 4); }
// A operand = X^T fragment of a row-major LDS tile X[row][d] for the 16-dim tile dt and the 32-row step ks2 (fa_read_vt):
// element e < 4: row 32 ks2 + 4 quad + e, e >= 4: the same + 16; M index (lane & 15) = dim 16 dt + li. The lane's address for
// d-tile dt is tr_off[dt & 1] + 64 (dt >> 1): chunk 2 dt + ((li & 3) >> 1) with bits 0-1 swizzled by the row.
__device__ __forceinline__ void ab8_tr_offsets(int quad, int li, int (&off)[2]) {
  const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
  for (int d = 0; d < 2; ++d) off[d] = AB8_ROW_BYTES * row + 16 * ((d * 2 + (p4 >> 1)) ^ fa7_swz(row)) + 8 * (p4 & 1);
}

// Optional epilogue: gradient w.r.t. the UNROTATED q / k. A lane holds dims 16 dt + 4 quad + 0..3 = rotation pairs
// i0 = 8 dt + 2 quad and i0 + 1 of its row (packed layout: pair (x1_i, x2_i) adjacent); 48 pairs per position, so the two
// pairs are one aligned float4 of the table.
__device__ __forceinline__ void ab8_unrotate(float (&v)[4], const float* rope_cs, int pos, int dt, int quad) {
  if (!rope_cs) return;
  const float4 cs = *reinterpret_cast<const float4*>(rope_cs + ((size_t)pos * (AB8_HD / 2) + dt * 8 + 2 * quad) * 2);
  const float a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
  v[0] = a0 * cs.x + a1 * cs.y;
  v[1] = a1 * cs.x - a0 * cs.y;
  v[2] = b0 * cs.z + b1 * cs.w;
  v[3] = b1 * cs.z - b0 * cs.w;
}

// ---------------------------------------------------------------------------------------------
// dQ pass
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, AB8_MIN_WG) void attn_bwd_hd96_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, int max_qblocks,
    const float* __restrict__ rope_cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][K tile | V tile]
  const int hd = AB8_HD;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qb = max_qblocks - 1 - (int)blockIdx.x;   // heavy tiles first
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (qb * AB8_QROWS >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = h / (nh / nkv);
  const int stride = (nh + 2 * nkv) * hd;
  const u16* kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
  const u16* vbase = kbase + nkv * hd;

  // ---- Q and dO fragments (B operands): row q, d = 32 ks + 8 quad + 0..7; lse and D of the lane's rows
  bf16x8 qf[2][AB8_KSTEPS], dof[2][AB8_KSTEPS];
  int qabs[2];
  float lse2[2], dq_row[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    qabs[qt] = qb * AB8_QROWS + wave * 32 + qt * 16 + li;
    const int qr = min(qabs[qt], T - 1);
    const u16* qp = qkv + (size_t)(tok0 + qr) * stride + h * hd + quad * 8;
    const u16* dp = d_out + (size_t)(tok0 + qr) * nh * hd + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < AB8_KSTEPS; ++ks) {
      qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
      dof[qt][ks] = *reinterpret_cast<const bf16x8*>(dp + ks * 32);
    }
    lse2[qt] = lse[(size_t)(tok0 + qr) * nh + h] * AB8_LOG2E;
    dq_row[qt] = dsum[(size_t)(tok0 + qr) * nh + h];
  }
  floatx4 dqt[2][AB8_DT];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < AB8_DT; ++dt) dqt[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int q_last = min(qb * AB8_QROWS + AB8_QROWS - 1, T - 1);
  const int kb_last = q_last / AB8_KB;
  const int wave_q0 = qb * AB8_QROWS + wave * 32;
  const int wave_q_last = wave_q0 + 31;
  const bool wave_live = wave_q0 < T;
  const float sl2 = AB8_SCALE * AB8_LOG2E;

  // ---- DMA staging: wave w moves pieces 3w .. 3w + 2 of K and of V (V's rows stand nkv hd elements behind K's, which the
  // descriptors' bases carry). Rows past the prompt's end are range-checked to zero by the per-block buffer descriptor (those
  // keys are masked for every query row of the prompt).
  unsigned soff[AB8_WAVE_PIECES];
  ab8_piece_offsets(wave, lane, stride, soff);
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * AB8_STAGE_BYTES + wave * (AB8_WAVE_PIECES * 1024);
    const size_t blk_off = (size_t)kb * AB8_KB * stride * 2;
    const int records = ((T - 1 - kb * AB8_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < AB8_WAVE_PIECES; ++i) {
      fa_dma16(rk, base + i * 1024, soff[i]);
      fa_dma16(rv, base + AB8_TILE_BYTES + i * 1024, soff[i]);
    }
  };
  // LDS read addresses, the lane's part computed once
  lds_char* const lds = (lds_char*)smem;
  const int row_off = ab8_row_off(quad, li);
  int tr_off[2];
  ab8_tr_offsets(quad, li, tr_off);

  stage(0, 0);
  // Q, dO and the statistics must be resident before the loop: otherwise their loads are waited for behind the in-loop DMA
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int ks = 0; ks < AB8_KSTEPS; ++ks) asm volatile("" ::"v"(qf[qt][ks]), "v"(dof[qt][ks]));
    asm volatile("" ::"v"(lse2[qt]), "v"(dq_row[qt]));
  }
  AB8_DMA_LANDED();
  __syncthreads();

  for (int kb = 0; kb <= kb_last; ++kb) {
    const int KS = (kb & 1) * AB8_STAGE_BYTES, VS = KS + AB8_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, (kb + 1) & 1);
    if (wave_live && kb * AB8_KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T (rows = keys 16 nt + 4 quad + r, column = query li), then P^T in place
      floatx4 st[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < AB8_KSTEPS; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 kf = *reinterpret_cast<ab8_lds_bf16x8*>(lds + (KS + nt * 16 * AB8_ROW_BYTES + ks * 64 + row_off));
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
            const int key = kb * AB8_KB + nt * 16 + quad * 4 + r;
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qt][nt][r], sl2, -lse2[qt]));
            st[qt][nt][r] = (key <= qabs[qt] && qabs[qt] < T) ? p : 0.f;
          }
      // ---- dP^T = V dO^T, one 16-key tile at a time, and dS^T = P^T .* (dP^T - D) from it at once, packed as the B operand of
      // dQ^T += K^T dS^T (k index 8 quad + j <-> key 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it)
      bf16x8 dsb[2][2];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        floatx4 dpt[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < AB8_KSTEPS; ++ks) {
          const bf16x8 vf = *reinterpret_cast<ab8_lds_bf16x8*>(lds + (VS + nt * 16 * AB8_ROW_BYTES + ks * 64 + row_off));
#pragma unroll
          for (int qt = 0; qt < 2; ++qt) dpt[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[qt][ks], dpt[qt], 0, 0, 0);
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dsb[qt][nt >> 1][(nt & 1) * 4 + r] = (__bf16)(st[qt][nt][r] * (dpt[qt][r] - dq_row[qt]));
      }
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
        for (int dt = 0; dt < AB8_DT; ++dt) {
          const bf16x8 kt =
              fa_read_vt<AB8_ROW_BYTES>(lds + (KS + ks2 * 32 * AB8_ROW_BYTES + (dt >> 1) * 64 + tr_off[dt & 1]));
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            dqt[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, dsb[qt][ks2], dqt[qt][dt], 0, 0, 0);
        }
    }
    AB8_DMA_LANDED();   // this wave's pieces of block kb + 1
    __syncthreads();
  }
  // ---- store scale * dQ: lane owns query row li, d = 16 dt + 4 quad + r
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    if (qabs[qt] < T) {
      u16* op = dqkv + (size_t)(tok0 + qabs[qt]) * stride + h * hd + quad * 4;
#pragma unroll
      for (int dt = 0; dt < AB8_DT; ++dt) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = dqt[qt][dt][r] * AB8_SCALE;
        ab8_unrotate(v, rope_cs, qabs[qt], dt, quad);
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
__global__ __launch_bounds__(256, AB8_MIN_WG) void attn_bwd_hd96_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, const float* __restrict__ rope_cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][Q tile | dO tile], then the statistics
  float* stats = reinterpret_cast<float*>(smem + 2 * AB8_STAGE_BYTES);  // [2 stages][lse2[64] | D[64]]
  const int hd = AB8_HD;
  const int b = blockIdx.z, kvh = blockIdx.y, kb = blockIdx.x;
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (kb * AB8_KB >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int rep = nh / nkv;
  const int stride = (nh + 2 * nkv) * hd;
  const int ostride = nh * hd;

  // ---- this lane's key: K and V fragments (B operands), d = 32 ks + 8 quad + 0..7
  const int kabs = kb * AB8_KB + wave * 16 + li;
  const int kr = min(kabs, T - 1);
  bf16x8 kf[AB8_KSTEPS], vf[AB8_KSTEPS];
  {
    const u16* kp = qkv + (size_t)(tok0 + kr) * stride + (nh + kvh) * hd + quad * 8;
    const u16* vp = kp + nkv * hd;
#pragma unroll
    for (int ks = 0; ks < AB8_KSTEPS; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8*>(kp + ks * 32);
      vf[ks] = *reinterpret_cast<const bf16x8*>(vp + ks * 32);
    }
  }
  floatx4 dkt[AB8_DT], dvt[AB8_DT];
#pragma unroll
  for (int dt = 0; dt < AB8_DT; ++dt) dkt[dt] = dvt[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = AB8_SCALE * AB8_LOG2E;

  const int qb_first = kb, qb_last = (T - 1) / AB8_KB;
  const int nqb = qb_last - qb_first + 1;
  const int steps = nqb * rep;  // (query head of the group, query block) pairs, head-major
  // DMA staging as in the dQ pass: wave w moves pieces 3w .. 3w + 2 of the Q tile (row stride of qkv) and of the dO tile
  // (row stride of d_out); rows past the prompt's end come back as zeros and are masked in P.
  unsigned qoff[AB8_WAVE_PIECES], ooff[AB8_WAVE_PIECES];
  ab8_piece_offsets(wave, lane, stride, qoff);
  ab8_piece_offsets(wave, lane, ostride, ooff);
  // a step's tiles are requested at the top of the step before (LDS-DMA) together with its 64 query rows' statistics
  // (ordinary loads into two registers of wave 0); the statistics are written to LDS at the END of that step, so that the
  // wait hipcc puts in front of the write coincides with the hand-written one for the DMA
  float st_l = 0.f, st_dd = 0.f;
  auto stage = [&](int step, int buf) {
    const int h = kvh * rep + step / nqb, qb = qb_first + step % nqb;
    char* base = smem + buf * AB8_STAGE_BYTES + wave * (AB8_WAVE_PIECES * 1024);
    const int rows_left = T - 1 - qb * AB8_KB;
    const fa_int4 rq = fa_make_rsrc(
        reinterpret_cast<const char*>(qkv + (size_t)tok0 * stride + h * hd) + (size_t)qb * AB8_KB * stride * 2,
        (rows_left * stride + hd) * 2);
    const fa_int4 ro = fa_make_rsrc(
        reinterpret_cast<const char*>(d_out + (size_t)tok0 * ostride + h * hd) + (size_t)qb * AB8_KB * ostride * 2,
        (rows_left * ostride + hd) * 2);
#pragma unroll
    for (int i = 0; i < AB8_WAVE_PIECES; ++i) {
      fa_dma16(rq, base + i * 1024, qoff[i]);
      fa_dma16(ro, base + AB8_TILE_BYTES + i * 1024, ooff[i]);
    }
    if (tid < 64) {
      const int q = min(qb * AB8_KB + tid, T - 1);
      st_l = lse[(size_t)(tok0 + q) * nh + h];   // (first use of either value: commit_stats)
      st_dd = dsum[(size_t)(tok0 + q) * nh + h];
    }
  };
  auto commit_stats = [&](int buf) {
    __builtin_amdgcn_sched_barrier(0);
    if (tid < 64) {
      stats[buf * 128 + tid] = st_l * AB8_LOG2E;
      stats[buf * 128 + 64 + tid] = st_dd;
    }
  };
  lds_char* const lds = (lds_char*)smem;
  const int row_off = ab8_row_off(quad, li);
  int tr_off[2];
  ab8_tr_offsets(quad, li, tr_off);

  stage(0, 0);
#pragma unroll
  for (int ks = 0; ks < AB8_KSTEPS; ++ks) asm volatile("" ::"v"(kf[ks]), "v"(vf[ks]));
  commit_stats(0);
  AB8_DMA_LANDED();
  __syncthreads();

  for (int step = 0; step < steps; ++step) {
    const int qb = qb_first + step % nqb;
    const int QS = (step & 1) * AB8_STAGE_BYTES, OS = QS + AB8_TILE_BYTES;
    const float* st_lse = stats + (step & 1) * 128;
    const float* st_d = st_lse + 64;
    if (step + 1 < steps) stage(step + 1, (step + 1) & 1);
    // ---- S = Q K^T and dP = dO V^T : rows = queries 16 mt + 4 quad + r, column = this lane's key
    floatx4 s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) s[mt] = dp[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < AB8_KSTEPS; ++ks)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 qa = *reinterpret_cast<ab8_lds_bf16x8*>(lds + (QS + mt * 16 * AB8_ROW_BYTES + ks * 64 + row_off));
        const bf16x8 oa = *reinterpret_cast<ab8_lds_bf16x8*>(lds + (OS + mt * 16 * AB8_ROW_BYTES + ks * 64 + row_off));
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
        const int q = qb * AB8_KB + mt * 16 + quad * 4 + r;
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
      for (int dt = 0; dt < AB8_DT; ++dt) {
        const int off = ks2 * 32 * AB8_ROW_BYTES + (dt >> 1) * 64 + tr_off[dt & 1];
        const bf16x8 ot = fa_read_vt<AB8_ROW_BYTES>(lds + (OS + off));
        const bf16x8 qt = fa_read_vt<AB8_ROW_BYTES>(lds + (QS + off));
        dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ot, pb[ks2], dvt[dt], 0, 0, 0);
        dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, dsb[ks2], dkt[dt], 0, 0, 0);
      }
    if (step + 1 < steps) commit_stats((step + 1) & 1);
    AB8_DMA_LANDED();   // this wave's pieces of step + 1
    __syncthreads();
  }
  if (kabs < T) {
    u16* kp = dqkv + (size_t)(tok0 + kabs) * stride + (nh + kvh) * hd + quad * 4;
    u16* vp = kp + nkv * hd;
#pragma unroll
    for (int dt = 0; dt < AB8_DT; ++dt) {
      u16x4 ok, ov;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = dkt[dt][r] * AB8_SCALE;
      ab8_unrotate(v, rope_cs, kabs, dt, quad);
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
int lr_launch_attention_bwd_hd96(const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv,
                                 const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd,
                                 hipStream_t st, const float* rope_cs) {
  if (hd != AB8_HD) LR_FAIL(LR_EUNSUPPORTED, "attention backward variant 8 needs head_dim 96 (got %d)", hd);
  int maxT = 0;
  for (int b = 0; b < B; ++b) maxT = max(maxT, cu_host[b + 1] - cu_host[b]);
  // the tiles come through buffer descriptors (32-bit byte offsets from a tile's first element)
  if ((long long)n_tok * (nh + 2 * nkv) * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward: packed qkv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  const int mq = (maxT + AB8_QROWS - 1) / AB8_QROWS, mk = (maxT + AB8_KB - 1) / AB8_KB;
  if (mq == 0) return LR_OK;
  if (nh > 65535 || nkv > 65535 || B > 65535)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward variant 8: %d heads / %d prompts exceed the grid limit", nh, B);
  static bool lds_set_dq[LR_MAX_DEVICES] = {}, lds_set_dkv[LR_MAX_DEVICES] = {};
  const int dkv_lds = 2 * AB8_STAGE_BYTES + 2 * 128 * (int)sizeof(float);
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_bwd_hd96_dq_kernel), 2 * AB8_STAGE_BYTES, lds_set_dq))
    return rc;
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_bwd_hd96_dkv_kernel), dkv_lds, lds_set_dkv))
    return rc;
  hipLaunchKernelGGL(attn_bwd_hd96_dq_kernel, dim3(mq, nh, B), dim3(256), 2 * AB8_STAGE_BYTES, st, qkv, d_out, lse, dsum,
                     dqkv, cu, nh, nkv, mq, rope_cs);
  LR_CHECK_LAUNCH("attn_bwd_hd96_dq_kernel");
  hipLaunchKernelGGL(attn_bwd_hd96_dkv_kernel, dim3(mk, nkv, B), dim3(256), dkv_lds, st, qkv, d_out, lse, dsum, dqkv, cu, nh,
                     nkv, rope_cs);
  LR_CHECK_LAUNCH("attn_bwd_hd96_dkv_kernel");
  return LR_OK;
}
