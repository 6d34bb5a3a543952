// llama_attn_bwd_hd256.hip -- attention variant 9's backward: the two passes of llama_attn_bwd_hd96.hip at head_dim 256 (LoRA
// fine-tuning of a Llama-format model of Gemma's head size), on v_mfma_f32_16x16x32_bf16, no atomics, one writer per element
// of dqkv.
//
// With P = exp(S - lse), D = rowsum(dO .* O) (lr_launch_rowdot):
//     dV = P^T dO,   dP = dO V^T,   dS = P .* (dP - D),   dQ = scale dS K,   dK = scale dS^T Q.
//  attn_bwd_hd256_dq_kernel  : a workgroup owns 128 query rows of one (prompt, head), a wave 16 of them (8 waves, the forward's
//                 tile); 64-key K and V tiles (32 KiB each, rows of 512 B) stream through LDS (LDS-DMA, two stages). Everything
//                 transposed: S^T = K Q^T (8 k-steps) and dP^T = V dO^T put a query row in a lane's accumulator column, so lse
//                 and D are one scalar per lane, and dS^T is, as it stands in the accumulators, the B operand of
//                 dQ^T += K^T dS^T over 16 d-tiles (K^T through ds_read_b64_tr_b16 from the row-major tile). dP^T is formed one
//                 16-key tile at a time and turned into dS^T at once, as in variant 8.
//  attn_bwd_hd256_dkv_kernel : a workgroup owns 64 keys of one kv head, a wave 16 of them (4 waves: one per SIMD, see the
//                 budget); it walks the query heads of its group and, for each, the 64-query blocks at or after its keys (Q and
//                 dO tiles by LDS-DMA, two stages; the block's lse / D through LDS): S = Q K^T, dP = dO V^T put a key in the
//                 accumulator column; P and dS are the B operands of dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T through
//                 transposed LDS reads).
// Rounding points are those of the other MFMA passes: fp32 scores, P = exp2(fma(s, scale log2 e, -lse log2 e)) in fp32 with
// scale = 1/16, P and dS rounded to bf16 before the second product, fp32 accumulation, one bf16 rounding of the result; the
// inverse rotation (rope_cs given) acts on the fp32 accumulators. A prompt's gradient rows depend on that prompt only: tiles
// are aligned to positions inside the prompt, rows past its end are range-checked to zero by the tile's buffer descriptor,
// masked in P and never stored.
//
// LDS layout. Every tile here is read both row-wise (ds_read_b128) and transposed (ds_read_b64_tr_b16), so one swizzle has to
// serve both; the forward's two (K: c ^ (r & 15), V: fa4_vswz) each serve one kind. Rows are stored back to back at 512 B = 32
// chunks of 16 B = two bank rows of 256 B, so every row starts at bank 0 and chunk position p of any row sits on the 16-byte
// slot p mod 16: the swizzle alone spreads rows over the banks. Chunk c of row r sits at position c ^ ab9_swz(r),
//     ab9_swz(r) = 2 g(r) | r3,   g(r) = (r & 7) ^ 4 r3,   r3 = (r >> 3) & 1          (bits 0-3 of the chunk index only: a
// chunk stays in its 256-byte half of the row, and sub-tiles 16 rows apart have the same swizzle). Derivation from the bank
// rule (bank = (byte / 4) mod 64 for both instructions; lane groups as measured on this card):
//  transposed: ds_read_b64_tr_b16 is served in two 32-lane halves; lane (li, quad) takes 8 bytes of row 4 quad + (li >> 2)
//    at chunk 2 dt + ((li & 3) >> 1), so a half takes chunks 2 dt, 2 dt + 1 (32 B) of the 8 rows 8 m .. 8 m + 7. The 32-byte
//    slot of a row is bits 1-3 of its position: (dt ^ g(r)) & 7. g is a bijection of r & 7 on each aligned group of 8 rows, so
//    the 8 rows take the 8 slots = all 64 banks once. Bit 0 of the swizzle (r3) swaps the two 16-byte halves inside a row's
//    slot; each lane addresses its own 8 bytes through the same formula, so the read does not care. (Under c ^ (r & 15) rows r
//    and r ^ 1 share a slot: 2-way; under fa4_vswz rows r and r + 4 do.)
//  row-wise: ds_read_b128 is served in four 16-lane groups that are not the quads: a group holds rows {0-3, 12-15} at the
//    chunk of quad q and rows {4-11} at the chunk of quad q ^ 1 (same k-step). The slot is bits 0-3 of c ^ ab9_swz(r). Over
//    rows {0-3, 12-15} ab9_swz takes {0, 2, 4, 6} and {1, 3, 5, 7}: the eight values with bit 3 clear; over rows {4-11} it takes
//    {8, 10, 12, 14} and {9, 11, 13, 15}: the eight with bit 3 set, and that set is closed under ^ 1. XOR with the group's
//    chunk bits keeps the two sets on opposite values of bit 3 and distinct inside: 16 lanes on 16 slots. (The same holds if a
//    group were simply 16 rows at one chunk, since ab9_swz is a bijection of r & 15.)
// Staging: a tile is 32 lane-linear DMA pieces of 1 KiB = 2 rows; lane l of a piece writes position l & 31 of row l >> 5 and
// reads the SOURCE chunk (l & 31) ^ ab9_swz(row). The counters for both passes are in DESIGN.md section 9.
//
// Budget. dQ pass per lane: Q^T 32 + dO^T 32 + dQ^T 64 + S^T 16 + dP^T 4 (per 16-key tile) + dS 8
// registers and 12 read addresses: under the 256 of two waves per SIMD (8 waves, 512 threads, the forward's occupancy). dK/dV
// pass per lane: K 32 + V 32 + dK^T 64 + dV^T 64 + S 16 + dP 16 + P / dS 16 = 240 before any fragment or address: it runs 4
// waves, one per SIMD, on the 512-register budget. LDS: two stages of two 32 KiB tiles = 128 KiB (dK/dV: + 1 KiB of row
// statistics) of the CU's 160: one workgroup per CU in both passes, the forward's situation.
#include "llama_attn_hd256_body.h"
#include "llama_train.h"

typedef u16 u16x4 __attribute__((ext_vector_type(4)));

#define AB9_HD FA4_HD
#define AB9_KB FA4_KB                      // keys (dQ pass) / queries (dK/dV pass) per streamed block
#define AB9_KSTEPS (AB9_HD / 32)           // 8 k-steps of 32 dims in S and dP
#define AB9_DT (AB9_HD / 16)               // 16 d-tiles of 16 in dQ, dK and dV
#define AB9_ROW_BYTES FA4_ROW_BYTES        // 512 B = 32 chunks of 16 B
#define AB9_TILE_BYTES FA4_TILE_BYTES      // 32 KiB = 32 DMA pieces of 1 KiB
#define AB9_STAGE_BYTES FA4_STAGE_BYTES    // two tiles
#define AB9_QROWS 128                      // query rows per workgroup in the dQ pass: 8 waves of 16
#define AB9_DQ_WAVES 8
#define AB9_DQ_PIECES 4                    // per wave and tile in the dQ pass: rows 8 w .. 8 w + 7
#define AB9_DKV_WAVES 4
#define AB9_DKV_PIECES 8                   // per wave and tile in the dK/dV pass: rows 16 w .. 16 w + 15
#define AB9_SCALE 0.0625f                  // 1 / sqrt(256)
#define AB9_LOG2E 1.4426950408889634f

#define AB9_DMA_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

typedef __attribute__((address_space(3))) const bf16x8 ab9_lds_bf16x8;

__device__ __forceinline__ int ab9_swz(int row) {
  const int r3 = (row >> 3) & 1;
  return ((((row & 7) ^ (r3 << 2)) << 1) | r3);
}

// The lane's source byte offsets of its NP DMA pieces inside a 64-row block whose rows are `stride` elements apart: piece i of
// wave w is rows 2 (NP w + i), 2 (NP w + i) + 1; the swizzle is applied to the SOURCE chunk.
template <int NP>
__device__ __forceinline__ void ab9_piece_offsets(int wave, int lane, int stride, unsigned (&off)[NP]) {
  const int prow = lane >> 5, ppos = lane & 31;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row = (wave * NP + i) * 2 + prow;
    off[i] = (unsigned)(row * stride + (ppos ^ ab9_swz(row)) * 8) * 2u;
  }
}
// Row reads: row 16 t + li, chunk 4 ks + quad. The swizzle touches chunk bits 0-3, so the four k-steps of a 256-byte half are
// four addresses; k-steps 4-7 are the same + 256 B, sub-tiles differ by 16 rows (immediates).
__device__ __forceinline__ void ab9_row_offsets(int quad, int li, int (&off)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) off[ks] = li * AB9_ROW_BYTES + (((ks * 4 + quad) ^ ab9_swz(li)) << 4);
}
// A operand = X^T fragment of a row-major LDS tile X[row][d] for the 16-dim tile dt and the 32-row step ks2 (fa_read_vt):
// element e < 4: row 32 ks2 + 4 quad + e, e >= 4: the same + 16; M index (lane & 15) = dim 16 dt + li. The lane's address for
// d-tile dt is tr_off[dt & 7] + 256 (dt >> 3): chunk 2 dt + ((li & 3) >> 1) with bits 0-3 swizzled by the row.
__device__ __forceinline__ void ab9_tr_offsets(int quad, int li, int (&off)[8]) {
  const int qp = li >> 2, p4 = li & 3, row = quad * 4 + qp;
#pragma unroll
  for (int d = 0; d < 8; ++d) off[d] = AB9_ROW_BYTES * row + 16 * ((d * 2 + (p4 >> 1)) ^ ab9_swz(row)) + 8 * (p4 & 1);
}

// Optional epilogue: gradient w.r.t. the UNROTATED q / k. A lane holds dims 16 dt + 4 quad + 0..3 = rotation pairs
// i0 = 8 dt + 2 quad and i0 + 1 of its row (packed layout: pair (x1_i, x2_i) adjacent); 128 pairs per position, so the two
// pairs are one aligned float4 of the table.
__device__ __forceinline__ void ab9_unrotate(float (&v)[4], const float* rope_cs, int pos, int dt, int quad) {
  if (!rope_cs) return;
  const float4 cs = *reinterpret_cast<const float4*>(rope_cs + ((size_t)pos * (AB9_HD / 2) + dt * 8 + 2 * quad) * 2);
  const float a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
  v[0] = a0 * cs.x + a1 * cs.y;
  v[1] = a1 * cs.x - a0 * cs.y;
  v[2] = b0 * cs.z + b1 * cs.w;
  v[3] = b1 * cs.z - b0 * cs.w;
}

// ---------------------------------------------------------------------------------------------
// dQ pass
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * AB9_DQ_WAVES, 1) void attn_bwd_hd256_dq_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, int max_qblocks,
    const float* __restrict__ rope_cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][K tile | V tile]
  const int hd = AB9_HD;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qb = max_qblocks - 1 - (int)blockIdx.x;   // heavy tiles first
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (qb * AB9_QROWS >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = h / (nh / nkv);
  const int stride = (nh + 2 * nkv) * hd;
  const u16* kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
  const u16* vbase = kbase + nkv * hd;

  // ---- Q and dO fragments (B operands): row q, d = 32 ks + 8 quad + 0..7; lse and D of the lane's row
  const int wave_q0 = qb * AB9_QROWS + wave * 16;
  const int qabs = wave_q0 + li;
  bf16x8 qf[AB9_KSTEPS], dof[AB9_KSTEPS];
  float lse2, dq_row;
  {
    const int qr = min(qabs, T - 1);
    const u16* qp = qkv + (size_t)(tok0 + qr) * stride + h * hd + quad * 8;
    const u16* dp = d_out + (size_t)(tok0 + qr) * nh * hd + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < AB9_KSTEPS; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
      dof[ks] = *reinterpret_cast<const bf16x8*>(dp + ks * 32);
    }
    lse2 = lse[(size_t)(tok0 + qr) * nh + h] * AB9_LOG2E;
    dq_row = dsum[(size_t)(tok0 + qr) * nh + h];
  }
  floatx4 dqt[AB9_DT];
#pragma unroll
  for (int dt = 0; dt < AB9_DT; ++dt) dqt[dt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int q_last = min(qb * AB9_QROWS + AB9_QROWS - 1, T - 1);
  const int kb_last = q_last / AB9_KB;
  const int wave_q_last = wave_q0 + 15;
  const bool wave_live = wave_q0 < T;
  const float sl2 = AB9_SCALE * AB9_LOG2E;

  // ---- DMA staging: wave w moves pieces 4w .. 4w + 3 of K and of V (V's rows stand nkv hd elements behind K's, which the
  // descriptors' bases carry). Rows past the prompt's end are range-checked to zero by the per-block buffer descriptor (those
  // keys are masked for every query row of the prompt).
  unsigned soff[AB9_DQ_PIECES];
  ab9_piece_offsets<AB9_DQ_PIECES>(wave, lane, stride, soff);
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * AB9_STAGE_BYTES + wave * (AB9_DQ_PIECES * 1024);
    const size_t blk_off = (size_t)kb * AB9_KB * stride * 2;
    const int records = ((T - 1 - kb * AB9_KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < AB9_DQ_PIECES; ++i) {
      fa_dma16(rk, base + i * 1024, soff[i]);
      fa_dma16(rv, base + AB9_TILE_BYTES + i * 1024, soff[i]);
    }
  };
  // LDS read addresses, the lane's part computed once
  lds_char* const lds = (lds_char*)smem;
  int row_off[4], tr_off[8];
  ab9_row_offsets(quad, li, row_off);
  ab9_tr_offsets(quad, li, tr_off);

  stage(0, 0);
  // Q, dO and the statistics must be resident before the loop: otherwise their loads are waited for behind the in-loop DMA
#pragma unroll
  for (int ks = 0; ks < AB9_KSTEPS; ++ks) asm volatile("" ::"v"(qf[ks]), "v"(dof[ks]));
  asm volatile("" ::"v"(lse2), "v"(dq_row));
  AB9_DMA_LANDED();
  __syncthreads();

  for (int kb = 0; kb <= kb_last; ++kb) {
    const int KS = (kb & 1) * AB9_STAGE_BYTES, VS = KS + AB9_TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, (kb + 1) & 1);
    if (wave_live && kb * AB9_KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T (rows = keys 16 nt + 4 quad + r, column = query li), then P^T in place
      floatx4 st[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) st[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < AB9_KSTEPS; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 kf = *reinterpret_cast<ab9_lds_bf16x8*>(
              lds + (KS + nt * 16 * AB9_ROW_BYTES + (ks >> 2) * 256 + row_off[ks & 3]));
          st[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], st[nt], 0, 0, 0);
        }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb * AB9_KB + nt * 16 + quad * 4 + r;
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[nt][r], sl2, -lse2));
          st[nt][r] = (key <= qabs && qabs < T) ? p : 0.f;
        }
      // ---- dP^T = V dO^T, one 16-key tile at a time, and dS^T = P^T .* (dP^T - D) from it at once, packed as the B operand of
      // dQ^T += K^T dS^T (k index 8 quad + j <-> key 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it)
      bf16x8 dsb[2];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        floatx4 dpt = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < AB9_KSTEPS; ++ks) {
          const bf16x8 vf = *reinterpret_cast<ab9_lds_bf16x8*>(
              lds + (VS + nt * 16 * AB9_ROW_BYTES + (ks >> 2) * 256 + row_off[ks & 3]));
          dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[ks], dpt, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dsb[nt >> 1][(nt & 1) * 4 + r] = (__bf16)(st[nt][r] * (dpt[r] - dq_row));
      }
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
        for (int dt = 0; dt < AB9_DT; ++dt) {
          const bf16x8 kt =
              fa_read_vt<AB9_ROW_BYTES>(lds + (KS + ks2 * 32 * AB9_ROW_BYTES + (dt >> 3) * 256 + tr_off[dt & 7]));
          dqt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, dsb[ks2], dqt[dt], 0, 0, 0);
        }
    }
    AB9_DMA_LANDED();   // this wave's pieces of block kb + 1
    __syncthreads();
  }
  // ---- store scale * dQ: lane owns query row li, d = 16 dt + 4 quad + r
  if (qabs < T) {
    u16* op = dqkv + (size_t)(tok0 + qabs) * stride + h * hd + quad * 4;
#pragma unroll
    for (int dt = 0; dt < AB9_DT; ++dt) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = dqt[dt][r] * AB9_SCALE;
      ab9_unrotate(v, rope_cs, qabs, dt, quad);
      u16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f2bf(v[r]);
      *reinterpret_cast<u16x4*>(op + dt * 16) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// dK / dV pass
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * AB9_DKV_WAVES, 1) void attn_bwd_hd256_dkv_kernel(
    const u16* __restrict__ qkv, const u16* __restrict__ d_out, const float* __restrict__ lse,
    const float* __restrict__ dsum, u16* dqkv, const int32_t* cu, int nh, int nkv, const float* __restrict__ rope_cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][Q tile | dO tile], then the statistics
  float* stats = reinterpret_cast<float*>(smem + 2 * AB9_STAGE_BYTES);  // [2 stages][lse2[64] | D[64]]
  const int hd = AB9_HD;
  const int b = blockIdx.z, kvh = blockIdx.y, kb = blockIdx.x;
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (kb * AB9_KB >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int rep = nh / nkv;
  const int stride = (nh + 2 * nkv) * hd;
  const int ostride = nh * hd;

  // ---- this lane's key: K and V fragments (B operands), d = 32 ks + 8 quad + 0..7
  const int kabs = kb * AB9_KB + wave * 16 + li;
  const int kr = min(kabs, T - 1);
  bf16x8 kf[AB9_KSTEPS], vf[AB9_KSTEPS];
  {
    const u16* kp = qkv + (size_t)(tok0 + kr) * stride + (nh + kvh) * hd + quad * 8;
    const u16* vp = kp + nkv * hd;
#pragma unroll
    for (int ks = 0; ks < AB9_KSTEPS; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8*>(kp + ks * 32);
      vf[ks] = *reinterpret_cast<const bf16x8*>(vp + ks * 32);
    }
  }
  floatx4 dkt[AB9_DT], dvt[AB9_DT];
#pragma unroll
  for (int dt = 0; dt < AB9_DT; ++dt) dkt[dt] = dvt[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = AB9_SCALE * AB9_LOG2E;

  const int qb_first = kb, qb_last = (T - 1) / AB9_KB;
  const int nqb = qb_last - qb_first + 1;
  const int steps = nqb * rep;  // (query head of the group, query block) pairs, head-major
  // DMA staging as in the dQ pass: wave w moves pieces 8w .. 8w + 7 of the Q tile (row stride of qkv) and of the dO tile
  // (row stride of d_out); rows past the prompt's end come back as zeros and are masked in P.
  unsigned qoff[AB9_DKV_PIECES], ooff[AB9_DKV_PIECES];
  ab9_piece_offsets<AB9_DKV_PIECES>(wave, lane, stride, qoff);
  ab9_piece_offsets<AB9_DKV_PIECES>(wave, lane, ostride, ooff);
  // a step's tiles are requested at the top of the step before (LDS-DMA) together with its 64 query rows' statistics
  // (ordinary loads into two registers of wave 0); the statistics are written to LDS at the END of that step, so that the
  // wait hipcc puts in front of the write coincides with the hand-written one for the DMA
  float st_l = 0.f, st_dd = 0.f;
  auto stage = [&](int step, int buf) {
    const int h = kvh * rep + step / nqb, qb = qb_first + step % nqb;
    char* base = smem + buf * AB9_STAGE_BYTES + wave * (AB9_DKV_PIECES * 1024);
    const int rows_left = T - 1 - qb * AB9_KB;
    const fa_int4 rq = fa_make_rsrc(
        reinterpret_cast<const char*>(qkv + (size_t)tok0 * stride + h * hd) + (size_t)qb * AB9_KB * stride * 2,
        (rows_left * stride + hd) * 2);
    const fa_int4 ro = fa_make_rsrc(
        reinterpret_cast<const char*>(d_out + (size_t)tok0 * ostride + h * hd) + (size_t)qb * AB9_KB * ostride * 2,
        (rows_left * ostride + hd) * 2);
#pragma unroll
    for (int i = 0; i < AB9_DKV_PIECES; ++i) {
      fa_dma16(rq, base + i * 1024, qoff[i]);
      fa_dma16(ro, base + AB9_TILE_BYTES + i * 1024, ooff[i]);
    }
    if (tid < 64) {
      const int q = min(qb * AB9_KB + tid, T - 1);
      st_l = lse[(size_t)(tok0 + q) * nh + h];   // (first use of either value: commit_stats)
      st_dd = dsum[(size_t)(tok0 + q) * nh + h];
    }
  };
  auto commit_stats = [&](int buf) {
    __builtin_amdgcn_sched_barrier(0);
    if (tid < 64) {
      stats[buf * 128 + tid] = st_l * AB9_LOG2E;
      stats[buf * 128 + 64 + tid] = st_dd;
    }
  };
  lds_char* const lds = (lds_char*)smem;
  int row_off[4], tr_off[8];
  ab9_row_offsets(quad, li, row_off);
  ab9_tr_offsets(quad, li, tr_off);

  stage(0, 0);
#pragma unroll
  for (int ks = 0; ks < AB9_KSTEPS; ++ks) asm volatile("" ::"v"(kf[ks]), "v"(vf[ks]));
  commit_stats(0);
  AB9_DMA_LANDED();
  __syncthreads();

  for (int step = 0; step < steps; ++step) {
    const int qb = qb_first + step % nqb;
    const int QS = (step & 1) * AB9_STAGE_BYTES, OS = QS + AB9_TILE_BYTES;
    const float* st_lse = stats + (step & 1) * 128;
    const float* st_d = st_lse + 64;
    if (step + 1 < steps) stage(step + 1, (step + 1) & 1);
    // ---- S = Q K^T and dP = dO V^T : rows = queries 16 mt + 4 quad + r, column = this lane's key
    floatx4 s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) s[mt] = dp[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < AB9_KSTEPS; ++ks)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int off = mt * 16 * AB9_ROW_BYTES + (ks >> 2) * 256 + row_off[ks & 3];
        const bf16x8 qa = *reinterpret_cast<ab9_lds_bf16x8*>(lds + (QS + off));
        const bf16x8 oa = *reinterpret_cast<ab9_lds_bf16x8*>(lds + (OS + off));
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
        const int q = qb * AB9_KB + mt * 16 + quad * 4 + r;
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
      for (int dt = 0; dt < AB9_DT; ++dt) {
        const int off = ks2 * 32 * AB9_ROW_BYTES + (dt >> 3) * 256 + tr_off[dt & 7];
        const bf16x8 ot = fa_read_vt<AB9_ROW_BYTES>(lds + (OS + off));
        const bf16x8 qt = fa_read_vt<AB9_ROW_BYTES>(lds + (QS + off));
        dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ot, pb[ks2], dvt[dt], 0, 0, 0);
        dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, dsb[ks2], dkt[dt], 0, 0, 0);
      }
    if (step + 1 < steps) commit_stats((step + 1) & 1);
    AB9_DMA_LANDED();   // this wave's pieces of step + 1
    __syncthreads();
  }
  if (kabs < T) {
    u16* kp = dqkv + (size_t)(tok0 + kabs) * stride + (nh + kvh) * hd + quad * 4;
    u16* vp = kp + nkv * hd;
#pragma unroll
    for (int dt = 0; dt < AB9_DT; ++dt) {
      u16x4 ok, ov;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = dkt[dt][r] * AB9_SCALE;
      ab9_unrotate(v, rope_cs, kabs, dt, quad);
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
int lr_launch_attention_bwd_hd256(const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv,
                                  const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd,
                                  hipStream_t st, const float* rope_cs) {
  if (hd != AB9_HD) LR_FAIL(LR_EUNSUPPORTED, "attention backward variant 9 needs head_dim 256 (got %d)", hd);
  int maxT = 0;
  for (int b = 0; b < B; ++b) maxT = max(maxT, cu_host[b + 1] - cu_host[b]);
  // the tiles come through buffer descriptors (32-bit byte offsets from a tile's first element)
  if ((long long)n_tok * (nh + 2 * nkv) * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward: packed qkv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  const int mq = (maxT + AB9_QROWS - 1) / AB9_QROWS, mk = (maxT + AB9_KB - 1) / AB9_KB;
  if (mq == 0) return LR_OK;
  if (nh > 65535 || nkv > 65535 || B > 65535)
    LR_FAIL(LR_EUNSUPPORTED, "attention backward variant 9: %d heads / %d prompts exceed the grid limit", nh, B);
  static bool lds_set_dq[LR_MAX_DEVICES] = {}, lds_set_dkv[LR_MAX_DEVICES] = {};
  const int dkv_lds = 2 * AB9_STAGE_BYTES + 2 * 128 * (int)sizeof(float);
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_bwd_hd256_dq_kernel), 2 * AB9_STAGE_BYTES, lds_set_dq))
    return rc;
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_bwd_hd256_dkv_kernel), dkv_lds, lds_set_dkv))
    return rc;
  hipLaunchKernelGGL(attn_bwd_hd256_dq_kernel, dim3(mq, nh, B), dim3(64 * AB9_DQ_WAVES), 2 * AB9_STAGE_BYTES, st, qkv, d_out,
                     lse, dsum, dqkv, cu, nh, nkv, mq, rope_cs);
  LR_CHECK_LAUNCH("attn_bwd_hd256_dq_kernel");
  hipLaunchKernelGGL(attn_bwd_hd256_dkv_kernel, dim3(mk, nkv, B), dim3(64 * AB9_DKV_WAVES), dkv_lds, st, qkv, d_out, lse, dsum,
                     dqkv, cu, nh, nkv, rope_cs);
  LR_CHECK_LAUNCH("attn_bwd_hd256_dkv_kernel");
  return LR_OK;
}
