// llama_attn_hd256.hip -- attention variant 4: varlen causal flash attention at head_dim 256 on gfx950 (Gemma-2B / 7B).
//
// Variant 2's transposed formulation (llama_attn.hip) widened to 256 dimensions:
//   S^T = K Q^T   (A = K rows from LDS, B = Q rows held in registers) -> a lane owns ONE query row (lane & 15) and
//                 16 of the block's 64 keys
//   O^T = V^T P^T (A = V read with ds_read_b64_tr_b16 from the row-major LDS tile, B = P straight from the S^T
//                 accumulators) -> O's column is again the lane's query row: the online-softmax rescale is lane-local.
// Budget. At hd 256 a wave of variant 2's shape (32 query rows) holds 128 O^T accumulators and 64 Q^T
// registers per lane before any K fragment, score or address: only one such wave fits a SIMD. Here a wave owns 16 query
// rows: O^T 64, Q^T 32, S^T 16, two K fragment sets 32, P 8, row sums 4 -> < 256 registers, two waves per SIMD. A workgroup
// = 8 waves = 128 query rows of one (prompt, head), the same causal tile as variant 2; 64-key blocks, K and V tiles of
// 64 x 512 B = 32 KiB each, double-buffered: 128 KiB of LDS, one workgroup (8 waves) per CU.
// Each K / V fragment read from LDS feeds one MFMA (two in variant 2): 1 KiB per 16x16x32 MFMA, which one CU's LDS
// (256 B/clk) serves for four SIMDs at their full MFMA rate -- the kernel is bound by the softmax and the barriers long
// before that.
// Rounding points are variant 2's: fp32 scores and online softmax with the deferred maximum (a row's reference moves only
// when a score exceeds it by more than 2^FA4_DEFER), bf16 P into both the numerator and the row sum (an MFMA against a row
// of ones), one bf16 rounding of O / l. A query row's bits depend only on its own prompt: tiles and key blocks are aligned
// to positions inside the prompt, and the rescale decision is per row.
// Forward only, no log-sum-exp output (the LoRA path keeps its own kernels). This kernel takes no shared prefix: with one, and
// for the pruned last layer's one-query-row mode, lr_launch_attention runs the kernels of llama_attn_hd256_prefix.hip (same bits).
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
// 0-3 are 64 rows of head 2p, waves 4-7 the same rows of head 2p + 1, both fed by one staged K/V tile (same reuse of the LDS
// tile per stage, half-height causal tiles). Selected by lr_launch_attention_hd256; the other form is an A/B arm
// (tools/diag/attn_hd256_mqa_ab.py). A row's arithmetic is the same in both.
template <int HPW>
__global__ __launch_bounds__(512, 1) void attn_hd256_kernel(const u16* __restrict__ qkv, u16* out, const int32_t* cu,
                                                            int nh, int nkv, int max_qblocks, int n_pairs) {
  constexpr int WPH = FA4_WAVES / HPW;   // waves per head
  constexpr int QR = 16 * WPH;           // query rows per head and workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hd = FA4_HD;
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
    const int hg = nh / HPW;   // head groups per prompt
    seg = __builtin_amdgcn_readfirstlane(pair / hg);
    h = __builtin_amdgcn_readfirstlane((pair - seg * hg) * HPW);   // first head of the group
    qb = __builtin_amdgcn_readfirstlane(qb);
  }
  const int tok0 = cu[seg];
  const int T = cu[seg + 1] - tok0;
  if (qb * QR >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));   // (HPW = 2: both heads' KV head)
  h += wave / WPH;                                                      // this wave's head
  const int stride = (nh + 2 * nkv) * hd;
  const u16* kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
  const u16* vbase = kbase + nkv * hd;

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32 ks + 8 quad + 0..7
  const int wave_q0 = qb * QR + (wave % WPH) * 16;
  const int qabs = wave_q0 + li;
  bf16x8 qf[8];
  {
    const u16* qp = qkv + (size_t)(tok0 + min(qabs, T - 1)) * stride + h * hd + quad * 8;
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

  const int q_last = min(qb * QR + QR - 1, T - 1);
  const int kb_last = q_last / FA4_KB;
  const int wave_q_last = wave_q0 + 15;
  const bool wave_live = wave_q0 < T;              // the wave owns at least one row of the prompt
  const float sl2 = 0.0625f * 1.4426950408889634f;  // 1/sqrt(256) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

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
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * FA4_STAGE_BYTES + wave * 4096;
    const size_t blk_off = (size_t)kb * FA4_KB * stride * 2;
    const int records = ((T - 1 - kb * FA4_KB) * stride + hd) * 2;
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa_dma16(rk, base + i * 1024, koff[i]);
      fa_dma16(rv, base + FA4_TILE_BYTES + i * 1024, voff[i]);
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
    if (wave_live && kb * FA4_KB <= wave_q_last) {
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
      // ---- online softmax (lane-local row), P packed as the B operand of O^T = V^T P^T
      bf16x8 pa[2];
      const bool diag = (kb * FA4_KB + FA4_KB - 1) > wave_q0;
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
        const float m_new = grew ? rmx * sl2 : m_run;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
        for (int r = 0; r < 4; ++r) l_acc[r] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 16; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) ot[dt][r] *= alpha;
        m_run = m_new;
        mthr = (m_new + FA4_DEFER) * inv_sl2;
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pa[nt >> 1][(nt & 1) * 4 + r] = (__bf16)__builtin_amdgcn_exp2f(__builtin_fmaf(st[nt][r], sl2, -m_run));
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
  // (2k, 2k+1) gives even quads d = 32 k + 8 (quad / 2) .. +7 and odd quads the same + 16: 16-byte stores.
  const float inv = 1.0f / l_acc[0];
  const bool live = qabs < T;
  u16* op = out + (size_t)(tok0 + (live ? qabs : 0)) * nh * hd + h * hd + (quad & 1) * 16 + (quad >> 1) * 8;
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

template <int HPW>
static int launch_hd256(const u16* qkv, u16* out, const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh,
                        int nkv, int hd, hipStream_t st) {
  if (n_tok <= 0 || B <= 0) return LR_OK;
  if (hd != FA4_HD) LR_FAIL(LR_EUNSUPPORTED, "attention variant 4 needs head_dim 256 (got %d)", hd);
  if (nh < 1 || nkv < 1 || nh % nkv != 0)
    LR_FAIL(LR_EINVAL, "attention: num_heads %d not a multiple of num_kv_heads %d", nh, nkv);
  double work = 0;
  int maxT = 0;
  for (int b = 0; b < B; ++b) {
    const double T = cu_host[b + 1] - cu_host[b];
    work += 4.0 * nh * hd * (T * (T + 1) / 2);
    maxT = max(maxT, (int)T);
  }
  LrProfScope prof(LR_PROF_ATTN_MFMA, work, st);
  if (HPW == 2 && (nh / nkv) % 2 != 0) LR_FAIL(LR_EINVAL, "attention: two heads per workgroup need an even nh / nkv");
  constexpr int QR = 16 * FA4_WAVES / HPW;
  const int mq = (maxT + QR - 1) / QR;
  if (mq == 0) return LR_OK;
  const long long n_pairs_ll = (long long)B * (nh / HPW), grid_ll = 8 * ((n_pairs_ll + 7) / 8) * mq;
  if (grid_ll > 0x7fffffffLL) LR_FAIL(LR_EUNSUPPORTED, "attention: %lld workgroups exceed the grid limit", grid_ll);
  if ((long long)n_tok * (nh + 2 * nkv) * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention: packed qkv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  static bool lds_set[LR_MAX_DEVICES] = {};
  if (int rc = lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_hd256_kernel<HPW>), FA4_LDS_BYTES, lds_set)) return rc;
  hipLaunchKernelGGL(attn_hd256_kernel<HPW>, dim3((unsigned)grid_ll), dim3(512), FA4_LDS_BYTES, st, qkv, out, cu, nh, nkv, mq,
                     (int)n_pairs_ll);
  LR_CHECK_LAUNCH("attn_hd256_kernel");
  return LR_OK;
}

// cu / cu_host: prompt starts [B + 1] in packed rows (no shared prefix at head_dim 256)
int lr_launch_attention_hd256(const LrAttnArgs& a, hipStream_t st) {
  return launch_hd256<1>(a.qkv, a.out, a.cu, a.cu_host, a.S, a.n_tok, a.nh, a.nkv, a.hd, st);
}
