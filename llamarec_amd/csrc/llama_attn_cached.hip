// llama_attn_cached.hip -- causal varlen attention whose query rows and key rows are different sets (ranker sessions,
// DESIGN 16): segment b has q_len[b] query rows of THIS call at prompt positions cached_len[b] .. cached_len[b] + q_len[b] - 1
// and reads its kv_len[b] = cached_len[b] + q_len[b] keys and values from the user's cache slot, whose row p is
// [K rotated | V] of position p (width 2 nkv hd: the row format of the one-query-row kernels). Query row i sees keys
// 0 .. cached_len[b] + i. The call's own K | V rows are copied into the slot first (kv_cache_write_kernel), so the attention
// has one K / V source.
//
//  kv_cache_meta_kernel        : per new row its position; per prompt its last row and that row's position
//  kv_cache_write_kernel       : K | V columns of the call's packed rows -> slot rows cached_len[b] ..
//  attn_cached_generic_kernel  : any head_dim <= 256, GQA, one wave per (query row, head): attn_generic_kernel's arithmetic
//                                 (llama_attn.hip) on the slot's rows
//  attn_cached128_kernel       : head_dim 128: attn_mfma128_kernel's arithmetic (llama_attn.hip: S^T = K Q^T and
//                                 O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, K / V by LDS-DMA, 128 query rows per workgroup,
//                                 16-row tiles against 64-key blocks, deferred maximum) with the K / V source and the row
//                                 ownership changed and nothing else: query tiles and 64-key blocks stay aligned to positions
//                                 inside the prompt, a key block's LDS image (swizzles, zero rows past the prompt's end) is the
//                                 one that kernel builds, and a row runs the same operations in the same order on it. That is
//                                 why a row's bits equal the whole-prompt kernel's. LASTQ = its one-query-row mode: one row per
//                                 prompt, the query at position kv_len - 1 (the pruned last layer).
// The whole-prompt kernels are held to their instruction streams, so this is a translation unit of its own and no mode of
// theirs.
#include "llama_kernels.h"
#include "lr_attn_util.h"

#include <type_traits>

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// =============================================================================================
// metadata and the cache write
// =============================================================================================
// the prompt of packed row r: largest b with cu[b] <= r
__device__ __forceinline__ int kc_segment_of(const int32_t* cu, int B, int r) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void kv_cache_meta_kernel(const int32_t* cu, const int32_t* cached_len, int B, int n,
                                                            int32_t* tok_pos, int32_t* last_rows, int32_t* last_pos) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n) {
    const int b = kc_segment_of(cu, B, r);
    tok_pos[r] = cached_len[b] + r - cu[b];
  }
  if (r < B) {
    last_rows[r] = cu[r + 1] - 1;
    last_pos[r] = cached_len[r] + cu[r + 1] - cu[r] - 1;
  }
}

// src [n][ld] holds K | V (kv_w columns) from column col0; packed row r of prompt b goes to row cached_len[b] + r - cu[b] of
// slot slots[b] in dst = the table at the layer's row offset (rows of kv_w columns, slot_elems elements from slot to slot).
// A workgroup per row, 8 bytes per lane and step: col0 and ld are multiples of 4 elements (head_dim % 4 == 0).
__global__ __launch_bounds__(256) void kv_cache_write_kernel(const u16* src, int ld, int col0, int kv_w, const int32_t* cu,
                                                             const int32_t* cached_len, const int32_t* slots, int B,
                                                             long long slot_elems, u16* dst, int n) {
  const int r = blockIdx.x;
  if (r >= n) return;
  const int b = kc_segment_of(cu, B, r);
  const int pos = cached_len[b] + r - cu[b];
  const uint2* s = reinterpret_cast<const uint2*>(src + (size_t)r * ld + col0);
  uint2* d = reinterpret_cast<uint2*>(dst + (size_t)slots[b] * (size_t)slot_elems + (size_t)pos * kv_w);
  for (int i = threadIdx.x; i < kv_w / 4; i += 256) d[i] = s[i];
}

// =============================================================================================
// generic
// =============================================================================================
__global__ __launch_bounds__(256) void attn_cached_generic_kernel(const u16* q, int q_ld, u16* out, const u16* kv,
                                                                  long long slot_elems, const int32_t* slots,
                                                                  const int32_t* cached_len, const int32_t* cu, int B, int n_rows,
                                                                  int nh, int nkv, int hd, const int32_t* q_rows) {
  __shared__ float qs[4][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + wave;  // (query row, head)
  if (item >= n_rows * nh) return;
  // q_rows (optional): only these packed rows are evaluated and the output is compact [n_rows][nh * hd]
  const int orow = item / nh, h = item % nh;
  const int tok = q_rows ? q_rows[orow] : orow;
  const int kvh = h / (nh / nkv);
  const int stride = 2 * nkv * hd;
  const int b = kc_segment_of(cu, B, tok);
  const int pos = cached_len[b] + tok - cu[b];
  const u16* kbase = kv + (size_t)slots[b] * slot_elems + kvh * hd;
  const u16* vbase = kbase + nkv * hd;
  const u16* qp = q + (size_t)tok * q_ld + h * hd;
  for (int d = lane; d < hd; d += 64) qs[wave][d] = bf2f(qp[d]);
  __builtin_amdgcn_wave_barrier();
  const float scale = 1.0f / sqrtf((float)hd);
  float m = -__builtin_inff(), l = 0.f;
  float o[4] = {0.f, 0.f, 0.f, 0.f};  // dims lane, lane+64, lane+128, lane+192
  for (int k0 = 0; k0 <= pos; k0 += 64) {
    const int key = k0 + lane;
    float s = -__builtin_inff();
    if (key <= pos) {
      const u16* kp = kbase + (size_t)key * stride;
      float acc = 0.f;
      for (int d = 0; d < hd; ++d) acc = __builtin_fmaf(qs[wave][d], bf2f(kp[d]), acc);
      s = acc * scale;
    }
    float mx = s;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sft, 64));
    const float m_new = fmaxf(m, mx);
    const float alpha = __expf(m - m_new);
    const float p = (key <= pos) ? __expf(s - m_new) : 0.f;
    float ps = p;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) ps += __shfl_xor(ps, sft, 64);
    l = l * alpha + ps;
    m = m_new;
    const float pb = bf2f(f2bf(p));  // P enters the PV product in bf16, like the MFMA path
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] *= alpha;
    const int nk = min(64, pos - k0 + 1);
    for (int j = 0; j < nk; ++j) {
      const float pj = __shfl(pb, j, 64);
      const u16* vp = vbase + (size_t)(k0 + j) * stride;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int d = lane + 64 * i;
        if (d < hd) o[i] = __builtin_fmaf(pj, bf2f(vp[d]), o[i]);
      }
    }
  }
  u16* op = out + (size_t)orow * nh * hd + h * hd;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int d = lane + 64 * i;
    if (d < hd) op[d] = f2bf(o[i] / l);
  }
}

// =============================================================================================
// MFMA, head_dim 128
// =============================================================================================
#define FC_QROWS 128  // query rows per workgroup
#define FC_KB 64      // keys per block
#define FC_DEFER 8.0f  // a row's softmax reference moves only when a score exceeds it by more than this (exp2 domain)

__device__ __forceinline__ int fc_v_off(int row, int ch) {  // dual-use swizzle, 256-byte rows
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

#define FC_TILE_BYTES (FC_KB * 256)        // one K or V tile: 64 keys x 128 dims bf16
#define FC_STAGE_BYTES (2 * FC_TILE_BYTES)  // K tile + V tile

// grid (query tiles of the call's longest new part, nh, B). A workgroup's tile is tile cached_len / 128 + (its x from the
// end: heavy tiles first) of the prompt's positions; rows of the tile at positions < cached_len (they are cached, not this
// call's) or >= kv_len are computed on a clamped row and not stored. LASTQ: grid (1, nh, B), q / out hold one row per prompt.
template <bool LASTQ>
__global__ __launch_bounds__(256, 2) void attn_cached128_kernel(const u16* __restrict__ q, int q_ld, u16* out,
                                                                const u16* __restrict__ kv, long long slot_elems,
                                                                const int32_t* slots, const int32_t* cached_len,
                                                                const int32_t* cu, int nh, int nkv) {
  // [2 stages][K 16 KiB | V 16 KiB]; filled by LDS-DMA (lane-linear 1 KiB pieces = 4 rows x 256 B),
  // the XOR swizzles are applied to the SOURCE chunk: position p of row r holds chunk p ^ s(r).
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hd = 128;
  const int seg = blockIdx.z, h = blockIdx.y;
  const int q0 = cu[seg];
  const int c = cached_len[seg];          // keys [0, c) were cached by earlier calls
  const int T = c + cu[seg + 1] - q0;     // sequence length, cached part included
  int qb;
  if (LASTQ) {
    qb = (T - 1) / FC_QROWS;
  } else {
    qb = c / FC_QROWS + ((int)gridDim.x - 1 - (int)blockIdx.x);
    if (qb * FC_QROWS >= T) return;  // no query row of this prompt in the tile
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const int stride = 2 * nkv * hd;
  const u16* kbase = kv + (size_t)slots[seg] * (size_t)slot_elems + kvh * hd;   // the row of position p is row p of the slot
  const u16* vbase = kbase + nkv * hd;

  // ---- Q fragments (B operand of S^T = K Q^T): row q, d = 32*ks + 8*quad + 0..7
  bf16x8 qf[2][4];
  int qabs[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    qabs[qt] = LASTQ ? T - 1 : qb * FC_QROWS + wave * 32 + qt * 16 + li;
    const int qr = min(max(qabs[qt], c), T - 1);
    const u16* qp = LASTQ ? q + (size_t)seg * q_ld + h * hd + quad * 8
                          : q + (size_t)(q0 + qr - c) * q_ld + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  }

  floatx4 ot[2][8];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) ot[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-__builtin_inff(), -__builtin_inff()};
  float mthr[2] = {-__builtin_inff(), -__builtin_inff()};   // (m + FC_DEFER) / scale of the lane's row, in raw-score units
  // row sums of P through the matrix pipe: one more A row of ones beside V^T
  floatx4 l_acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
  bf16x8 ones_f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones_f[i] = (__bf16)1.0f;

  const int q_last = min(qb * FC_QROWS + FC_QROWS - 1, T - 1);   // (LASTQ: qb is the tile of row T - 1, so this is T - 1)
  const int kb_last = q_last / FC_KB;
  const int wave_q_last = LASTQ ? T - 1 : qb * FC_QROWS + wave * 32 + 31;  // last query row this wave owns
  const float sl2 = 0.08838834764831845f * 1.4426950408889634f;  // 1/sqrt(128) * log2(e)
  const float inv_sl2 = 1.0f / sl2;

  // ---- DMA staging: 16 pieces per tile (4 rows each); wave w moves pieces 4w..4w+3 of K and of V
  const int prow = lane >> 4, ppos = lane & 15;
  unsigned koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 4 + prow;
    koff[i] = (unsigned)(row * stride + (ppos ^ (row & 15)) * 8) * 2u;
    voff[i] = (unsigned)(row * stride + (ppos ^ (((row & 3) << 2) | ((row >> 2) & 3))) * 8) * 2u;
  }
  // Every block is fetched through a per-block buffer descriptor: base = the block's first K (V) row in the slot,
  // num_records = the bytes up to the end of row T - 1, so rows past the sequence end -- slot rows an earlier, longer prompt
  // may have left behind -- are range-checked to ZERO by the hardware, as the whole-prompt kernel's are (those keys are
  // causally masked for every stored query row: P = 0 exactly).
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * FC_STAGE_BYTES + wave * 4096;
    const size_t blk_off = (size_t)kb * FC_KB * stride * 2;
    const int records = ((T - 1 - kb * FC_KB) * stride + hd) * 2;  // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa_dma16(rk, base + i * 1024, koff[i]);
      fa_dma16(rv, base + FC_TILE_BYTES + i * 1024, voff[i]);
    }
  };

  // LDS read addresses: everything lane-dependent is computed ONCE (4 K bases, 8 V bases)
  typedef __attribute__((address_space(3))) char lds_char;
  lds_char* const lds = (lds_char*)smem;
  lds_char *kb_off[4], *vb_off[8];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kb_off[ks] = lds + (li * 256 + (((ks * 4 + quad) ^ li) << 4));   // row nt*16 + li: (row & 15) = li
  {
    const int qp = li >> 2, p4 = li & 3;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) vb_off[dt] = lds + (fc_v_off(quad * 4 + qp, dt * 2 + (p4 >> 1)) + 8 * (p4 & 1));   // + 8192 ks2 + 4096 half
  }

  stage(0, 0);
  // Q must be resident before the loop (llama_attn.hip)
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" ::"v"(qf[qt][ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm DMAs of block 0 (hipcc does not count them)
  __syncthreads();

  auto block = [&](const int kb, auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    constexpr int KS = BUF * FC_STAGE_BYTES, VS = KS + FC_TILE_BYTES;   // LDS byte offsets of this block's K and V tiles
    if (kb < kb_last) stage(kb + 1, BUF ^ 1);

    if (kb * FC_KB <= wave_q_last && wave_q_last >= c && (!LASTQ || wave == 0)) {  // otherwise every key of the block is masked
                                                          // for this wave (or all its rows are cached rows)
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

      // ---- online softmax (lane-local row), P packed as the B operand of O^T = V^T P^T
      bf16x8 pa[2][2];
      const bool diag = (kb * FC_KB + FC_KB - 1) > (LASTQ ? T - 1 : qb * FC_QROWS + wave * 32);  // block needs masking
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float mx = -__builtin_inff();
        if (diag) {  // a real (wave-uniform) branch
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kb * FC_KB + nt * 16 + quad * 4 + r;
              st[qt][nt][r] = (key <= qabs[qt]) ? st[qt][nt][r] : -__builtin_inff();
            }
          __builtin_amdgcn_sched_barrier(0);
        }
        mx = fa_max3(st[qt][0][0], st[qt][0][1], st[qt][0][2]);
        mx = fa_max3(mx, st[qt][0][3], st[qt][1][0]);
#pragma unroll
        for (int nt = 1; nt < 4; ++nt) {
          mx = fa_max3(mx, st[qt][nt][1], st[qt][nt][2]);
          if (nt < 3) mx = fa_max3(mx, st[qt][nt][3], st[qt][nt + 1][0]);
        }
        mx = fa_max2(mx, st[qt][3][3]);      // this lane's 16 keys of the row
        // deferred maximum, decided per row: a row that keeps its reference multiplies by exactly 1 (llama_attn.hip)
        if (__any(mx > mthr[qt])) {
          const float rmx = fa_max_xor16_32(mx);
          const bool grew = rmx > mthr[qt];
          const float m_new = grew ? rmx * sl2 : m_run[qt];
          const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);
#pragma unroll
          for (int r = 0; r < 4; ++r) l_acc[qt][r] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 8; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[qt][dt][r] *= alpha;
          m_run[qt] = m_new;
          mthr[qt] = (m_new + FC_DEFER) * inv_sl2;
        }
        const float m_new = m_run[qt];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qt][nt][r], sl2, -m_new));
            pa[qt][nt >> 1][(nt & 1) * 4 + r] = (__bf16)p;
          }
      }

      // ---- O^T += V^T P^T : A = V^T fragment via transposed LDS reads
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) l_acc[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pa[qt][ks2], l_acc[qt], 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
          const short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt] + (VS + ks2 * 8192)));
          const short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(vb_off[dt] + (VS + ks2 * 8192 + 4096)));
          bf16x8 vf;
          const bf16x4 b0 = __builtin_bit_cast(bf16x4, t0), b1 = __builtin_bit_cast(bf16x4, t1);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            vf[r] = b0[r];
            vf[4 + r] = b1[r];
          }
#pragma unroll
          for (int qt = 0; qt < 2; ++qt)
            ot[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pa[qt][ks2], ot[qt][dt], 0, 0, 0);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of block kb + 1 have landed
    __syncthreads();  // ... and every wave is done with block kb
  };
  for (int kb = 0; kb <= kb_last; kb += 2) {
    block(kb, std::integral_constant<int, 0>{});
    if (kb + 1 <= kb_last) block(kb + 1, std::integral_constant<int, 1>{});
  }

  // ---- normalise and store: lane owns query row li, d = dt*16 + 4*quad + r (v_permlane16_swap pairs -> 16-byte stores).
  // Every lane takes part in the swaps; only rows this call owns store.
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float l = l_acc[qt][0];
    const float inv = 1.0f / l;
    const bool live = LASTQ ? (wave == 0 && qt == 0 && li == 0) : (qabs[qt] < T && qabs[qt] >= c);
    u16* op = out + (size_t)(LASTQ ? seg : q0 + (live ? qabs[qt] - c : 0)) * nh * hd + h * hd + (quad & 1) * 16 + (quad >> 1) * 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
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

// =============================================================================================
// launchers (declared in llama_kernels.h)
// =============================================================================================
int lr_launch_kv_cache_meta(const int32_t* cu, const int32_t* cached_len, int B, int n, int32_t* tok_pos, int32_t* last_rows,
                            int32_t* last_pos, hipStream_t st) {
  if (n <= 0 || B <= 0) return LR_OK;
  LrProfScope prof(LR_PROF_ELEMENTWISE, 0, st);
  const int rows = n > B ? n : B;
  hipLaunchKernelGGL(kv_cache_meta_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, cu, cached_len, B, n, tok_pos, last_rows,
                     last_pos);
  LR_CHECK_LAUNCH("kv_cache_meta_kernel");
  return LR_OK;
}

int lr_launch_kv_cache_write(const u16* src, int ld, int col0, int kv_w, const int32_t* cu, const int32_t* cached_len,
                             const int32_t* slots, int B, long long slot_elems, u16* dst, int n, hipStream_t st) {
  if (n <= 0 || B <= 0) return LR_OK;
  if (kv_w < 4 || kv_w % 4 != 0 || col0 % 4 != 0 || ld % 4 != 0 || slot_elems % 4 != 0 ||
      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 7))
    LR_FAIL(LR_EINVAL, "kv cache write: rows of %d columns from column %d of %d are not 8-byte pieces", kv_w, col0, ld);
  LrProfScope prof(LR_PROF_ELEMENTWISE, 2.0 * n * kv_w * 2, st);
  hipLaunchKernelGGL(kv_cache_write_kernel, dim3(n), dim3(256), 0, st, src, ld, col0, kv_w, cu, cached_len, slots, B, slot_elems,
                     dst, n);
  LR_CHECK_LAUNCH("kv_cache_write_kernel");
  return LR_OK;
}

int lr_launch_attention_cached(const LrAttnCachedArgs& a, hipStream_t st) {
  const int B = a.B, nh = a.nh, nkv = a.nkv, hd = a.hd;
  if (B <= 0) return LR_OK;
  if (nh < 1 || nkv < 1 || nh % nkv != 0) LR_FAIL(LR_EINVAL, "cached attention: num_heads %d not a multiple of num_kv_heads %d", nh, nkv);
  const int n = a.cu_host[B];
  double work = 0;
  int max_tiles = 0;
  for (int b = 0; b < B; ++b) {
    const double c = a.cached_len_host[b], T = c + a.cu_host[b + 1] - a.cu_host[b];
    work += 4.0 * nh * hd * (a.last ? T : T * (T + 1) / 2 - c * (c + 1) / 2);
    const int tiles = ((int)T - 1) / FC_QROWS - (int)c / FC_QROWS + 1;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  if (a.generic) {
    if (hd > 256) LR_FAIL(LR_EUNSUPPORTED, "cached attention: head_dim %d > 256", hd);
    LrProfScope prof(LR_PROF_ATTN_GENERIC, work, st);
    // last: the rows a.q_rows names (each prompt's last row) of the packed q, or one compact row per prompt
    const int n_rows = a.last ? B : n;
    const long long items = (long long)n_rows * nh;
    if ((items + 3) / 4 > 0x7fffffffLL) LR_FAIL(LR_EUNSUPPORTED, "cached attention: %lld (row, head) items exceed the grid limit", items);
    hipLaunchKernelGGL(attn_cached_generic_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, a.q, a.q_ld, a.out, a.kv,
                       a.slot_elems, a.slots, a.cached_len, a.cu, B, n_rows, nh, nkv, hd, a.q_rows);
    LR_CHECK_LAUNCH("attn_cached_generic_kernel");
    return LR_OK;
  }
  if (hd != 128) LR_FAIL(LR_EUNSUPPORTED, "cached attention: the MFMA kernel needs head_dim 128 (got %d)", hd);
  if (a.q_rows) LR_FAIL(LR_EINVAL, "cached attention: the MFMA kernel takes no row list");
  if (a.q_ld % 8 != 0 || ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.kv)) & 15))
    LR_FAIL(LR_EINVAL, "cached attention: q, out and the cache must be 16-byte aligned");
  if (nh > 65535 || B > 65535) LR_FAIL(LR_EUNSUPPORTED, "cached attention: %d heads x %d prompts exceed the grid limit", nh, B);
  LrProfScope prof(LR_PROF_ATTN_MFMA, work, st);
  static bool lds_set[LR_MAX_DEVICES] = {}, lds_set_last[LR_MAX_DEVICES] = {};
  if (a.last) {
    LR_RUN(lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_cached128_kernel<true>), 2 * FC_STAGE_BYTES, lds_set_last));
    hipLaunchKernelGGL(attn_cached128_kernel<true>, dim3(1, nh, B), dim3(256), 2 * FC_STAGE_BYTES, st, a.q, a.q_ld, a.out, a.kv,
                       a.slot_elems, a.slots, a.cached_len, a.cu, nh, nkv);
    LR_CHECK_LAUNCH("attn_cached128_kernel<last>");
  } else {
    LR_RUN(lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_cached128_kernel<false>), 2 * FC_STAGE_BYTES, lds_set));
    hipLaunchKernelGGL(attn_cached128_kernel<false>, dim3(max_tiles, nh, B), dim3(256), 2 * FC_STAGE_BYTES, st, a.q, a.q_ld, a.out,
                       a.kv, a.slot_elems, a.slots, a.cached_len, a.cu, nh, nkv);
    LR_CHECK_LAUNCH("attn_cached128_kernel");
  }
  return LR_OK;
}
