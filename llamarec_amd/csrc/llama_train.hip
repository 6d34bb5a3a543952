// llama_train.hip -- the small kernels of the ranker's LoRA training step: everything between
// the big bf16 GEMMs (llama_gemm.hip) and the attention kernels (llama_attn.hip / llama_attn_bwd.hip).
//
// Replaces, on the reference side: peft 0.11.1's lora.Linear forward/backward on q_proj and v_proj
// (train_ranker.py:71-79; y = W x + (alpha/r) B A dropout(x)), torch autograd through transformers' RMSNorm,
// rotary embedding and SwiGLU (modeling_llama.py, reached from model/llm.py:89-100), the shifted cross-entropy of
// model/llm.py:116-127, clip_grad_norm_ and the optimizer step of HF Trainer (trainer/llm.py:103-136).
//
// All of these are HBM-bound row or column sweeps; none is reshaped into a GEMM except the two rank-r products
// (x A^T and dq B), which are 16-column MFMA tiles reading each activation row exactly once.
#include <stdlib.h>

#include "llama_train.h"

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef u16 u16x2 __attribute__((ext_vector_type(2)));
typedef u16 u16x8 __attribute__((ext_vector_type(8)));

// ---- dropout: counter-based, the same mask wherever (stream, row, col) is asked for ------------------------
__device__ __forceinline__ uint32_t lt_mix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// keep-probability test: true = element survives. `stream` already folds seed, pass counter and layer.
__device__ __forceinline__ bool lt_keep(uint32_t stream, uint32_t row, uint32_t col, uint32_t thresh) {
  return lt_mix(lt_mix(stream ^ (row * 0x9e3779b9u)) + col * 0x7f4a7c15u) >= thresh;
}
static uint32_t lt_drop_thresh(float p) {
  if (p <= 0.f) return 0u;
  double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

__device__ __forceinline__ float lt_block_sum(float v, float* sh) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ float lt_block_max(float v, float* sh) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// =============================================================================================
// bf16 transpose (setup): dst[c][r] = src[r][c]
// =============================================================================================
__global__ __launch_bounds__(256) void lt_transpose_kernel(const u16* src, int rows, int cols, u16* dst) {
  __shared__ u16 tile[64][66];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int r = i >> 6, c = i & 63;
    tile[r][c] = (r0 + r < rows && c0 + c < cols) ? src[(size_t)(r0 + r) * cols + c0 + c] : (u16)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int c = i >> 6, r = i & 63;
    if (r0 + r < rows && c0 + c < cols) dst[(size_t)(c0 + c) * rows + r0 + r] = tile[r][c];
  }
}
int lr_launch_transpose_bf16(const u16* src, int rows, int cols, u16* dst, hipStream_t st) {
  if (rows < 1 || cols < 1) LR_FAIL(LR_EINVAL, "transpose: rows=%d cols=%d", rows, cols);
  hipLaunchKernelGGL(lt_transpose_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, st, src, rows, cols,
                     dst);
  LR_CHECK_LAUNCH("lt_transpose_kernel");
  return LR_OK;
}

// =============================================================================================
// LoRA working copies (bf16, zero-padded to LT_RP rows) of the fp32 masters, once per loss_grad call
// =============================================================================================
// a_cat [2*LT_RP][d]      rows 0..r-1 = A_q, LT_RP..LT_RP+r-1 = A_v
// bq_t  [LT_RP][nh*hd]    bq_t[j][c] = B_q[orig(c)][j], c in the PACKED (pair-interleaved) q column order
// bv_t  [LT_RP][nkv*hd]   bv_t[j][c] = B_v[c][j]
__global__ __launch_bounds__(256) void lt_prep_lora_kernel(const float* aq, const float* bq, const float* av,
                                                           const float* bv, int r, int d, int qcols, int vcols, int hd,
                                                           u16* a_cat, u16* bq_t, u16* bv_t) {
  const int na = 2 * LT_RP * d, nq = LT_RP * qcols, nv = LT_RP * vcols;
  const int half = hd >> 1;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < na + nq + nv; i += gridDim.x * 256) {
    if (i < na) {
      const int row = i / d, c = i % d;
      const int j = row % LT_RP;
      const float* src = row < LT_RP ? aq : av;
      a_cat[i] = j < r ? f2bf(src[(size_t)j * d + c]) : (u16)0;
    } else if (i < na + nq) {
      const int k = i - na, j = k / qcols, c = k % qcols;
      const int head = c / hd, within = c % hd;
      const int orig = head * hd + (within & 1) * half + (within >> 1);
      bq_t[k] = j < r ? f2bf(bq[(size_t)orig * r + j]) : (u16)0;
    } else {
      const int k = i - na - nq, j = k / vcols, c = k % vcols;
      bv_t[k] = j < r ? f2bf(bv[(size_t)c * r + j]) : (u16)0;
    }
  }
}
int lr_launch_prep_lora(const float* aq, const float* bq, const float* av, const float* bv, int r, int d, int qcols,
                        int vcols, int hd, u16* a_cat, u16* bq_t, u16* bv_t, hipStream_t st) {
  const int total = 2 * LT_RP * d + LT_RP * (qcols + vcols);
  hipLaunchKernelGGL(lt_prep_lora_kernel, dim3(min(1024, (total + 255) / 256)), dim3(256), 0, st, aq, bq, av, bv, r, d,
                     qcols, vcols, hd, a_cat, bq_t, bv_t);
  LR_CHECK_LAUNCH("lt_prep_lora_kernel");
  return LR_OK;
}

// =============================================================================================
// rank-r products: out[n][ldo] (NT 16-column tiles from column `ocol`) = scale * drop(X)[n][K] . W[16*NT][K]^T
// =============================================================================================
// A workgroup = 16 rows; its 4 waves take the K steps (64 wide) round-robin and add their partial tiles through LDS,
// so even a 7 k-token batch is ~450 workgroups of short loops. Lane (row li, group g) reads 32 contiguous bytes of its
// row (k0 + 16 g ..): a row's 128-byte line is read by its 4 lanes and every activation byte is read once. The
// k -> (instruction, slot) assignment is the same for X and W, which is all a dot product needs.
template <int NT>
__global__ __launch_bounds__(256) void lt_skinny_kernel(const u16* __restrict__ X, int ldx, int n, int K,
                                                        const u16* __restrict__ W, u16* out, int ldo, int ocol,
                                                        float scale, uint32_t drop_stream, uint32_t drop_thresh,
                                                        float drop_scale) {
  __shared__ floatx4 part[3][NT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * 16 + li;
  const int rr = min(row, n - 1);
  const u16* xp = X + (size_t)rr * ldx + g * 16;
  floatx4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = wave * 64; k0 < K; k0 += 256) {
    u16x8 x0 = *reinterpret_cast<const u16x8*>(xp + k0);
    u16x8 x1 = *reinterpret_cast<const u16x8*>(xp + k0 + 8);
    if (drop_thresh) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = k0 + g * 16 + e;
        x0[e] = lt_keep(drop_stream, rr, c, drop_thresh) ? f2bf(bf2f(x0[e]) * drop_scale) : (u16)0;
        x1[e] = lt_keep(drop_stream, rr, c + 8, drop_thresh) ? f2bf(bf2f(x1[e]) * drop_scale) : (u16)0;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const u16* wp = W + (size_t)(t * 16 + li) * K + k0 + g * 16;
      const u16x8 w0 = *reinterpret_cast<const u16x8*>(wp);
      const u16x8 w1 = *reinterpret_cast<const u16x8*>(wp + 8);
      // D[i][j] = sum_k A[i][k] B[k][j]: A row = lane&15 (token row), B column = lane&15 (weight row)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x0), __builtin_bit_cast(bf16x8, w0),
                                                       acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x1), __builtin_bit_cast(bf16x8, w1),
                                                       acc[t], 0, 0, 0);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) part[wave - 1][t][lane] = acc[t];
  }
  __syncthreads();
  if (wave > 0) return;
  // accumulator: column = li (weight row), rows 4g + i
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const floatx4 a = acc[t] + part[0][t][lane] + part[1][t][lane] + part[2][t][lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int orow = blockIdx.x * 16 + g * 4 + i;
      if (orow < n) out[(size_t)orow * ldo + ocol + t * 16 + li] = f2bf(a[i] * scale);
    }
  }
}
int lr_launch_skinny(const u16* X, int ldx, int n, int K, const u16* W, int nt, u16* out, int ldo, int ocol, float scale,
                     uint32_t drop_stream, float drop_p, hipStream_t st) {
  if (n < 1) return LR_OK;
  if (K % 64 != 0 || ldx % 8 != 0) LR_FAIL(LR_EUNSUPPORTED, "rank-r product: K=%d must be a multiple of 64", K);
  const uint32_t th = lt_drop_thresh(drop_p);
  const float ds = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  const dim3 grid((n + 15) / 16);
  if (nt == 1)
    hipLaunchKernelGGL(lt_skinny_kernel<1>, grid, dim3(256), 0, st, X, ldx, n, K, W, out, ldo, ocol, scale, drop_stream,
                       th, ds);
  else if (nt == 2)
    hipLaunchKernelGGL(lt_skinny_kernel<2>, grid, dim3(256), 0, st, X, ldx, n, K, W, out, ldo, ocol, scale, drop_stream,
                       th, ds);
  else
    LR_FAIL(LR_EINVAL, "rank-r product: %d column tiles", nt);
  LR_CHECK_LAUNCH("lt_skinny_kernel");
  return LR_OK;
}

// =============================================================================================
// forward: qkv (plain GEMM output, packed column order) += LoRA on q and v, then rotary embedding on q and k
// =============================================================================================
// peft: result = base(x) + lora_B(lora_A(drop(x))) * scaling, every Linear output a bf16 tensor under autocast.
// A workgroup sweeps LT_ROWS rows; a thread owns 8 consecutive columns (4 rotation pairs, one 16-byte access) of all of
// them, so the r rows of B^T it needs are fetched (from L2) once per LT_ROWS activation rows.
#define LT_ROWS 4
// HASK: k_proj carries an adapter too: its t columns come from tk [n][ldtk] (column tkcol), its B^T from bk_t, and its
// delta is added before the rotation like q's
// NORM (Qwen3): between "add the delta" and "rotate" every q / k head gets its RMSNorm over head_dim, lr_launch_qk_norm_rope's
// arithmetic (a k_proj adapter's delta is normed too, as in HF); the pre-norm values, delta included, go to xsave
// [n][qcols + kcols] for lr_launch_qk_norm_bwd. A head is hd / 8 consecutive threads of one wave (hd a power of two from 16 to
// 256, the widths multiples of hd), so its square sum is a butterfly over those lanes.
template <bool HASK, bool NORM>
__global__ __launch_bounds__(256) void lt_lora_rope_fwd_kernel(u16* qkv, int n, int qw, int qcols, int kcols, int hd,
                                                               const u16* t /*[n][2*LT_RP]*/, const u16* bq_t,
                                                               const u16* bv_t, int r, float scaling,
                                                               const int32_t* tok_pos, const float* rope_cs,
                                                               const u16* tk, int ldtk, int tkcol, const u16* bk_t,
                                                               const u16* q_norm, const u16* k_norm, float eps, u16* xsave) {
  __shared__ float ts[LT_ROWS][(HASK ? 3 : 2) * LT_RP];
  __shared__ int pos[LT_ROWS];
  const int row0 = blockIdx.x * LT_ROWS;
  const int nrows = min(LT_ROWS, n - row0);
  if (threadIdx.x < LT_ROWS * 2 * LT_RP) {
    const int rr = threadIdx.x / (2 * LT_RP), j = threadIdx.x % (2 * LT_RP);
    ts[rr][j] = rr < nrows ? bf2f(t[(size_t)(row0 + rr) * 2 * LT_RP + j]) : 0.f;
  } else if (HASK && threadIdx.x < LT_ROWS * 3 * LT_RP) {
    const int i = threadIdx.x - LT_ROWS * 2 * LT_RP, rr = i / LT_RP, j = i % LT_RP;
    ts[rr][2 * LT_RP + j] = rr < nrows ? bf2f(tk[(size_t)(row0 + rr) * ldtk + tkcol + j]) : 0.f;
  }
  if (threadIdx.x < LT_ROWS) pos[threadIdx.x] = threadIdx.x < nrows ? tok_pos[row0 + threadIdx.x] : 0;
  __syncthreads();
  const int half = hd >> 1, vcols = qw - qcols - kcols;
  for (int c = threadIdx.x * 8; c < qw; c += 256 * 8) {
    const bool isq = c < qcols, isv = c >= qcols + kcols;
    float v[LT_ROWS][8];
#pragma unroll
    for (int rr = 0; rr < LT_ROWS; ++rr) {
      const u16x8 in = *reinterpret_cast<const u16x8*>(qkv + (size_t)(row0 + min(rr, nrows - 1)) * qw + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[rr][e] = bf2f(in[e]);
    }
    if (isq || isv || HASK) {
      const u16* bt = isq ? bq_t + c : isv ? bv_t + (c - qcols - kcols) : bk_t + (c - qcols);
      const int ld = isq ? qcols : isv ? vcols : kcols, toff = isq ? 0 : isv ? LT_RP : 2 * LT_RP;
      float l[LT_ROWS][8];
#pragma unroll
      for (int rr = 0; rr < LT_ROWS; ++rr)
#pragma unroll
        for (int e = 0; e < 8; ++e) l[rr][e] = 0.f;
      for (int j = 0; j < r; ++j) {
        const u16x8 b = *reinterpret_cast<const u16x8*>(bt + (size_t)j * ld);
#pragma unroll
        for (int rr = 0; rr < LT_ROWS; ++rr) {
          const float tj = ts[rr][toff + j];
#pragma unroll
          for (int e = 0; e < 8; ++e) l[rr][e] = __builtin_fmaf(tj, bf2f(b[e]), l[rr][e]);
        }
      }
#pragma unroll
      for (int rr = 0; rr < LT_ROWS; ++rr)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[rr][e] = bf2f(f2bf(v[rr][e] + bf2f(f2bf(bf2f(f2bf(l[rr][e])) * scaling))));
    }
    const int i0 = (c % hd) >> 1;
    if (NORM && !isv) {
      const u16x8 wn = *reinterpret_cast<const u16x8*>((isq ? q_norm : k_norm) + c % hd);
#pragma unroll
      for (int rr = 0; rr < LT_ROWS; ++rr) {   // every row, so that all lanes of a head take part in the shuffles
        u16x8 xb;
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xb[e] = f2bf(v[rr][e]);   // exact: the values are bf16 already
          ss = __builtin_fmaf(v[rr][e], v[rr][e], ss);
        }
        if (rr < nrows) *reinterpret_cast<u16x8*>(xsave + (size_t)(row0 + rr) * (qcols + kcols) + c) = xb;
        for (int sft = hd >> 4; sft >= 1; sft >>= 1) ss += __shfl_xor(ss, sft, 64);
        const float rstd = 1.0f / sqrtf(ss / (float)hd + eps);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[rr][e] = bf2f(rms_apply<0>(wn[e], xb[e], rstd));
      }
    }
#pragma unroll
    for (int rr = 0; rr < LT_ROWS; ++rr) {
      if (rr >= nrows) continue;
      if (!isv) {  // pairs (x1_i, x2_i) of one head: rotate-half convention in the packed layout
        const float* cs = rope_cs + ((size_t)pos[rr] * half + i0) * 2;
        const float4 c01 = *reinterpret_cast<const float4*>(cs), c23 = *reinterpret_cast<const float4*>(cs + 4);
        const float co[4] = {c01.x, c01.z, c23.x, c23.z}, si[4] = {c01.y, c01.w, c23.y, c23.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float a0 = v[rr][2 * q], a1 = v[rr][2 * q + 1];
          v[rr][2 * q] = a0 * co[q] - a1 * si[q];
          v[rr][2 * q + 1] = a1 * co[q] + a0 * si[q];
        }
      }
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(v[rr][e]);
      *reinterpret_cast<u16x8*>(qkv + (size_t)(row0 + rr) * qw + c) = o;
    }
  }
}
int lr_launch_lora_rope_fwd(u16* qkv, int n, int qw, int qcols, int kcols, int hd, const u16* t, const u16* bq_t,
                            const u16* bv_t, int r, float scaling, const int32_t* tok_pos, const float* rope_cs,
                            hipStream_t st, const u16* tk, int ldtk, int tkcol, const u16* bk_t, const LrQkNormFwd& qkn) {
  if (n < 1) return LR_OK;
  if (hd % 8 != 0 || qcols % 8 != 0 || kcols % 8 != 0 || qw % 8 != 0)
    LR_FAIL(LR_EUNSUPPORTED, "lora + rotary sweep: head_dim and projection widths must be multiples of 8");
  const bool norm = qkn.q_norm != nullptr;
  if (norm) {
    if (!lr_qk_norm_head_dim_ok(hd) || qcols % hd != 0 || kcols % hd != 0)
      LR_FAIL(LR_EUNSUPPORTED, "lora + q/k norm + rotary sweep: head_dim %d (a power of two from 16 to 256)", hd);
    if (!qkn.k_norm || !qkn.xsave) LR_FAIL(LR_EINVAL, "lora + q/k norm + rotary sweep: null k norm or save buffer");
  }
  const dim3 grid((n + LT_ROWS - 1) / LT_ROWS);
#define LT_ROPE_FWD(HASK, NORM)                                                                                            \
  hipLaunchKernelGGL((lt_lora_rope_fwd_kernel<HASK, NORM>), grid, dim3(256), 0, st, qkv, n, qw, qcols, kcols, hd, t, bq_t, \
                     bv_t, r, scaling, tok_pos, rope_cs, tk, ldtk, tkcol, bk_t, qkn.q_norm, qkn.k_norm, qkn.eps, qkn.xsave)
  if (bk_t && norm) LT_ROPE_FWD(true, true);
  else if (bk_t) LT_ROPE_FWD(true, false);
  else if (norm) LT_ROPE_FWD(false, true);
  else LT_ROPE_FWD(false, false);
#undef LT_ROPE_FWD
  LR_CHECK_LAUNCH("lt_lora_rope_fwd_kernel");
  return LR_OK;
}

// =============================================================================================
// backward of Qwen3's per-head q / k RMSNorm (frozen weights: no weight gradient)
// =============================================================================================
// In place on the q and k columns of dqkv [n][ld] (nq + nk heads of hd columns from column 0 on), which hold the gradient
// w.r.t. the normed, unrotated q / k (lr_launch_attention_bwd's output); x [n][ldx] = the pre-norm values the forward saved.
// Per (row, head), with g = w .* dy and xh = x * rstd:  dx = rstd * (g - xh * mean(xh .* g)), formed in fp32 as
// rstd * (g - x * (rstd^2 * sum(x .* g) / hd)) and rounded once. lr_launch_qk_norm_rope's thread layout: a thread owns 8 columns, a head is
// hd / 8 lanes, both sums are butterflies over them. Every element has one owner and nothing is added atomically: two runs
// give the same bits.
template <int HD>
__global__ __launch_bounds__(256) void lt_qk_norm_bwd_kernel(u16* dqk, size_t total, int per_row, int ld, const u16* x, int ldx,
                                                             int nq, const u16* q_norm, const u16* k_norm, float eps) {
  constexpr int L = HD / 8;
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = id < total;
  const size_t row = live ? id / per_row : 0;
  const int chunk = live ? (int)(id % per_row) : 0;
  const int head = chunk / L, part = chunk % L;
  u16* p = dqk + row * ld + (size_t)chunk * 8;
  u16x8 xv = {0, 0, 0, 0, 0, 0, 0, 0}, dy = xv, w = xv;
  if (live) {
    xv = *reinterpret_cast<const u16x8*>(x + row * ldx + (size_t)chunk * 8);
    dy = *reinterpret_cast<const u16x8*>(p);
    w = *reinterpret_cast<const u16x8*>((head < nq ? q_norm : k_norm) + part * 8);
  }
  float xf[8], g[8], ss = 0.f, sg = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xf[j] = bf2f(xv[j]);
    g[j] = bf2f(w[j]) * bf2f(dy[j]);
    ss = __builtin_fmaf(xf[j], xf[j], ss);
    sg = __builtin_fmaf(xf[j], g[j], sg);
  }
#pragma unroll
  for (int s = L / 2; s >= 1; s >>= 1) {
    ss += __shfl_xor(ss, s, 64);
    sg += __shfl_xor(sg, s, 64);
  }
  if (!live) return;
  const float rstd = 1.0f / sqrtf(ss / (float)HD + eps);
  const float m = rstd * rstd * (sg / (float)HD);
  u16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2bf(rstd * (g[j] - xf[j] * m));
  *reinterpret_cast<u16x8*>(p) = o;
}

int lr_launch_qk_norm_bwd(u16* dqk, int rows, int ld, const u16* x, int ldx, int nq, int nk, int hd, const u16* q_norm,
                          const u16* k_norm, float eps, hipStream_t st) {
  if (rows <= 0 || nq + nk == 0) return LR_OK;
  if (!lr_qk_norm_head_dim_ok(hd)) LR_FAIL(LR_EUNSUPPORTED, "q/k norm backward: head_dim %d (a power of two from 16 to 256)", hd);
  if (!dqk || !x || nq < 0 || nk < 0 || (nq > 0 && !q_norm) || (nk > 0 && !k_norm) || ld % 8 != 0 || ldx % 8 != 0 ||
      (long long)(nq + nk) * hd > ld || (long long)(nq + nk) * hd > ldx ||
      ((reinterpret_cast<uintptr_t>(dqk) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(q_norm) |
        reinterpret_cast<uintptr_t>(k_norm)) & 15))
    LR_FAIL(LR_EINVAL, "q/k norm backward: bad argument (nq %d, nk %d, head_dim %d, row strides %d / %d; 16-byte aligned pointers)",
            nq, nk, hd, ld, ldx);
  const int per_row = (nq + nk) * (hd / 8);
  const size_t total = (size_t)rows * per_row;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffu) LR_FAIL(LR_EUNSUPPORTED, "q/k norm backward: %d rows exceed the grid limit", rows);
#define LT_QKN_CASE(HD)                                                                                                    \
  case HD:                                                                                                                 \
    hipLaunchKernelGGL(lt_qk_norm_bwd_kernel<HD>, dim3((unsigned)blocks), dim3(256), 0, st, dqk, total, per_row, ld, x, ldx, \
                       nq, q_norm, k_norm, eps);                                                                           \
    break;
  switch (hd) {
    LT_QKN_CASE(16) LT_QKN_CASE(32) LT_QKN_CASE(64) LT_QKN_CASE(128) LT_QKN_CASE(256)
  }
#undef LT_QKN_CASE
  LR_CHECK_LAUNCH("lt_qk_norm_bwd_kernel");
  return LR_OK;
}

// =============================================================================================
// backward of the rotary embedding (generic attention path only; the MFMA passes rotate in their epilogues)
// =============================================================================================
__global__ __launch_bounds__(256) void lt_rope_bwd_kernel(u16* dqkv, int n, int qw, int rot_cols, int hd,
                                                          const int32_t* tok_pos, const float* rope_cs) {
  const int per_row = rot_cols / 8;
  const int half = hd >> 1;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n * per_row; i += (size_t)gridDim.x * 256) {
    const int row = (int)(i / per_row), c = (int)(i % per_row) * 8;
    u16* x = dqkv + (size_t)row * qw + c;
    const u16x8 in = *reinterpret_cast<const u16x8*>(x);
    const float* cs = rope_cs + ((size_t)tok_pos[row] * half + ((c % hd) >> 1)) * 2;
    u16x8 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v0 = bf2f(in[2 * q]), v1 = bf2f(in[2 * q + 1]), co = cs[2 * q], si = cs[2 * q + 1];
      o[2 * q] = f2bf(v0 * co + v1 * si);  // transpose of the rotation
      o[2 * q + 1] = f2bf(v1 * co - v0 * si);
    }
    *reinterpret_cast<u16x8*>(x) = o;
  }
}
int lr_launch_rope_bwd(u16* dqkv, int n, int qw, int rot_cols, int hd, const int32_t* tok_pos, const float* rope_cs,
                       hipStream_t st) {
  if (n < 1 || rot_cols < 1) return LR_OK;
  // a thread rotates 4 pairs of one head with one 16-byte access, and reads their 8 table entries in a row
  if (hd % 8 != 0 || rot_cols % hd != 0 || qw % 8 != 0 || rot_cols > qw)
    LR_FAIL(LR_EUNSUPPORTED, "rotary backward: head_dim %d must be a multiple of 8 and divide the %d rotated columns of %d (a multiple of 8)",
            hd, rot_cols, qw);
  const size_t total = (size_t)n * (rot_cols / 8);
  hipLaunchKernelGGL(lt_rope_bwd_kernel, dim3((unsigned)min((size_t)8192, (total + 255) / 256)), dim3(256), 0, st, dqkv,
                     n, qw, rot_cols, hd, tok_pos, rope_cs);
  LR_CHECK_LAUNCH("lt_rope_bwd_kernel");
  return LR_OK;
}

// =============================================================================================
// token reductions: out[j][c] += scale * sum_tok T[tok][tcol + j] * drop(X)[tok][c]      (d B, d A)
// =============================================================================================
// M = the adapter's rank (one or two 16-row tiles of T's columns), N = activation columns, K = tokens: both operands
// are indexed k-major in memory, so a lane gathers its 8 tokens with 2-byte loads (16 lanes = 32 contiguous bytes;
// T is a few hundred KB and stays in L2, X is read exactly once). A wave owns 64 columns (4 tiles sharing the T
// fragment), a workgroup 256, and walks one chunk of tokens; partial sums leave with one fp32 atomic per (j, c).
//   layout 0: out_t[j * cols + c]                          (d A: [r][hidden], tile t -> out0 / out1)
//   layout 1: out0[c * r + j]                              (d B_v: [cols][r])
//   layout 2: out0[orig(c) * r + j], packed -> HF column   (d B_q, d B_k)
//   layout 3: X = the interleaved gate/up gradient (16 gate columns, 16 up columns, ...): tile 0 keeps the gate columns
//             (out0[f_col * r + j]), tile 1 the up columns (out1); a null out0 / out1 = that adapter is not trained
// Where a (column block, token chunk) workgroup's accumulators leave (column = activation column li of the tile, rows j = 4g + i).
// Default: one fp32 atomic per (j, c) into the gradient. DET (lr_llama_lora_set_deterministic): out0 / out1 are chunk 0's
// partial tiles instead, laid out like the gradient they stand for (E elements each, chunk k's pair NJ * E floats further on), and
// the scaled tile is STORED to its chunk's: 16 lanes = 64 contiguous bytes per j in layout 0; in the [column][r] layouts a lane's
// four j are adjacent, so with r a multiple of 4 a lane stores 16 bytes and a 16-lane group r * 64 contiguous ones.
// lt_tn_fold_kernel then adds the chunks in ascending order. (A macro, not a function: the default instantiations of both bodies
// compile to the instructions they had before the mode existed.)
#define LT_TN_STORE()                                                                                     \
  const int half = hd >> 1;                                                                               \
  _Pragma("unroll") for (int a = 0; a < NJ; ++a) {                                                        \
    float* out = a == 0 ? out0 : out1;                                                                    \
    if (!out) continue; /* a tile whose adapter is not trained */                                         \
    if (DET) out += (size_t)blockIdx.y * NJ * ((size_t)r * cols >> (layout == 3));                        \
    _Pragma("unroll") for (int ct = 0; ct < 4; ++ct) {                                                    \
      const int c = c0 + ct * 16 + li;                                                                    \
      if (DET && layout != 0 && (r & 3) == 0) {                                                           \
        if (g * 4 >= r || (layout == 3 && ((c >> 4) & 1) != a)) continue;                                 \
        int row = c;                                                                                      \
        if (layout == 3) row = (c >> 5) * 16 + (c & 15);                                                  \
        else if (layout == 2) row = c / hd * hd + (c % hd & 1) * half + (c % hd >> 1);                    \
        *reinterpret_cast<floatx4*>(out + (size_t)row * r + g * 4) = acc[a][ct] * scale;                  \
        continue;                                                                                         \
      }                                                                                                   \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                     \
        const int j = g * 4 + i;                                                                          \
        if (j >= r) continue;                                                                             \
        size_t at;                                                                                        \
        if (layout == 0) {                                                                                \
          at = (size_t)j * cols + c;                                                                      \
        } else if (layout == 1) {                                                                         \
          at = (size_t)c * r + j;                                                                         \
        } else if (layout == 3) {                                                                         \
          if (((c >> 4) & 1) != a) continue;                                                              \
          at = (size_t)((c >> 5) * 16 + (c & 15)) * r + j;                                                \
        } else {                                                                                          \
          const int head = c / hd, within = c % hd;                                                       \
          at = (size_t)(head * hd + (within & 1) * half + (within >> 1)) * r + j;                         \
        }                                                                                                 \
        if (DET) out[at] = acc[a][ct][i] * scale;                                                         \
        else atomicAdd(out + at, acc[a][ct][i] * scale);                                                  \
      }                                                                                                   \
    }                                                                                                     \
  }
template <int NJ, bool DET>
__global__ __launch_bounds__(256) void lt_tn_kernel(const u16* __restrict__ T, int ldt, int tcol,
                                                    const u16* __restrict__ X, int ldx, int n, int cols, int chunk,
                                                    float scale, float* out0, float* out1, int r, int layout, int hd,
                                                    uint32_t drop_stream, uint32_t drop_thresh, float drop_scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * 256 + wave * 64;
  if (c0 >= cols) return;
  const int t0 = blockIdx.y * chunk, t1 = min(n, t0 + chunk);
  floatx4 acc[NJ][4];
#pragma unroll
  for (int a = 0; a < NJ; ++a)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[a][ct] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = t0; k0 < t1; k0 += 32) {
    u16x8 tf[NJ], xf[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int tok = k0 + g * 8 + e;
      const bool ok = tok < t1;
      const size_t tr = (size_t)min(tok, n - 1);
#pragma unroll
      for (int a = 0; a < NJ; ++a) tf[a][e] = ok ? T[tr * ldt + tcol + a * 16 + li] : (u16)0;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int c = c0 + ct * 16 + li;
        u16 v = X[tr * ldx + c];
        if (drop_thresh) v = lt_keep(drop_stream, (uint32_t)tr, c, drop_thresh) ? f2bf(bf2f(v) * drop_scale) : (u16)0;
        xf[ct][e] = v;
      }
    }
#pragma unroll
    for (int a = 0; a < NJ; ++a)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        acc[a][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, tf[a]),
                                                             __builtin_bit_cast(bf16x8, xf[ct]), acc[a][ct], 0, 0, 0);
  }
  LT_TN_STORE()
}
// The same reduction with both operands staged through LDS: 16-byte global loads in memory order (8 lanes per token row of the
// wave's 64 columns, 2 lanes per row of T's 16 columns), then ds_read_b64_tr_b16 hands every lane its 8 consecutive TOKENS of one
// column -- the k-major fragment the 2-byte gathers above assemble with 32 vector loads per 4 MFMAs (rocprofv3, round 5: 166 us
// per call at 7 k tokens against ~15 us of HBM time for X). Same fragments, same MFMA order: bit-identical sums. The next
// 32-token step's loads are in flight while this one's products run; the LDS tiles are wave-private (no barrier).
// Needs 16-byte-aligned rows of X and T (launch_tn checks and otherwise takes the kernel above).
template <int NJ, bool DET>
__global__ __launch_bounds__(256) void lt_tn_lds_kernel(const u16* __restrict__ T, int ldt, int tcol,
                                                        const u16* __restrict__ X, int ldx, int n, int cols, int chunk,
                                                        float scale, float* out0, float* out1, int r, int layout, int hd,
                                                        uint32_t drop_stream, uint32_t drop_thresh, float drop_scale) {
  constexpr int XS = 144, TS = NJ * 32 + 16;                    // LDS row strides in bytes (16-byte multiples, not 128: banks)
  __shared__ __attribute__((aligned(16))) char lds[4 * (32 * XS + 32 * TS)];
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * 256 + wave * 64;
  if (c0 >= cols) return;                                       // whole waves leave: EXEC stays all ones for the transposed reads
  const int t0 = blockIdx.y * chunk, t1 = min(n, t0 + chunk);
  char* const xs = lds + wave * (32 * XS + 32 * TS);
  char* const ts = xs + 32 * XS;
  floatx4 acc[NJ][4];
#pragma unroll
  for (int a = 0; a < NJ; ++a)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[a][ct] = floatx4{0.f, 0.f, 0.f, 0.f};
  u32x4 xr[4], tr_[NJ];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t row = (size_t)min(k0 + i * 8 + (lane >> 3), n - 1);
      xr[i] = *reinterpret_cast<const u32x4*>(X + row * ldx + c0 + (lane & 7) * 8);
    }
#pragma unroll
    for (int a = 0; a < NJ; ++a) {
      const size_t row = (size_t)min(k0 + (lane >> 1), n - 1);
      tr_[a] = *reinterpret_cast<const u32x4*>(T + row * ldt + tcol + a * 16 + (lane & 1) * 8);
    }
  };
  fetch(t0);
  for (int k0 = t0; k0 < t1; k0 += 32) {
    // this step's rows -> LDS (dropout on X and the zero rows of T past the chunk's end applied on the way)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 v = xr[i];
      if (drop_thresh) {
        const uint32_t row = (uint32_t)min(k0 + i * 8 + (lane >> 3), n - 1);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int c = c0 + (lane & 7) * 8 + 2 * w;
          const u16 lo = lt_keep(drop_stream, row, c, drop_thresh) ? f2bf(bf2f((u16)(v[w] & 0xffff)) * drop_scale) : (u16)0;
          const u16 hi = lt_keep(drop_stream, row, c + 1, drop_thresh) ? f2bf(bf2f((u16)(v[w] >> 16)) * drop_scale) : (u16)0;
          v[w] = (unsigned)lo | ((unsigned)hi << 16);
        }
      }
      *reinterpret_cast<u32x4*>(xs + (i * 8 + (lane >> 3)) * XS + (lane & 7) * 16) = v;
    }
#pragma unroll
    for (int a = 0; a < NJ; ++a) {
      const bool ok = k0 + (lane >> 1) < t1;
      *reinterpret_cast<u32x4*>(ts + (lane >> 1) * TS + a * 32 + (lane & 1) * 16) = ok ? tr_[a] : u32x4{0, 0, 0, 0};
    }
    if (k0 + 32 < t1) fetch(k0 + 32);
    // lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a 4 x 16 block; lane i receives column i of the 4 rows
    const int q = li >> 2, p = li & 3;
    u16x8 tf[NJ], xf[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 8 * g + 4 * h + q;
#pragma unroll
      for (int a = 0; a < NJ; ++a) {
        const s16x4 t4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(ts + row * TS + (a * 16 + 4 * p) * 2));
#pragma unroll
        for (int e = 0; e < 4; ++e) tf[a][4 * h + e] = (u16)t4[e];
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const s16x4 x4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(xs + row * XS + (ct * 16 + 4 * p) * 2));
#pragma unroll
        for (int e = 0; e < 4; ++e) xf[ct][4 * h + e] = (u16)x4[e];
      }
    }
#pragma unroll
    for (int a = 0; a < NJ; ++a)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        acc[a][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, tf[a]),
                                                             __builtin_bit_cast(bf16x8, xf[ct]), acc[a][ct], 0, 0, 0);
  }
  LT_TN_STORE()
}
static int lt_tn_forced_chunk() {
  static int forced = -1;
  if (forced < 0) {
    const char* e = getenv("LR_TN_CHUNK");  // tuning knob: tokens per workgroup (multiple of 32)
    forced = e ? atoi(e) / 32 * 32 : 0;
  }
  return forced;
}
static int lt_tn_chunk(int n) {
  const int forced = lt_tn_forced_chunk();
  if (forced > 0) return forced;
  return n >= 4096 ? 256 : (n >= 512 ? 128 : 32);  // 7 k tokens: 128-256 measured best (512: too few workgroups)
}
// Deterministic mode's fold: out[e] += part[0][e] + part[1][e] + ... in ascending chunk order -- ONE read-modify-write of the
// gradient per element, so a zeroed and an accumulating buffer both work. part: [chunks][tiles][E] as lt_tn_store left it,
// E a multiple of 4; a thread owns 4 adjacent elements (16-byte accesses, whole lines per wave), blockIdx.y = the tile.
__global__ __launch_bounds__(256) void lt_tn_fold_kernel(const float* __restrict__ part, size_t stride, int chunks, size_t E,
                                                         float* out0, float* out1) {
  float* out = blockIdx.y == 0 ? out0 : out1;
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (!out || e >= E) return;
  const float* p = part + blockIdx.y * E + e;
  floatx4 s = *reinterpret_cast<const floatx4*>(p);
#pragma unroll 4
  for (int k = 1; k < chunks; ++k) s += *reinterpret_cast<const floatx4*>(p + k * stride);
  floatx4* o = reinterpret_cast<floatx4*>(out + e);
  *o = *o + s;
}
// floats of partial tiles one deterministic token reduction over AT MOST n tokens may need. The chunk count is not monotonic in
// n (511 tokens: 16 chunks of 32; 512: 4 of 128), and a workspace sized for max_tokens serves every smaller batch.
size_t lr_lora_tn_partial_floats(int nj, int n, int cols, int r, int layout) {
  if (n < 1) return 0;
  size_t chunks;
  if (const int forced = lt_tn_forced_chunk()) {
    chunks = ((size_t)n + forced - 1) / forced;
  } else {
    chunks = (size_t)(min(n, 511) + 31) / 32;
    if (n >= 512) chunks = max(chunks, (size_t)(min(n, 4095) + 127) / 128);
    if (n >= 4096) chunks = max(chunks, ((size_t)n + 255) / 256);
  }
  return chunks * nj * ((size_t)r * cols >> (layout == 3));
}
// det_part != nullptr: deterministic mode, with lr_lora_tn_partial_floats floats there that no launch which may run at the same
// time uses. The chunk length stays a function of n alone: the summation tree is fixed by the batch.
static int launch_tn(int nj, const u16* T, int ldt, int tcol, const u16* X, int ldx, int n, int cols, float scale,
                     float* out0, float* out1, int r, int layout, int hd, uint32_t drop_stream, float drop_p,
                     hipStream_t st, float* det_part) {
  if (n < 1) return LR_OK;
  if (cols % 64 != 0) LR_FAIL(LR_EUNSUPPORTED, "token reduction: %d columns (must be a multiple of 64)", cols);
  const int chunk = lt_tn_chunk(n);
  const dim3 grid((cols + 255) / 256, (n + chunk - 1) / chunk);
  const uint32_t th = lt_drop_thresh(drop_p);
  const float ds = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  static int gather = -1;   // LR_TN_GATHER=1: the 2-byte gather kernel whatever the alignment (the bit-identity test's other side)
  if (gather < 0) {
    const char* e = getenv("LR_TN_GATHER");
    gather = e && e[0] == '1';
  }
  const bool aligned = !gather && ((uintptr_t)X & 15) == 0 && ((uintptr_t)(T + tcol) & 15) == 0 && ldx % 8 == 0 && ldt % 8 == 0;
#define LT_TN_LAUNCH(KERNEL, NJ, DET, O0, O1)                                                                              \
  hipLaunchKernelGGL((KERNEL<NJ, DET>), grid, dim3(256), 0, st, T, ldt, tcol, X, ldx, n, cols, chunk, scale, O0, O1, r, layout, \
                     hd, drop_stream, th, ds)
  if (det_part) {
    if (nj == 1) out1 = nullptr;
    const size_t E = (size_t)r * cols >> (layout == 3);
    if ((((uintptr_t)det_part | (uintptr_t)out0 | (uintptr_t)out1) & 15) != 0)
      LR_FAIL(LR_EUNSUPPORTED, "deterministic token reduction: gradients and partial tiles must be 16-byte aligned");
    float *p0 = out0 ? det_part : nullptr, *p1 = out1 ? det_part + E : nullptr;
    if (aligned && nj == 1) LT_TN_LAUNCH(lt_tn_lds_kernel, 1, true, p0, p1);
    else if (aligned) LT_TN_LAUNCH(lt_tn_lds_kernel, 2, true, p0, p1);
    else if (nj == 1) LT_TN_LAUNCH(lt_tn_kernel, 1, true, p0, p1);
    else LT_TN_LAUNCH(lt_tn_kernel, 2, true, p0, p1);
    LR_CHECK_LAUNCH("lt_tn_kernel");
    hipLaunchKernelGGL(lt_tn_fold_kernel, dim3((unsigned)((E / 4 + 255) / 256), nj), dim3(256), 0, st, det_part, nj * E,
                       (int)grid.y, E, out0, out1);
    LR_CHECK_LAUNCH("lt_tn_fold_kernel");
    return LR_OK;
  }
  if (aligned && nj == 1) LT_TN_LAUNCH(lt_tn_lds_kernel, 1, false, out0, out1);
  else if (aligned) LT_TN_LAUNCH(lt_tn_lds_kernel, 2, false, out0, out1);
  else if (nj == 1) LT_TN_LAUNCH(lt_tn_kernel, 1, false, out0, out1);
  else LT_TN_LAUNCH(lt_tn_kernel, 2, false, out0, out1);
#undef LT_TN_LAUNCH
  LR_CHECK_LAUNCH("lt_tn_kernel");
  return LR_OK;
}
// d B_q += scaling * dq_pre^T t_q,  d B_v += scaling * dv^T t_v      (dqkv: gradient w.r.t. the UNROTATED q, k, v)
int lr_launch_lora_db(const u16* dqkv, int n, int qw, int qcols, int kcols, int hd, const u16* t, int r, float scaling,
                      float* dbq, float* dbv, hipStream_t st, float* det_part) {
  int rc = launch_tn(1, t, 2 * LT_RP, 0, dqkv, qw, n, qcols, scaling, dbq, nullptr, r, 2, hd, 0, 0.f, st, det_part);
  if (rc) return rc;
  return launch_tn(1, t, 2 * LT_RP, LT_RP, dqkv + qcols + kcols, qw, n, qw - qcols - kcols, scaling, dbv, nullptr, r, 1,
                   hd, 0, 0.f, st, det_part);
}
// d A_q[j][c], d A_v[j][c] += sum_rows dt[row][j (+LT_RP)] * drop(xn)[row][c]   (dt already carries `scaling`)
int lr_launch_lora_da(const u16* xn, int n, int d, const u16* dt, int r, uint32_t drop_stream, float drop_p, float* daq,
                      float* dav, hipStream_t st, float* det_part) {
  return launch_tn(2, dt, 2 * LT_RP, 0, xn, d, n, d, 1.0f, daq, dav, r, 0, 0, drop_stream, drop_p, st, det_part);
}

int lr_launch_lora_tn(int nj, const u16* T, int ldt, int tcol, const u16* X, int ldx, int n, int cols, float scale,
                      float* out0, float* out1, int r, int layout, int hd, uint32_t drop_stream, float drop_p,
                      hipStream_t st, float* det_part) {
  return launch_tn(nj, T, ldt, tcol, X, ldx, n, cols, scale, out0, out1, r, layout, hd, drop_stream, drop_p, st, det_part);
}

// =============================================================================================
// adapters on any Linear (k, o, gate, up, down): working copies, and the rank-r expand-add sweep
// =============================================================================================
// One module's bf16 working copies from its fp32 masters (peft's A [r][in], B [out][r]):
//   a_w [LT_RP][in]      rows >= r zero
//   b_t [LT_RP][ldb]     b_t[j][dest(o)] = B[o][j]: the transpose, in the column order of the activation it is added to
//     perm 0 plain; 1 rotary pair interleave within each head (q, k); 2 / 3 the gate / up columns of the interleaved
//     gate-up activation (ldb = 2 * out; the other half's columns of these rows are never written and stay zero from
//     the state's initial memset: the [2*LT_RP][2f] pair is then a plain weight for the d t product over d gu)
__global__ __launch_bounds__(256) void lt_prep_module_kernel(const float* a, const float* b, int r, int in, int out,
                                                             int perm, int hd, u16* a_w, u16* b_t, int ldb) {
  const int na = LT_RP * in, nb = LT_RP * out;
  const int half = hd >> 1;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < na + nb; i += gridDim.x * 256) {
    if (i < na) {
      const int j = i / in, c = i % in;
      a_w[i] = j < r ? f2bf(a[(size_t)j * in + c]) : (u16)0;
    } else {
      const int k = i - na, j = k / out, c = k % out;
      int orig = c, dest = c;
      if (perm == 1) {
        const int head = c / hd, within = c % hd;
        orig = head * hd + (within & 1) * half + (within >> 1);
      } else if (perm >= 2) {
        dest = (c >> 4) * 32 + (perm == 3 ? 16 : 0) + (c & 15);
      }
      b_t[(size_t)j * ldb + dest] = j < r ? f2bf(b[(size_t)orig * r + j]) : (u16)0;
    }
  }
}
int lr_launch_prep_module(const float* a, const float* b, int r, int in, int out, int perm, int hd, u16* a_w, u16* b_t,
                          int ldb, hipStream_t st) {
  const int total = LT_RP * (in + out);
  hipLaunchKernelGGL(lt_prep_module_kernel, dim3(min(1024, (total + 255) / 256)), dim3(256), 0, st, a, b, r, in, out,
                     perm, hd, a_w, b_t, ldb);
  LR_CHECK_LAUNCH("lt_prep_module_kernel");
  return LR_OK;
}

// Y[row][c] = bf16(Y[row][c] + keep(row, c) * bf16(bf16(sum_j T[row][tcol + j] * W[j][c]) * s))
//   forward  (Y = xmid / x_next behind o_proj's / down_proj's residual GEMM, T = drop(X) A^T, W = B^T, s = alpha / r, no mask):
//            the adapter's delta, rounded like peft's bf16 lora_B output and its scaling under autocast
//   backward (Y = the gradient of the adapter's INPUT, T = d t, W = A, s = 1 / (1 - p), mask = the input's dropout mask)
// (k's and gate / up's deltas ride in lt_lora_rope_fwd_kernel, lt_swiglu_lora_fwd_kernel and the norm backward's LoRA arm.)
// A workgroup sweeps LT_ROWS rows; a thread owns 8 consecutive columns (one 16-byte access, whole 128-byte lines per 8 lanes) of
// all of them, so the r rows of W it needs come from L2 once per LT_ROWS activation rows -- lt_lora_rope_fwd_kernel's shape.
__global__ __launch_bounds__(256) void lt_lora_expand_kernel(u16* Y, int ldy, int n, int cols, const u16* T, int ldt,
                                                             int tcol, const u16* W, int r, float s,
                                                             uint32_t drop_stream, uint32_t drop_thresh) {
  __shared__ float ts[LT_ROWS][LT_RP];
  const int row0 = blockIdx.x * LT_ROWS;
  const int nrows = min(LT_ROWS, n - row0);
  if (threadIdx.x < LT_ROWS * LT_RP) {
    const int rr = threadIdx.x / LT_RP, j = threadIdx.x % LT_RP;
    ts[rr][j] = rr < nrows ? bf2f(T[(size_t)(row0 + rr) * ldt + tcol + j]) : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x * 8; c < cols; c += 256 * 8) {
    float l[LT_ROWS][8];
#pragma unroll
    for (int rr = 0; rr < LT_ROWS; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) l[rr][e] = 0.f;
    for (int j = 0; j < r; ++j) {
      const u16x8 b = *reinterpret_cast<const u16x8*>(W + (size_t)j * cols + c);
#pragma unroll
      for (int rr = 0; rr < LT_ROWS; ++rr) {
        const float tj = ts[rr][j];
#pragma unroll
        for (int e = 0; e < 8; ++e) l[rr][e] = __builtin_fmaf(tj, bf2f(b[e]), l[rr][e]);
      }
    }
#pragma unroll
    for (int rr = 0; rr < LT_ROWS; ++rr) {
      if (rr >= nrows) continue;
      u16* yp = Y + (size_t)(row0 + rr) * ldy + c;
      const u16x8 in = *reinterpret_cast<const u16x8*>(yp);
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool keep = !drop_thresh || lt_keep(drop_stream, row0 + rr, c + e, drop_thresh);
        o[e] = keep ? f2bf(bf2f(in[e]) + bf2f(f2bf(bf2f(f2bf(l[rr][e])) * s))) : in[e];
      }
      *reinterpret_cast<u16x8*>(yp) = o;
    }
  }
}
int lr_launch_lora_expand(u16* Y, int ldy, int n, int cols, const u16* T, int ldt, int tcol, const u16* W, int r, float s,
                          uint32_t drop_stream, float drop_p, hipStream_t st) {
  if (n < 1) return LR_OK;
  if (cols % 8 != 0 || ldy % 8 != 0 || ((uintptr_t)Y & 15) != 0)
    LR_FAIL(LR_EUNSUPPORTED, "rank-r expand-add: cols=%d ld=%d", cols, ldy);
  hipLaunchKernelGGL(lt_lora_expand_kernel, dim3((n + LT_ROWS - 1) / LT_ROWS), dim3(256), 0, st, Y, ldy, n, cols, T, ldt,
                     tcol, W, r, s, drop_stream, lt_drop_thresh(drop_p));
  LR_CHECK_LAUNCH("lt_lora_expand_kernel");
  return LR_OK;
}

// =============================================================================================
// SwiGLU on the interleaved gate/up layout of the packed wgu GEMM (16 gate columns, 16 up columns, ...)
// =============================================================================================
// a thread owns 8 consecutive h columns = 16 bytes of gate, 16 of up, 16 of h
__global__ __launch_bounds__(256) void lt_swiglu_fwd_kernel(const u16* gu, u16* h, size_t total8 /* n*f/8 */, int f) {
  const int per_row = f >> 3;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += (size_t)gridDim.x * 256) {
    const size_t row = i / per_row;
    const int c = (int)(i % per_row) * 8;
    const u16* p = gu + row * 2 * f + (c >> 4) * 32 + (c & 15);
    const u16x8 g = *reinterpret_cast<const u16x8*>(p), u = *reinterpret_cast<const u16x8*>(p + 16);
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = swiglu_bf16(bf2f(g[e]), bf2f(u[e]));
    *reinterpret_cast<u16x8*>(h + row * f + c) = o;
  }
}
// The same pass with the gate / up adapters' delta: gu += s * t W (t [n][ldt] from column tcol: 16 gate ranks, 16 up ranks;
// W [2*LT_RP][2f] = their B^T in gu's interleaved column order), written BACK to gu -- the saved pre-activation values the
// backward differentiates at -- and h = swiglu of the sum. Rounded like lt_lora_rope_fwd_kernel's q / v delta. A workgroup
// takes LT_ROWS rows so that the 2r rows of W a thread needs come from L2 once per LT_ROWS activation rows.
__global__ __launch_bounds__(256) void lt_swiglu_lora_fwd_kernel(u16* gu, u16* h, int n, int f, const u16* t, int ldt, int tcol,
                                                                 const u16* W, int r, float s) {
  __shared__ float ts[LT_ROWS][2 * LT_RP];
  const int row0 = blockIdx.x * LT_ROWS;
  const int nrows = min(LT_ROWS, n - row0);
  if (threadIdx.x < LT_ROWS * 2 * LT_RP) {
    const int rr = threadIdx.x / (2 * LT_RP), j = threadIdx.x % (2 * LT_RP);
    ts[rr][j] = rr < nrows ? bf2f(t[(size_t)(row0 + rr) * ldt + tcol + j]) : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x * 8; c < f; c += 256 * 8) {
    const int pc = (c >> 4) * 32 + (c & 15);  // gate columns pc .. pc+7, up columns pc+16 .. pc+23
    float lg[LT_ROWS][8], lu[LT_ROWS][8];
#pragma unroll
    for (int rr = 0; rr < LT_ROWS; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) lg[rr][e] = lu[rr][e] = 0.f;
    for (int j = 0; j < r; ++j) {
      const u16x8 bg = *reinterpret_cast<const u16x8*>(W + (size_t)j * 2 * f + pc);
      const u16x8 bu = *reinterpret_cast<const u16x8*>(W + (size_t)(LT_RP + j) * 2 * f + pc + 16);
#pragma unroll
      for (int rr = 0; rr < LT_ROWS; ++rr) {
        const float tg = ts[rr][j], tu = ts[rr][LT_RP + j];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          lg[rr][e] = __builtin_fmaf(tg, bf2f(bg[e]), lg[rr][e]);
          lu[rr][e] = __builtin_fmaf(tu, bf2f(bu[e]), lu[rr][e]);
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < LT_ROWS; ++rr) {
      if (rr >= nrows) continue;
      u16* p = gu + (size_t)(row0 + rr) * 2 * f + pc;
      u16x8 g = *reinterpret_cast<const u16x8*>(p), u = *reinterpret_cast<const u16x8*>(p + 16);
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        g[e] = f2bf(bf2f(g[e]) + bf2f(f2bf(bf2f(f2bf(lg[rr][e])) * s)));
        u[e] = f2bf(bf2f(u[e]) + bf2f(f2bf(bf2f(f2bf(lu[rr][e])) * s)));
        o[e] = swiglu_bf16(bf2f(g[e]), bf2f(u[e]));
      }
      *reinterpret_cast<u16x8*>(p) = g;
      *reinterpret_cast<u16x8*>(p + 16) = u;
      *reinterpret_cast<u16x8*>(h + (size_t)(row0 + rr) * f + c) = o;
    }
  }
}
int lr_launch_swiglu_lora_fwd(u16* gu, u16* h, int n, int f, const u16* t, int ldt, int tcol, const u16* W, int r, float s,
                              hipStream_t st) {
  if (n < 1) return LR_OK;
  if (f % 16 != 0) LR_FAIL(LR_EUNSUPPORTED, "swiglu: intermediate size %d", f);
  hipLaunchKernelGGL(lt_swiglu_lora_fwd_kernel, dim3((n + LT_ROWS - 1) / LT_ROWS), dim3(256), 0, st, gu, h, n, f, t, ldt, tcol,
                     W, r, s);
  LR_CHECK_LAUNCH("lt_swiglu_lora_fwd_kernel");
  return LR_OK;
}
// in place: (gate, up) -> (d gate, d up) given d h
__global__ __launch_bounds__(256) void lt_swiglu_bwd_kernel(u16* gu, const u16* dh, size_t total8, int f) {
  const int per_row = f >> 3;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += (size_t)gridDim.x * 256) {
    const size_t row = i / per_row;
    const int c = (int)(i % per_row) * 8;
    u16* p = gu + row * 2 * f + (c >> 4) * 32 + (c & 15);
    const u16x8 gv = *reinterpret_cast<const u16x8*>(p), uv = *reinterpret_cast<const u16x8*>(p + 16);
    const u16x8 dv = *reinterpret_cast<const u16x8*>(dh + row * f + c);
    u16x8 og, ou;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float g = bf2f(gv[e]), u = bf2f(uv[e]), dy = bf2f(dv[e]);
      const float sg = 1.0f / (1.0f + __expf(-g));
      og[e] = f2bf(dy * u * (sg * (1.0f + g * (1.0f - sg))));
      ou[e] = f2bf(dy * (g * sg));
    }
    *reinterpret_cast<u16x8*>(p) = og;
    *reinterpret_cast<u16x8*>(p + 16) = ou;
  }
}
int lr_launch_swiglu_fwd(const u16* gu, u16* h, int n, int f, hipStream_t st) {
  if (n < 1) return LR_OK;
  if (f % 16 != 0) LR_FAIL(LR_EUNSUPPORTED, "swiglu: intermediate size %d", f);
  const size_t total = (size_t)n * f / 8;
  hipLaunchKernelGGL(lt_swiglu_fwd_kernel, dim3((unsigned)min((size_t)16384, (total + 255) / 256)), dim3(256), 0, st, gu,
                     h, total, f);
  LR_CHECK_LAUNCH("lt_swiglu_fwd_kernel");
  return LR_OK;
}
int lr_launch_swiglu_bwd(u16* gu, const u16* dh, int n, int f, hipStream_t st) {
  if (n < 1) return LR_OK;
  if (f % 16 != 0) LR_FAIL(LR_EUNSUPPORTED, "swiglu: intermediate size %d", f);
  const size_t total = (size_t)n * f / 8;
  hipLaunchKernelGGL(lt_swiglu_bwd_kernel, dim3((unsigned)min((size_t)16384, (total + 255) / 256)), dim3(256), 0, st, gu,
                     dh, total, f);
  LR_CHECK_LAUNCH("lt_swiglu_bwd_kernel");
  return LR_OK;
}

// =============================================================================================
// RMSNorm backward (+ residual gradient, + the LoRA path's contribution to d xn)
// =============================================================================================
// y = w * x * rstd. With g = w .* dy:  dx = rstd * g - x * rstd^3 * mean(x .* g).
// out[out_row] = (res ? res[row] : 0) + dx.   dy may get the LoRA term first:
//   dy[c] += keep(row, c) * drop_scale * sum_j dt[row][j] * a_cat[j][c]     (j over both projections)
// A workgroup sweeps ROWS rows; a thread owns 8 consecutive columns (16-byte accesses) of up to LT_NORM_CHUNKS chunks
// of every row, kept in registers between the statistics pass and the output pass. With the LoRA term ROWS = 4
// (hidden <= 4096), so the 2r rows of A_cat a chunk needs come from L2 once per four activation rows.
#define LT_NORM_CHUNKS 4  // hidden <= 256 * 8 * 4 = 8192
template <int ROWS, int CHUNKS, bool LORA>
__global__ __launch_bounds__(256) void lt_rmsnorm_bwd_kernel(const u16* dy, const u16* x, const u16* w, const u16* res,
                                                             u16* out, int n, int d, float eps, const int32_t* out_rows,
                                                             const u16* dt, const u16* a_cat, int r,
                                                             uint32_t drop_stream, uint32_t drop_thresh,
                                                             float drop_scale, int ldt) {
  __shared__ float sh[4][2 * ROWS];
  __shared__ float ts[ROWS][2 * LT_RP];
  const int row0 = blockIdx.x * ROWS;
  const int nrows = min(ROWS, n - row0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (LORA) {
    if (threadIdx.x < ROWS * 2 * LT_RP) {
      const int rr = threadIdx.x / (2 * LT_RP), j = threadIdx.x % (2 * LT_RP);
      ts[rr][j] = rr < nrows ? bf2f(dt[(size_t)(row0 + rr) * ldt + j]) : 0.f;
    }
    __syncthreads();
  }
  u16x8 xv[ROWS][CHUNKS];
  float gv[ROWS][CHUNKS][8];
  float ss[ROWS], dot[ROWS];
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) ss[rr] = dot[rr] = 0.f;
#pragma unroll
  for (int ch = 0; ch < CHUNKS; ++ch) {
    const int c = (threadIdx.x + ch * 256) * 8;
    if (c >= d) continue;
    const u16x8 wv = *reinterpret_cast<const u16x8*>(w + c);
    float g[ROWS][8];
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
      const size_t at = (size_t)(row0 + min(rr, nrows - 1)) * d + c;
      xv[rr][ch] = *reinterpret_cast<const u16x8*>(x + at);
      const u16x8 dv = *reinterpret_cast<const u16x8*>(dy + at);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[rr][e] = bf2f(dv[e]);
    }
    if (LORA) {
      float l[ROWS][8];
#pragma unroll
      for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
        for (int e = 0; e < 8; ++e) l[rr][e] = 0.f;
      for (int j = 0; j < r; ++j) {
        const u16x8 a0 = *reinterpret_cast<const u16x8*>(a_cat + (size_t)j * d + c);
        const u16x8 a1 = *reinterpret_cast<const u16x8*>(a_cat + (size_t)(LT_RP + j) * d + c);
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
          const float t0 = ts[rr][j], t1 = ts[rr][LT_RP + j];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            l[rr][e] = __builtin_fmaf(t1, bf2f(a1[e]), __builtin_fmaf(t0, bf2f(a0[e]), l[rr][e]));
        }
      }
#pragma unroll
      for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (!drop_thresh || lt_keep(drop_stream, row0 + min(rr, nrows - 1), c + e, drop_thresh))
            g[rr][e] = bf2f(f2bf(g[rr][e] + bf2f(f2bf(l[rr][e] * drop_scale))));
    }
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xe = bf2f(xv[rr][ch][e]);
        gv[rr][ch][e] = g[rr][e] * bf2f(wv[e]);
        ss[rr] += xe * xe;
        dot[rr] += xe * gv[rr][ch][e];
      }
  }
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
#pragma unroll
    for (int s_ = 32; s_ >= 1; s_ >>= 1) {
      ss[rr] += __shfl_xor(ss[rr], s_, 64);
      dot[rr] += __shfl_xor(dot[rr], s_, 64);
    }
    if (lane == 0) {
      sh[wave][2 * rr] = ss[rr];
      sh[wave][2 * rr + 1] = dot[rr];
    }
  }
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    if (rr >= nrows) continue;
    const float s2 = sh[0][2 * rr] + sh[1][2 * rr] + sh[2][2 * rr] + sh[3][2 * rr];
    const float dt_ = sh[0][2 * rr + 1] + sh[1][2 * rr + 1] + sh[2][2 * rr + 1] + sh[3][2 * rr + 1];
    const float rstd = 1.0f / sqrtf(s2 / (float)d + eps);
    const float coef = dt_ / (float)d * rstd * rstd * rstd;
    const int orow = out_rows ? out_rows[row0 + rr] : row0 + rr;
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
      const int c = (threadIdx.x + ch * 256) * 8;
      if (c >= d) continue;
      u16x8 rv;
      if (res) rv = *reinterpret_cast<const u16x8*>(res + (size_t)(row0 + rr) * d + c);
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = rstd * gv[rr][ch][e] - bf2f(xv[rr][ch][e]) * coef;
        if (res) v = bf2f(f2bf(v)) + bf2f(rv[e]);
        o[e] = f2bf(v);
      }
      *reinterpret_cast<u16x8*>(out + (size_t)orow * d + c) = o;
    }
  }
}
int lr_launch_rmsnorm_bwd(const u16* dy, const u16* x, const u16* w, const u16* res, u16* out, int rows, int d, float eps,
                          const int32_t* out_rows, const u16* dt, const u16* a_cat, int r, uint32_t drop_stream,
                          float drop_p, hipStream_t st, int ldt) {
  if (rows < 1) return LR_OK;
  if (d % 8 != 0 || d > 256 * 8 * LT_NORM_CHUNKS)
    LR_FAIL(LR_EUNSUPPORTED, "rmsnorm backward: hidden_size %d (multiple of 8, <= %d)", d, 256 * 8 * LT_NORM_CHUNKS);
  const uint32_t th = lt_drop_thresh(drop_p);
  const float ds = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
#define LT_NORM_LAUNCH(ROWS, CH, LORA)                                                                              \
  hipLaunchKernelGGL((lt_rmsnorm_bwd_kernel<ROWS, CH, LORA>), dim3((rows + ROWS - 1) / ROWS), dim3(256), 0, st, dy, x, w, \
                     res, out, rows, d, eps, out_rows, dt, a_cat, r, drop_stream, th, ds, ldt)
  const int chunks = (d + 2047) / 2048;
  if (dt) {
    if (chunks <= 1) LT_NORM_LAUNCH(4, 1, true);
    else if (chunks == 2) LT_NORM_LAUNCH(4, 2, true);
    else LT_NORM_LAUNCH(2, 4, true);
  } else {
    if (chunks <= 1) LT_NORM_LAUNCH(1, 1, false);
    else if (chunks == 2) LT_NORM_LAUNCH(1, 2, false);
    else LT_NORM_LAUNCH(1, 4, false);
  }
#undef LT_NORM_LAUNCH
  LR_CHECK_LAUNCH("lt_rmsnorm_bwd_kernel");
  return LR_OK;
}

// =============================================================================================
// loss head: softmax cross-entropy over bf16 logit rows, rewritten in place into d logits
// =============================================================================================
// model/llm.py:113-126: logits = lm_head(h).float(); CrossEntropyLoss() = mean over the labelled tokens.
// scal[0] += sum of -log p(target); d logits = (softmax - onehot) * gscale, gscale = grad_scale / n_labelled.
// DET (deterministic mode): scal is a buffer of 2 + m floats and row i's loss is STORED to scal[2 + i] (0 for a row without a
// token id) for lt_finish_loss_det_kernel to sum in a fixed order. scal[1] counts in both modes: adding 1.0f is exact in any order.
template <bool DET>
__global__ __launch_bounds__(256) void lt_ce_kernel(u16* logits, int V, const int32_t* targets, float gscale,
                                                    float* scal) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  u16* x = logits + (size_t)row * V;
  const int tgt = targets[row];
  if (tgt < 0 || tgt >= V) {  // not a token id: no loss, no gradient, counted
    for (int j = threadIdx.x; j < V; j += 256) x[j] = 0;
    if (threadIdx.x == 0) {
      atomicAdd(scal + 1, 1.0f);
      if (DET) scal[2 + row] = 0.f;
    }
    return;
  }
  float mx = -__builtin_inff();
  for (int j = threadIdx.x; j < V; j += 256) mx = fmaxf(mx, bf2f(x[j]));
  mx = lt_block_max(mx, sh);
  float se = 0.f;
  for (int j = threadIdx.x; j < V; j += 256) se += __expf(bf2f(x[j]) - mx);
  se = lt_block_sum(se, sh);
  const float picked = bf2f(x[tgt]);
  __syncthreads();
  const float inv = 1.0f / se;
  for (int j = threadIdx.x; j < V; j += 256) {
    const float p = __expf(bf2f(x[j]) - mx) * inv;
    x[j] = f2bf((p - (j == tgt ? 1.0f : 0.0f)) * gscale);
  }
  if (threadIdx.x == 0) {
    if (DET) scal[2 + row] = logf(se) + mx - picked;
    else atomicAdd(scal, logf(se) + mx - picked);
  }
}
int lr_launch_ce_bf16(u16* logits, int m, int V, const int32_t* targets, float gscale, float* scal, hipStream_t st,
                      bool deterministic) {
  if (m < 1) return LR_OK;
  if (deterministic) hipLaunchKernelGGL(lt_ce_kernel<true>, dim3(m), dim3(256), 0, st, logits, V, targets, gscale, scal);
  else hipLaunchKernelGGL(lt_ce_kernel<false>, dim3(m), dim3(256), 0, st, logits, V, targets, gscale, scal);
  LR_CHECK_LAUNCH("lt_ce_kernel");
  return LR_OK;
}

// out[0] = loss sum / m (mean over the labelled tokens), out[1] = m, out[2] = targets outside the vocabulary
__global__ void lt_finish_loss_kernel(const float* scal, int m, float* out) {
  out[0] = m > 0 ? scal[0] / (float)m : 0.f;
  out[1] = (float)m;
  out[2] = scal[1];
}
// One workgroup's sum of g[0 .. n) (or of their squares) in an order fixed by n alone: thread t adds elements t, t + 256, ... in
// ascending order, the 64 lanes of a wave and then the 4 waves combine in lt_block_sum's fixed tree. Every thread gets the sum.
template <bool SQUARE>
__device__ __forceinline__ float lt_ordered_sum(const float* g, size_t n, float* sh) {
  float s = 0.f;
  for (size_t i = threadIdx.x; i < n; i += 256) s += SQUARE ? g[i] * g[i] : g[i];
  return lt_block_sum(s, sh);
}
// deterministic mode: the same three outputs from lt_ce_kernel<true>'s per-row losses (scal[2 + i]), summed in row order
__global__ __launch_bounds__(256) void lt_finish_loss_det_kernel(const float* scal, int m, float* out) {
  __shared__ float sh[4];
  const float sum = lt_ordered_sum<false>(scal + 2, (size_t)m, sh);
  if (threadIdx.x != 0) return;
  out[0] = m > 0 ? sum / (float)m : 0.f;
  out[1] = (float)m;
  out[2] = scal[1];
}
int lr_launch_finish_loss(const float* scal, int m, float* out, hipStream_t st, bool deterministic) {
  if (deterministic) hipLaunchKernelGGL(lt_finish_loss_det_kernel, dim3(1), dim3(256), 0, st, scal, m, out);
  else hipLaunchKernelGGL(lt_finish_loss_kernel, dim3(1), dim3(1), 0, st, scal, m, out);
  LR_CHECK_LAUNCH("lt_finish_loss_kernel");
  return LR_OK;
}

// D[row][h] = sum_d dO[row][h][d] * O[row][h][d]   (softmax backward's row term)
__global__ __launch_bounds__(256) void lt_rowdot_kernel(const u16* o, const u16* d_o, int n_items /* n*nh */, int hd,
                                                        float* out) {
  // 16 lanes x 8 elements cover up to 128 dims per step: 4 (token, head) items per wave
  const int lane = threadIdx.x & 63, sub = lane >> 4, l16 = lane & 15;
  const int item = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + sub;
  float s = 0.f;
  if (item < n_items)
    for (int c = l16 * 8; c < hd; c += 128) {
      const u16x8 a = *reinterpret_cast<const u16x8*>(o + (size_t)item * hd + c);
      const u16x8 b = *reinterpret_cast<const u16x8*>(d_o + (size_t)item * hd + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = __builtin_fmaf(bf2f(a[e]), bf2f(b[e]), s);
    }
#pragma unroll
  for (int sft = 8; sft >= 1; sft >>= 1) s += __shfl_xor(s, sft, 64);
  if (l16 == 0 && item < n_items) out[item] = s;
}
int lr_launch_rowdot(const u16* o, const u16* d_o, int n, int nh, int hd, float* out, hipStream_t st) {
  if (n < 1) return LR_OK;
  if (hd % 8 != 0) LR_FAIL(LR_EUNSUPPORTED, "rowdot: head_dim %d", hd);
  hipLaunchKernelGGL(lt_rowdot_kernel, dim3((n * nh + 15) / 16), dim3(256), 0, st, o, d_o, n * nh, hd, out);
  LR_CHECK_LAUNCH("lt_rowdot_kernel");
  return LR_OK;
}

// =============================================================================================
// clipping + AdamW over the flat fp32 LoRA buffer (torch.optim.AdamW arithmetic, HF Trainer defaults)
// =============================================================================================
__global__ __launch_bounds__(256) void lt_sumsq_kernel(const float* g, size_t n, float* out) {
  __shared__ float sh[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += g[i] * g[i];
  s = lt_block_sum(s, sh);
  if (threadIdx.x == 0) atomicAdd(out, s);
}
// Deterministic mode's squared gradient norm: lr_llama_lora_apply has no workspace and the handle's scratch no room for
// per-workgroup partials, so ONE workgroup of 1024 threads sums the whole buffer. Thread t takes the 16-byte groups t, t + 1024,
// ... in ascending order into four running sums (one per float of the group), adds them 0..3, the tail n % 4 goes to thread 0;
// lanes, then waves, combine in a fixed tree. 20 M gradients (Llama-2-7b, all seven modules, r = 8) are 80 MB through one CU.
__global__ __launch_bounds__(1024) void lt_sumsq_det_kernel(const float* g, size_t n, float* out) {
  __shared__ float sh[16];
  floatx4 s4 = floatx4{0.f, 0.f, 0.f, 0.f};
  const size_t n4 = n >> 2;
#pragma unroll 4
  for (size_t i = threadIdx.x; i < n4; i += 1024) {
    const floatx4 v = *reinterpret_cast<const floatx4*>(g + 4 * i);
    s4 += v * v;
  }
  float s = ((s4[0] + s4[1]) + s4[2]) + s4[3];
  if (threadIdx.x == 0)
    for (size_t i = n4 << 2; i < n; ++i) s += g[i] * g[i];
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) s += __shfl_xor(s, sft, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = sh[0];
    for (int w = 1; w < 16; ++w) t += sh[w];
    out[0] = t;
  }
}
// hyper[0] lr, hyper[1] max_grad_norm (<= 0: no clipping); ctr[0] = optimizer steps taken so far
__global__ __launch_bounds__(256) void lt_adamw_kernel(float* p, float* g, float* m, float* v, size_t n,
                                                       const float* sumsq, const float* hyper, const int* ctr,
                                                       float beta1, float beta2, float eps, float wd, float* out_norm) {
  const float norm = sqrtf(sumsq[0]);
  const float lr = hyper[0], limit = hyper[1];
  const float coef = limit > 0.f ? fminf(1.0f, limit / (norm + 1e-6f)) : 1.0f;  // torch clip_grad_norm_
  const int step = ctr[0] + 1;
  const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float gi = g[i] * coef;
    float pi = p[i] * (1.0f - lr * wd);
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    pi -= (lr / bc1) * mi / (sqrtf(vi) / sqrtf(bc2) + eps);
    p[i] = pi;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && out_norm) out_norm[0] = norm;
}
__global__ void lt_set_hyper_kernel(float* hyper, float lr, float limit, float* sumsq) {
  hyper[0] = lr;
  hyper[1] = limit;
  sumsq[0] = 0.f;
}
__global__ void lt_bump_kernel(int* ctr) { ctr[0] += 1; }
int lr_launch_lora_adamw(float* p, float* g, float* m, float* v, size_t n, float* scratch /*[4]*/, int* ctr, float lr,
                         float max_grad_norm, float beta1, float beta2, float eps, float wd, float* out_norm,
                         hipStream_t st, bool deterministic) {
  float* sumsq = scratch;
  float* hyper = scratch + 1;
  hipLaunchKernelGGL(lt_set_hyper_kernel, dim3(1), dim3(1), 0, st, hyper, lr, max_grad_norm, sumsq);
  const unsigned blocks = (unsigned)min((size_t)1024, (n + 255) / 256);
  if (deterministic) {
    if (((uintptr_t)g & 15) != 0) LR_FAIL(LR_EUNSUPPORTED, "deterministic gradient norm: the buffer must be 16-byte aligned");
    hipLaunchKernelGGL(lt_sumsq_det_kernel, dim3(1), dim3(1024), 0, st, g, n, sumsq);
  } else {
    hipLaunchKernelGGL(lt_sumsq_kernel, dim3(blocks), dim3(256), 0, st, g, n, sumsq);
  }
  hipLaunchKernelGGL(lt_adamw_kernel, dim3(blocks), dim3(256), 0, st, p, g, m, v, n, sumsq, hyper, ctr, beta1, beta2,
                     eps, wd, out_norm);
  hipLaunchKernelGGL(lt_bump_kernel, dim3(1), dim3(1), 0, st, ctr);
  LR_CHECK_LAUNCH("lt_adamw_kernel");
  return LR_OK;
}

uint32_t lr_lora_drop_stream(uint64_t seed, uint32_t pass, uint32_t layer) {
  uint64_t z = seed + 0x9e3779b97f4a7c15ull * ((uint64_t)pass * 131u + layer + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)(z ^ (z >> 31));
}
