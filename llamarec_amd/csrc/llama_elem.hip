// llama_elem.hip -- memory-bound pieces of the Llama prefill on gfx950: token-embedding gather,
// RMSNorm, the rotary cos/sin table, final norm + verbalizer GEMV. (RoPE itself and SwiGLU are
// fused into GEMM epilogues, llama_gemm.hip.)
//
// Replaces the ATen kernels reached from HF LlamaModel (transformers modeling_llama.py: RMSNorm
// with fp32 statistics, rotate_half RoPE, SiLU*mul) and, for the head, `lm_head` over ALL
// positions + `.float()` + `[:, -1]` (model/llm.py:113-114,131) followed by the verbalizer's
// column gather (trainer/verb.py:524-544): here only the LAST token of each prompt is normalised
// and only the C label-word rows of lm_head are multiplied.
//
// All activations are bf16 with fp32 arithmetic inside a kernel; 16-byte vector accesses.
#include "llama_kernels.h"
#include "lr_profile.h"

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float block_sum_256(float v, float* red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ---- packed-layout metadata ---------------------------------------------------------------------
// Without a shared prefix (P = 0) the internal rows are the caller's packed tokens: segment b = prompt b.
// With P > 0 (every prompt starts with the same P tokens, run once): S = B + 1 segments,
//   segment 0      rows [0, P)                                     = the prefix, taken from prompt 0
//   segment b + 1  rows [P + cu[b] - b P, P + cu[b+1] - (b+1) P)   = prompt b's tokens at positions P..T_b-1
// tok_pos = position inside the prompt (rotary embedding), tok_src = index into the caller's packed ids,
// last_rows[b] = internal row of prompt b's last token, seg_start[0..S] = segment starts.
// ids / prefix_bad (shared prefix only): the caller PROMISES that every prompt starts with prompt 0's first P tokens; the
// promise is checked here -- a prompt whose first P ids differ sets *prefix_bad, and head_kernel then writes NaN scores
// for the whole call (prefix rows, K and V come from prompt 0: a stale prefix_len would otherwise score prompts 1..B-1
// silently wrong).
__global__ void token_meta_kernel(const int32_t* cu, int B, int P, int32_t* seg_start, int32_t* tok_pos,
                                  int32_t* tok_src, int32_t* last_rows, int32_t* last_pos, const int32_t* ids,
                                  int32_t* prefix_bad) {
  const int seg = blockIdx.x;
  int start, len, pos0, src0;
  if (P > 0 && seg == 0) {
    start = 0, len = P, pos0 = 0, src0 = cu[0];
  } else {
    const int b = P > 0 ? seg - 1 : seg;
    const int s = cu[b], e = cu[b + 1];
    if (P > 0 && b > 0 && ids && prefix_bad) {
      const int s0 = cu[0];
      bool bad = false;
      for (int i = threadIdx.x; i < P; i += blockDim.x) bad |= ids[s + i] != ids[s0 + i];
      if (bad) atomicOr(prefix_bad, 1);
    }
    start = P > 0 ? P + s - b * P : s;
    len = e - s - P;
    pos0 = P;
    src0 = s + P;
    if (threadIdx.x == 0) {
      if (last_rows) last_rows[b] = start + len - 1;
      if (last_pos) last_pos[b] = pos0 + len - 1;   // position of the prompt's last token (rotary embedding of its query)
      if (seg_start && seg == (int)gridDim.x - 1) seg_start[seg + 1] = start + len;
    }
  }
  if (threadIdx.x == 0 && seg_start) seg_start[seg] = start;
  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    tok_pos[start + i] = pos0 + i;
    if (tok_src) tok_src[start + i] = src0 + i;
  }
}

// ---- embedding gather ------------------------------------------------------------------------
// SCALE (Gemma): every value bf16(e * scale), the scale already a bf16 value
template <bool SCALE>
__global__ __launch_bounds__(256) void embed_kernel(const int32_t* ids, const int32_t* tok_src, const u16* table,
                                                    int vocab, int d, u16* out, float scale) {
  const int tok = blockIdx.x;
  int id = ids[tok_src ? tok_src[tok] : tok];
  if (id < 0 || id >= vocab) id = 0;
  const u16x8* src = reinterpret_cast<const u16x8*>(table + (size_t)id * d);
  u16x8* dst = reinterpret_cast<u16x8*>(out + (size_t)tok * d);
  for (int i = threadIdx.x; i < d / 8; i += 256) {
    if (SCALE) {
      const u16x8 e = src[i];
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(e[j]) * scale);
      dst[i] = o;
    } else {
      dst[i] = src[i];
    }
  }
}

// ---- RMSNorm: out = bf16( w * bf16( x * rsqrt(mean(x^2) + eps) ) ) --------------------------
// One workgroup per row. Rows of up to 8192 features stay in registers between the square sum and the scaling (each
// thread keeps its <= 4 pieces of 8, and requests the matching weights with them): the kernel is a chain of memory
// latencies per row, not bandwidth, and re-reading the row after the reduction added one more link. Same arithmetic,
// same order, as the two-pass form that longer rows still take. NS = norm style (rms_apply: 0 Llama, 1 Gemma).
#define RMS_KEEP 4
template <int NS>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const u16* x, const u16* w, u16* out, int d,
                                                      float eps, const int32_t* row_map) {
  __shared__ float red[4];
  const int row = row_map ? row_map[blockIdx.x] : blockIdx.x;
  const u16x8* xr = reinterpret_cast<const u16x8*>(x + (size_t)row * d);
  const u16x8* wr = reinterpret_cast<const u16x8*>(w);
  u16x8* orow = reinterpret_cast<u16x8*>(out + (size_t)blockIdx.x * d);
  const int nv = d / 8;
  const bool keep = nv <= 256 * RMS_KEEP;
  u16x8 vb[RMS_KEEP], wb[RMS_KEEP];
  float ss = 0.f;
  if (keep) {
#pragma unroll
    for (int k = 0; k < RMS_KEEP; ++k) {
      const int i = threadIdx.x + 256 * k;
      if (i < nv) {
        vb[k] = xr[i];
        wb[k] = wr[i];
      }
    }
#pragma unroll
    for (int k = 0; k < RMS_KEEP; ++k) {
      if (threadIdx.x + 256 * k < nv) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = bf2f(vb[k][j]);
          ss = __builtin_fmaf(f, f, ss);
        }
      }
    }
  } else {
    for (int i = threadIdx.x; i < nv; i += 256) {
      u16x8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(v[j]);
        ss = __builtin_fmaf(f, f, ss);
      }
    }
  }
  ss = block_sum_256(ss, red);
  const float rstd = 1.0f / sqrtf(ss / (float)d + eps);
  if (keep) {
#pragma unroll
    for (int k = 0; k < RMS_KEEP; ++k) {
      const int i = threadIdx.x + 256 * k;
      if (i < nv) {
        u16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = rms_apply<NS>(wb[k][j], vb[k][j], rstd);
        orow[i] = o;
      }
    }
  } else {
    for (int i = threadIdx.x; i < nv; i += 256) {
      u16x8 v = xr[i], wv = wr[i], o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rms_apply<NS>(wv[j], v[j], rstd);
      orow[i] = o;
    }
  }
}

// ---- split-K reduce + residual add + the RMSNorm that follows, one pass per row --------------------------------------
// The latency mode's o_proj / down_proj leave S fp32 partial planes (llama_gemm.hip, variant 5); summing them, adding the
// residual and storing the new residual row is one launch, the RMSNorm of that row for the next projection another: two
// dependent ~5-9 us launches per product at B = 1. Here a workgroup owns a row: thread t takes the chunks t + 256 k of 8
// columns, exactly rmsnorm_kernel's assignment, so the square sum is formed from the same values in the same order and the
// two outputs (residual row C, normalised row `out`) carry the same bits as the two-launch form (planes summed in split
// order, then bf16(bf16(sum) + residual) as in the GEMM's residual epilogue).
template <int NS>
__global__ __launch_bounds__(256) void reduce_residual_rmsnorm_kernel(const float* __restrict__ part, int S, size_t plane,
                                                                      u16* C, const u16* R, int N, const u16* w, u16* out,
                                                                      float eps) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  const int nv = N / 8;
  u16x8 vb[RMS_KEEP], wb[RMS_KEEP];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < nv) {
      const size_t off = (size_t)row * N + (size_t)i * 8;
      floatx4 a = *reinterpret_cast<const floatx4*>(part + off), b = *reinterpret_cast<const floatx4*>(part + off + 4);
      for (int sp = 1; sp < S; ++sp) {
        a += *reinterpret_cast<const floatx4*>(part + sp * plane + off);
        b += *reinterpret_cast<const floatx4*>(part + sp * plane + off + 4);
      }
      const u16x8 r = *reinterpret_cast<const u16x8*>(R + off);
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = f2bf(bf2f(f2bf(a[j])) + bf2f(r[j]));
        o[4 + j] = f2bf(bf2f(f2bf(b[j])) + bf2f(r[4 + j]));
      }
      *reinterpret_cast<u16x8*>(C + off) = o;
      vb[k] = o;
      wb[k] = reinterpret_cast<const u16x8*>(w)[i];
    }
  }
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    if (threadIdx.x + 256 * k < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf2f(vb[k][j]);
        ss = __builtin_fmaf(f, f, ss);
      }
    }
  }
  ss = block_sum_256(ss, red);
  const float rstd = 1.0f / sqrtf(ss / (float)N + eps);
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < nv) {
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rms_apply<NS>(wb[k][j], vb[k][j], rstd);
      reinterpret_cast<u16x8*>(out + (size_t)row * N)[i] = o;
    }
  }
}
// false: the row is too long to keep in registers (the caller then runs the two launches)
bool lr_reduce_residual_rmsnorm_fits(int N) { return N % 8 == 0 && N / 8 <= 256 * RMS_KEEP; }
int lr_launch_reduce_residual_rmsnorm(const float* part, int S, u16* C, const u16* R, int M, int N, const u16* norm_w,
                                      u16* norm_out, float eps, hipStream_t st, int norm_style) {
  if (!lr_reduce_residual_rmsnorm_fits(N)) LR_FAIL(LR_EUNSUPPORTED, "fused reduce + RMSNorm: %d columns", N);
  if (norm_style == 1)
    hipLaunchKernelGGL(reduce_residual_rmsnorm_kernel<1>, dim3(M), dim3(256), 0, st, part, S, (size_t)M * N, C, R, N, norm_w,
                       norm_out, eps);
  else
    hipLaunchKernelGGL(reduce_residual_rmsnorm_kernel<0>, dim3(M), dim3(256), 0, st, part, S, (size_t)M * N, C, R, N, norm_w,
                       norm_out, eps);
  LR_CHECK_LAUNCH("reduce_residual_rmsnorm_kernel");
  return LR_OK;
}

// ---- RMSNorm statistic only (the normalisation itself is folded into the next GEMM, llama_gemm.hip RopeArgs) ------
// one wave per row: 16-byte loads, fp32 square-sum in a fixed order (lane-strided, then the 6-step butterfly), so a
// row's rstd never depends on what else is in the batch
__global__ __launch_bounds__(256) void rms_rstd_kernel(const u16* x, float* rstd, int rows, int d, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const u16x8* xr = reinterpret_cast<const u16x8*>(x + (size_t)row * d);
  float ss = 0.f;
  for (int i = lane; i < d / 8; i += 64) {
    const u16x8 v = xr[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = bf2f(v[j]);
      ss = __builtin_fmaf(f, f, ss);
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) ss += __shfl_xor(ss, s, 64);
  if (lane == 0) rstd[row] = 1.0f / sqrtf(ss / (float)d + eps);
}

__global__ __launch_bounds__(256) void fold_norm_kernel(const u16* w, const u16* nw, u16* out, size_t n_vec, int cols_vec) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_vec) return;
  const u16x8 a = reinterpret_cast<const u16x8*>(w)[i];
  const u16x8 b = reinterpret_cast<const u16x8*>(nw)[i % cols_vec];
  u16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(a[j]) * bf2f(b[j]));
  reinterpret_cast<u16x8*>(out)[i] = o;
}

int lr_launch_rms_rstd(const u16* x, float* rstd, int rows, int d, float eps, hipStream_t st) {
  if (rows <= 0) return LR_OK;
  if (d % 8 != 0) LR_FAIL(LR_EINVAL, "rms_rstd: hidden size %d is not a multiple of 8", d);
  hipLaunchKernelGGL(rms_rstd_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, rstd, rows, d, eps);
  LR_CHECK_LAUNCH("rms_rstd_kernel");
  return LR_OK;
}

int lr_launch_fold_norm(const u16* w, const u16* norm_w, u16* out, size_t rows, int cols, hipStream_t st) {
  if (rows == 0) return LR_OK;
  if (cols % 8 != 0) LR_FAIL(LR_EINVAL, "fold_norm: %d columns are not a multiple of 8", cols);
  const size_t n_vec = rows * (size_t)(cols / 8);
  hipLaunchKernelGGL(fold_norm_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, st, w, norm_w, out, n_vec,
                     cols / 8);
  LR_CHECK_LAUNCH("fold_norm_kernel");
  return LR_OK;
}

// ---- RoPE table: cos/sin(pos * theta^(-2i/hd)) rounded to bf16 like HF's bf16 rotary ---------
// cs16 (optional): the same values packed as bf16 pairs, cos in the low half-word and sin in the high one -- lossless (the
// fp32 table holds bf16-representable values); the 256-tile GEMM's rotary epilogue stages these 4-byte entries through LDS.
__global__ void rope_table_kernel(float* cs /*[T][hd/2][2]*/, unsigned* cs16 /*[T][hd/2]*/, int T, int hd, float theta) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int half = hd / 2;
  if (i >= T * half) return;
  int pos = i / half, j = i % half;
  float inv = 1.0f / powf(theta, (float)(2 * j) / (float)hd);
  float ang = (float)pos * inv;
  const u16 c = f2bf(cosf(ang)), sn = f2bf(sinf(ang));
  cs[2 * i + 0] = bf2f(c);
  cs[2 * i + 1] = bf2f(sn);
  if (cs16) cs16[i] = (unsigned)c | ((unsigned)sn << 16);
}

// The llama3 rule (include/llamarec_mi355x.h, LrRopeScaling) on the same fp32 inverse frequency; a kernel of its own, so the
// plain table's code and bits stay what they are.
__global__ void rope_table_llama3_kernel(float* cs, unsigned* cs16, int T, int hd, float theta, float factor, float low,
                                         float high, float orig) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int half = hd / 2;
  if (i >= T * half) return;
  int pos = i / half, j = i % half;
  float inv = 1.0f / powf(theta, (float)(2 * j) / (float)hd);
  const float wavelen = 6.283185307179586f / inv;
  if (wavelen > orig / low) {
    inv = inv / factor;
  } else if (!(wavelen < orig / high)) {
    const float s = (orig / wavelen - low) / (high - low);
    inv = (1.0f - s) * inv / factor + s * inv;
  }
  float ang = (float)pos * inv;
  const u16 c = f2bf(cosf(ang)), sn = f2bf(sinf(ang));
  cs[2 * i + 0] = bf2f(c);
  cs[2 * i + 1] = bf2f(sn);
  if (cs16) cs16[i] = (unsigned)c | ((unsigned)sn << 16);
}

// Linear scaling (LrRopeScaling kind 2; Gemma-3's global layers): every inverse frequency divided by factor, in fp32 like HF's
// inv_freq / factor. A kernel of its own for the same reason.
__global__ void rope_table_linear_kernel(float* cs, unsigned* cs16, int T, int hd, float theta, float factor) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int half = hd / 2;
  if (i >= T * half) return;
  int pos = i / half, j = i % half;
  float inv = 1.0f / powf(theta, (float)(2 * j) / (float)hd);
  inv = inv / factor;
  float ang = (float)pos * inv;
  const u16 c = f2bf(cosf(ang)), sn = f2bf(sinf(ang));
  cs[2 * i + 0] = bf2f(c);
  cs[2 * i + 1] = bf2f(sn);
  if (cs16) cs16[i] = (unsigned)c | ((unsigned)sn << 16);
}

// ---- final RMSNorm on each prompt's last token + dot with selected lm_head rows -------------
// grid (B, ceil(C/32)); out[b][c] = float(bf16(sum_k xn[k] * W[row_c][k])), row_c = ids ? ids[c] : c
// CAP (Gemma-2's final_logit_softcapping): HF runs logits / cap, tanh, * cap on the bf16 logits and then .float(), so each of
// the three steps rounds to bf16: out = bf16(bf16(tanh(bf16(bf16(acc) / cap))) * cap). Without CAP `cap` is not read, and the
// instructions of <0, false> and <1, false> are those of the kernel before it had the parameter ("What the
// existing code objects became").
template <int NS, bool CAP>
__global__ __launch_bounds__(256) void head_kernel(const u16* x, const int32_t* rows, const u16* norm_w,
                                                   const u16* lm_head, const int32_t* class_ids, int C,
                                                   int d, float eps, float* out, int vocab, const int32_t* poison, float cap) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  u16* xn = reinterpret_cast<u16*>(smem_raw);  // [d]
  __shared__ float red[4];
  const int b = blockIdx.x;
  if (poison && *poison) {  // the call's shared-prefix promise was broken (token_meta_kernel): no score is trustworthy
    for (int cc = threadIdx.x; cc < 32; cc += 256) {
      const int c = blockIdx.y * 32 + cc;
      if (c < C) out[(size_t)b * C + c] = __builtin_nanf("");
    }
    return;
  }
  const int row = rows ? rows[b] : b;  // rows == nullptr: x is already compact, one row per prompt
  const u16* xr = x + (size_t)row * d;
  float ss = 0.f;
  for (int i = threadIdx.x; i < d; i += 256) {
    float f = bf2f(xr[i]);
    ss = __builtin_fmaf(f, f, ss);
  }
  ss = block_sum_256(ss, red);
  const float rstd = 1.0f / sqrtf(ss / (float)d + eps);
  for (int i = threadIdx.x; i < d; i += 256)
    xn[i] = rms_apply<NS>(norm_w[i], xr[i], rstd);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int cc = wave; cc < 32; cc += 4) {
    int c = blockIdx.y * 32 + cc;
    if (c >= C) break;
    int r = class_ids ? class_ids[c] : c;
    if (r < 0 || r >= vocab) {  // a label word outside the vocabulary: NaN score instead of a wild read
      if (lane == 0) out[(size_t)b * C + c] = __builtin_nanf("");
      continue;
    }
    const u16* wr = lm_head + (size_t)r * d;
    float acc = 0.f;
    for (int k = lane * 8; k < d; k += 512) {
      u16x8 wv = *reinterpret_cast<const u16x8*>(wr + k);
      u16x8 xv = *reinterpret_cast<const u16x8*>(xn + k);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_fmaf(bf2f(wv[j]), bf2f(xv[j]), acc);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if constexpr (CAP) {
      if (lane == 0) out[(size_t)b * C + c] = bf2f(f2bf(bf2f(f2bf(tanhf(bf2f(f2bf(bf2f(f2bf(acc)) / cap))))) * cap));
    } else {
      if (lane == 0) out[(size_t)b * C + c] = bf2f(f2bf(acc));
    }
  }
}

// ---- gather rows: out[i][:] = x[rows[i]][:] ----------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const u16* x, const int32_t* rows, int d, u16* out) {
  const u16x8* src = reinterpret_cast<const u16x8*>(x + (size_t)rows[blockIdx.x] * d);
  u16x8* dst = reinterpret_cast<u16x8*>(out + (size_t)blockIdx.x * d);
  for (int i = threadIdx.x; i < d / 8; i += 256) dst[i] = src[i];
}

int lr_launch_gather_rows(const u16* x, const int32_t* rows, int n_rows, int d, u16* out, hipStream_t st) {
  if (n_rows <= 0) return LR_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(n_rows), dim3(256), 0, st, x, rows, d, out);
  LR_CHECK_LAUNCH("gather_rows_kernel");
  return LR_OK;
}

// ---------------------------------------------------------------------------------------------
int lr_launch_token_meta(const int32_t* cu, int B, int prefix_len, int32_t* seg_start, int32_t* tok_pos,
                         int32_t* tok_src, int32_t* last_rows, hipStream_t st, int32_t* last_pos, const int32_t* ids,
                         int32_t* prefix_bad) {
  const int S = prefix_len > 0 ? B + 1 : B;
  if (prefix_bad) LR_CHECK_HIP(hipMemsetAsync(prefix_bad, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(token_meta_kernel, dim3(S), dim3(256), 0, st, cu, B, prefix_len, seg_start, tok_pos, tok_src,
                     last_rows, last_pos, ids, prefix_bad);
  LR_CHECK_LAUNCH("token_meta_kernel");
  return LR_OK;
}

int lr_launch_embed(const int32_t* ids, const int32_t* tok_src, const u16* table, int vocab, int d, u16* out, int n,
                    hipStream_t st, float scale) {
  if (scale != 1.0f)
    hipLaunchKernelGGL(embed_kernel<true>, dim3(n), dim3(256), 0, st, ids, tok_src, table, vocab, d, out, scale);
  else
    hipLaunchKernelGGL(embed_kernel<false>, dim3(n), dim3(256), 0, st, ids, tok_src, table, vocab, d, out, scale);
  LR_CHECK_LAUNCH("embed_kernel");
  return LR_OK;
}

int lr_launch_rmsnorm(const u16* x, const u16* w, u16* out, int rows, int d, float eps,
                      const int32_t* row_map, hipStream_t st, int norm_style) {
  if (norm_style == 1)
    hipLaunchKernelGGL(rmsnorm_kernel<1>, dim3(rows), dim3(256), 0, st, x, w, out, d, eps, row_map);
  else
    hipLaunchKernelGGL(rmsnorm_kernel<0>, dim3(rows), dim3(256), 0, st, x, w, out, d, eps, row_map);
  LR_CHECK_LAUNCH("rmsnorm_kernel");
  return LR_OK;
}

int lr_check_rope_scaling(const LrRopeScaling* s, const char* who) {
  if (!s) return LR_OK;
  for (int i = 0; i < 3; ++i)
    if (s->reserved[i]) LR_FAIL(LR_EINVAL, "%s: rope scaling reserved word %d is not zero", who, i);
  if (s->kind == 0) return LR_OK;
  if (s->kind == 2) {   // linear: factor alone; the llama3 words it does not read must be zero (a llama3 block with the kind
                        // mistyped is refused, as every kind but 0 and 1 was before this one existed)
    if (!(s->factor > 0.f) || !(s->factor < __builtin_inff()) || s->low_freq_factor != 0.f || s->high_freq_factor != 0.f ||
        s->original_max_positions != 0)
      LR_FAIL(LR_EINVAL, "%s: linear rope scaling factor=%g (finite and > 0) low_freq_factor=%g high_freq_factor=%g "
              "original_max_positions=%d (must be zero: not read)", who, (double)s->factor, (double)s->low_freq_factor,
              (double)s->high_freq_factor, s->original_max_positions);
    return LR_OK;
  }
  if (s->kind != 1) LR_FAIL(LR_EINVAL, "%s: unknown rope scaling kind %d (0 none, 1 llama3, 2 linear)", who, s->kind);
  if (!(s->factor >= 1.0f) || !(s->low_freq_factor > 0.f) || !(s->low_freq_factor < s->high_freq_factor) ||
      !(s->high_freq_factor < __builtin_inff()) || !(s->factor < __builtin_inff()) || s->original_max_positions < 1)
    LR_FAIL(LR_EINVAL, "%s: llama3 rope scaling factor=%g low_freq_factor=%g high_freq_factor=%g original_max_positions=%d",
            who, (double)s->factor, (double)s->low_freq_factor, (double)s->high_freq_factor, s->original_max_positions);
  return LR_OK;
}

int lr_launch_rope_table(float* cs, int T, int hd, float theta, hipStream_t st, unsigned* cs16, const LrRopeScaling* scaling) {
  int n = T * (hd / 2);
  LR_RUN(lr_check_rope_scaling(scaling, "rope table"));
  if (scaling && scaling->kind == 1) {
    hipLaunchKernelGGL(rope_table_llama3_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cs, cs16, T, hd, theta,
                       scaling->factor, scaling->low_freq_factor, scaling->high_freq_factor,
                       (float)scaling->original_max_positions);
    LR_CHECK_LAUNCH("rope_table_llama3_kernel");
    return LR_OK;
  }
  if (scaling && scaling->kind == 2) {
    hipLaunchKernelGGL(rope_table_linear_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cs, cs16, T, hd, theta, scaling->factor);
    LR_CHECK_LAUNCH("rope_table_linear_kernel");
    return LR_OK;
  }
  hipLaunchKernelGGL(rope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cs, cs16, T, hd, theta);
  LR_CHECK_LAUNCH("rope_table_kernel");
  return LR_OK;
}

int lr_launch_head(const u16* x, const int32_t* rows, const u16* norm_w, const u16* lm_head,
                   const int32_t* class_ids, int B, int C, int d, float eps, float* out, int vocab,
                   hipStream_t st, const int32_t* poison, int norm_style, float final_softcap) {
  dim3 grid(B, (C + 31) / 32);
  if (final_softcap > 0.f) {
    if (norm_style != 1) LR_FAIL(LR_EUNSUPPORTED, "head: a final soft cap goes with the Gemma norm");
    hipLaunchKernelGGL((head_kernel<1, true>), grid, dim3(256), (size_t)d * sizeof(u16), st, x, rows, norm_w, lm_head,
                       class_ids, C, d, eps, out, vocab, poison, final_softcap);
  } else if (norm_style == 1)
    hipLaunchKernelGGL((head_kernel<1, false>), grid, dim3(256), (size_t)d * sizeof(u16), st, x, rows, norm_w, lm_head,
                       class_ids, C, d, eps, out, vocab, poison, 0.f);
  else
    hipLaunchKernelGGL((head_kernel<0, false>), grid, dim3(256), (size_t)d * sizeof(u16), st, x, rows, norm_w, lm_head,
                       class_ids, C, d, eps, out, vocab, poison, 0.f);
  LR_CHECK_LAUNCH("head_kernel");
  return LR_OK;
}

// ---- Gemma-2's sandwich norm: the output h of attention (of the MLP) is normalised BEFORE it joins the residual ----------
//   x'  = bf16( float(x) + float(bf16(h * rstd(h) * (1 + w_out))) )          written over x
//   xn  = bf16( x' * rstd(x') * (1 + w_next) )                               NEXT only: the norm in front of the next product
// One workgroup per row, rmsnorm_kernel's chunk assignment (thread t holds chunks t + 256 k of 8 columns in registers, so both
// square sums are formed from the same values in the same order as two rmsnorm_kernel<1> launches around an add would form
// them, and the bits are those), 16-byte loads and stores: three row reads (h, x, the weights come from cache) and one or two
// row writes. xn may alias h: a thread reads its chunks of h before it writes the same chunks of xn, and no other thread
// touches them. Rows longer than 256 * RMS_KEEP * 8 = 8192 columns are refused by the launcher.
template <bool NEXT>
__global__ __launch_bounds__(256) void residual_postnorm_kernel(u16* x, const u16* h, const u16* w_out, const u16* w_next,
                                                                u16* xn, int d, float eps) {
  __shared__ float red[4];
  const size_t row_off = (size_t)blockIdx.x * d;
  const int nv = d / 8;
  u16x8 hb[RMS_KEEP], xb[RMS_KEEP], wb[RMS_KEEP], nb[RMS_KEEP];
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < nv) {
      hb[k] = reinterpret_cast<const u16x8*>(h + row_off)[i];
      xb[k] = reinterpret_cast<const u16x8*>(x + row_off)[i];
      wb[k] = reinterpret_cast<const u16x8*>(w_out)[i];
      if (NEXT) nb[k] = reinterpret_cast<const u16x8*>(w_next)[i];
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    if (threadIdx.x + 256 * k < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf2f(hb[k][j]);
        ss = __builtin_fmaf(f, f, ss);
      }
    }
  }
  ss = block_sum_256(ss, red);
  const float rstd_h = 1.0f / sqrtf(ss / (float)d + eps);
  float ss2 = 0.f;
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf2f(f2bf(bf2f(xb[k][j]) + bf2f(rms_apply<1>(wb[k][j], hb[k][j], rstd_h))));
        xb[k][j] = f2bf(f);
        ss2 = __builtin_fmaf(f, f, ss2);
      }
      reinterpret_cast<u16x8*>(x + row_off)[i] = xb[k];
    }
  }
  if (!NEXT) return;
  ss2 = block_sum_256(ss2, red);
  const float rstd_x = 1.0f / sqrtf(ss2 / (float)d + eps);
#pragma unroll
  for (int k = 0; k < RMS_KEEP; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < nv) {
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rms_apply<1>(nb[k][j], xb[k][j], rstd_x);
      reinterpret_cast<u16x8*>(xn + row_off)[i] = o;
    }
  }
}

int lr_launch_residual_postnorm(u16* x, const u16* h, const u16* w_out, const u16* w_next, u16* xn, int rows, int d, float eps,
                                hipStream_t st) {
  if (rows <= 0) return LR_OK;
  if (d < 8 || d % 8 != 0 || d / 8 > 256 * RMS_KEEP)
    LR_FAIL(LR_EUNSUPPORTED, "residual + out-norm: %d columns (a multiple of 8, at most %d)", d, 256 * RMS_KEEP * 8);
  LrProfScope prof(LR_PROF_ELEMENTWISE, (w_next ? 5.0 : 3.0) * rows * d * 2, st);   // work = bytes the rows must move
  if (w_next)
    hipLaunchKernelGGL(residual_postnorm_kernel<true>, dim3(rows), dim3(256), 0, st, x, h, w_out, w_next, xn, d, eps);
  else
    hipLaunchKernelGGL(residual_postnorm_kernel<false>, dim3(rows), dim3(256), 0, st, x, h, w_out, w_next, xn, d, eps);
  LR_CHECK_LAUNCH("residual_postnorm_kernel");
  return LR_OK;
}

// ---- Qwen3: per-head RMSNorm of q and k + the rotary embedding, in place on a plain-stored QKV product --------------------
// buf [rows][ld] holds nq + nk heads of hd columns from column 0 on, in the packed pair-interleaved order LR_EPI_ROPE writes
// (the v columns behind them are neither read nor written). Per (row, head): rstd = 1 / sqrt(mean(x^2) + eps) in fp32 from
// the bf16 values the GEMM stored, y = rms_apply<0>(w, x, rstd) = bf16(w * bf16(x * rstd)) (HF's Qwen3RMSNorm), then the
// rotation of bf2f(y) with the rope epilogue's (cos, sin) pairs, operation order and single rounding. q_norm serves the first
// nq heads, k_norm the rest; both [hd], permuted like a head's rows of wq / wk.
// A thread owns 8 consecutive columns (one 16-byte access each way), a head is L = HD / 8 consecutive lanes: chunk ids run
// row-major over rows x (nq + nk) L chunks, every count a multiple of L and L a divisor of 64, so a head never straddles a
// wave and the square sum is an L-lane butterfly without LDS. Lanes past the end stay in the shuffles (their groups are whole).
// NS = the norm's rounding (rms_apply): 0 Qwen3's bf16(w * bf16(x * rstd)), 1 Gemma-3's bf16(x * rstd * (1 + w)) in fp32.
template <int HD, int NS = 0>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(u16* buf, size_t total, int per_row, int ld, int nq,
                                                           const u16* q_norm, const u16* k_norm, float eps,
                                                           const int32_t* tok_pos, const float* rope_cs) {
  constexpr int L = HD / 8;
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = id < total;
  const size_t row = live ? id / per_row : 0;
  const int chunk = live ? (int)(id % per_row) : 0;
  const int head = chunk / L, part = chunk % L;
  u16* p = buf + row * ld + (size_t)chunk * 8;
  u16x8 x = {0, 0, 0, 0, 0, 0, 0, 0}, w = x;
  if (live) {
    x = *reinterpret_cast<const u16x8*>(p);
    w = *reinterpret_cast<const u16x8*>((head < nq ? q_norm : k_norm) + part * 8);
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = bf2f(x[j]);
    ss = __builtin_fmaf(f, f, ss);
  }
#pragma unroll
  for (int s = L / 2; s >= 1; s >>= 1) ss += __shfl_xor(ss, s, 64);
  if (!live) return;
  const float rstd = 1.0f / sqrtf(ss / (float)HD + eps);
  const float* cs = rope_cs + ((size_t)tok_pos[row] * (HD / 2) + part * 4) * 2;
  const float4 c01 = *reinterpret_cast<const float4*>(cs), c23 = *reinterpret_cast<const float4*>(cs + 4);
  const float co[4] = {c01.x, c01.z, c23.x, c23.z}, si[4] = {c01.y, c01.w, c23.y, c23.w};
  u16x8 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a0 = bf2f(rms_apply<NS>(w[2 * q], x[2 * q], rstd)), a1 = bf2f(rms_apply<NS>(w[2 * q + 1], x[2 * q + 1], rstd));
    o[2 * q] = f2bf(a0 * co[q] - a1 * si[q]);
    o[2 * q + 1] = f2bf(a1 * co[q] + a0 * si[q]);
  }
  *reinterpret_cast<u16x8*>(p) = o;
}

// head_dim a power of two in [16, 256] (a head = 2 .. 32 lanes)
bool lr_qk_norm_head_dim_ok(int hd) { return hd >= 16 && hd <= 256 && (hd & (hd - 1)) == 0; }

int lr_launch_qk_norm_rope(u16* buf, int rows, int ld, int nq, int nk, int hd, const u16* q_norm, const u16* k_norm,
                           float eps, const int32_t* tok_pos, const float* rope_cs, hipStream_t st, int norm_style) {
  if (rows <= 0 || nq + nk == 0) return LR_OK;
  if (norm_style != 0 && norm_style != 1) LR_FAIL(LR_EINVAL, "q/k norm sweep: norm_style %d (0 Qwen3, 1 Gemma-3)", norm_style);
  if (!lr_qk_norm_head_dim_ok(hd)) LR_FAIL(LR_EUNSUPPORTED, "q/k norm sweep: head_dim %d (a power of two from 16 to 256)", hd);
  if (!buf || nq < 0 || nk < 0 || (nq > 0 && !q_norm) || (nk > 0 && !k_norm) || !tok_pos || !rope_cs || ld % 8 != 0 ||
      (long long)(nq + nk) * hd > ld || (reinterpret_cast<uintptr_t>(buf) & 15) ||
      ((reinterpret_cast<uintptr_t>(q_norm) | reinterpret_cast<uintptr_t>(k_norm)) & 15))
    LR_FAIL(LR_EINVAL, "q/k norm sweep: bad argument (nq %d, nk %d, head_dim %d, row stride %d; 16-byte aligned pointers)", nq,
            nk, hd, ld);
  const int per_row = (nq + nk) * (hd / 8);
  const size_t total = (size_t)rows * per_row;
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffu) LR_FAIL(LR_EUNSUPPORTED, "q/k norm sweep: %d rows exceed the grid limit", rows);
  LrProfScope prof(LR_PROF_ELEMENTWISE, 2.0 * total * 16, st);   // work = bytes moved: every chunk read and written once
#define LR_QKN_CASE(HD)                                                                                                   \
  case HD:                                                                                                                \
    if (norm_style == 1)                                                                                                  \
      hipLaunchKernelGGL((qk_norm_rope_kernel<HD, 1>), dim3((unsigned)blocks), dim3(256), 0, st, buf, total, per_row, ld, \
                         nq, q_norm, k_norm, eps, tok_pos, rope_cs);                                                      \
    else                                                                                                                  \
      hipLaunchKernelGGL((qk_norm_rope_kernel<HD, 0>), dim3((unsigned)blocks), dim3(256), 0, st, buf, total, per_row, ld, \
                         nq, q_norm, k_norm, eps, tok_pos, rope_cs);                                                      \
    break;
  switch (hd) {
    LR_QKN_CASE(16) LR_QKN_CASE(32) LR_QKN_CASE(64) LR_QKN_CASE(128) LR_QKN_CASE(256)
  }
#undef LR_QKN_CASE
  LR_CHECK_LAUNCH("qk_norm_rope_kernel");
  return LR_OK;
}
