// llama_attn_generic_body.h -- the one text of the scalar attention, one wave per (query row, head), any head_dim <= 256:
// attn_generic_row, inlined into attn_generic_kernel (llama_attn.hip: K / V rows of the packed qkv) and
// attn_cached_generic_kernel (llama_attn_cached.hip: rows of a user's cache slot). A kernel finds its (row, head) item, the
// row's position in its prompt and where the prompt's K / V rows are; the arithmetic of a row is here, so both run the same
// operations in the same order on the same keys.
#ifndef LLAMA_ATTN_GENERIC_BODY_H
#define LLAMA_ATTN_GENERIC_BODY_H

#include "llama_kernels.h"

// The query at position pos (qp: its head's hd dims) over keys 0 .. pos: the K / V row of position p (the KV head's dims) is
// kbase / vbase + p * stride. cap > 0: Gemma-2's soft cap. window = W > 0: the row sees keys pos - W < key <= pos, and the walk
// starts at its first visible key (every 64-key step then holds a visible key, as in the causal walk); 0: from key 0.
// op = the output row's head; lse_out (optional) = where the row's log-sum-exp of the scaled scores goes (training).
// Call with 256 threads, a row per wave.
__device__ __forceinline__ void attn_generic_row(const unsigned short* qp, const unsigned short* kbase,
                                                 const unsigned short* vbase, int stride, int pos, int hd, float scale, float cap,
                                                 int window, unsigned short* op, float* lse_out) {
  __shared__ float qs[4][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int d = lane; d < hd; d += 64) qs[wave][d] = bf2f(qp[d]);
  __builtin_amdgcn_wave_barrier();
  float m = -__builtin_inff(), l = 0.f;
  float o[4] = {0.f, 0.f, 0.f, 0.f};  // dims lane, lane+64, lane+128, lane+192
  const int key_lo = window > 0 ? max(0, pos - window + 1) : 0;
  for (int k0 = key_lo; k0 <= pos; k0 += 64) {
    const int key = k0 + lane;
    float s = -__builtin_inff();
    if (key <= pos) {
      const unsigned short* kp = kbase + (size_t)key * stride;
      float acc = 0.f;
      for (int d = 0; d < hd; ++d) acc = __builtin_fmaf(qs[wave][d], bf2f(kp[d]), acc);
      s = acc * scale;
      if (cap > 0.f) s = cap * tanhf(s / cap);   // fp32, before masking and the maximum
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
      const unsigned short* vp = vbase + (size_t)(k0 + j) * stride;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int d = lane + 64 * i;
        if (d < hd) o[i] = __builtin_fmaf(pj, bf2f(vp[d]), o[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int d = lane + 64 * i;
    if (d < hd) op[d] = f2bf(o[i] / l);
  }
  if (lse_out && lane == 0) *lse_out = m + logf(l);
}

#endif
