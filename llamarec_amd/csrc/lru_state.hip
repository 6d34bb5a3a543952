// lru_state.hip -- LRURec user states for gfx950: carry a user's recurrence state forward by the ids that arrived since the
// last call instead of re-encoding the whole history (include/llamarec_mi355x.h, "LRURec user states").
//
// The encoder (lru_encoder.hip) runs h_t = lambda * h_{t-1} + bu_t as a sequential scan per complex channel and every other
// operation per position, so (h_re, h_im) of every block after t tokens summarises the history. This kernel repeats the
// encoder's chains from a stored state and returns the encoder's -- and the oracle's -- bits for the concatenated history:
// bias first, k ascending lr_fma chains in the projections, butterfly LayerNorm sums over the 64 lanes of a wave, the
// `h = bu` branch at a history's first token.
//
// Design:
//  * rows of a tile are USERS, not positions: one 256-thread workgroup (4 wave64) serves 16 users, so 4 096 users are 256
//    workgroups, one per CU. A workgroup reads each weight element once per token step, coalesced from the L2-resident
//    image (256 KB per block), exactly the encoder's weight traffic per 16 rows.
//  * the hot case, one new id per user, has no scan: gather the state, project, write the state.
//  * Ln > 1 loops the token columns inside the kernel. A row takes part in a column when its id there is > 0; everything a
//    row computes in a column it does not take part in is discarded. A column no row of the workgroup takes part in costs
//    one barrier. The state lives in the table between columns (the thread that wrote an element is the one that reads it
//    again), so a long bootstrap is correct, not fast.
//  * the last block's out_proj / FFN tail runs once per call, on each row's last consumed token, as the encoder runs it
//    for its last tile only.
//  * a slot outside [0, num_slots) makes its row inert: nothing of the table is read or written for it.
//  * a state for a history that already exists is not made here column by column: the batched encoder exports every block's
//    state at each user's last row in its own pass and lru_state_seed_kernel (below) writes the table rows.
#include "lr_common.h"
#include "lr_profile.h"

#define SR 16  // users per workgroup

__device__ const float st_erf_tab[LR_ERF_NINT * (LR_ERF_DEG + 1)] = LR_ERF_TABLE;  // same table as lru_encoder.hip

struct StateParams {
  const float* img;
  LrLruLayout lay;
  char* states;
  size_t row_bytes;
  int num_slots;
  const int32_t* slots;    // [B] or null: row u -> slot u
  const int64_t* new_ids;  // [B][Ln] or null when Ln == 0
  int B, Ln;
  float* out_q;            // [B][64] or null
};

// ---- the encoder's helpers, copied so that lru_encoder.hip stays as it is (same text -> same instruction chains) ----
__device__ __forceinline__ float st_wave_sum64(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}

// LayerNorm over the 64 features held one per lane.
__device__ __forceinline__ float st_wave_layer_norm(float x, float w, float b) {
  float mean = st_wave_sum64(x) * 0.015625f;
  float d = x - mean;
  float var = st_wave_sum64(d * d) * 0.015625f;
  float rstd = 1.0f / sqrtf(var + LR_LN_EPS);
  return lr_fma(d * rstd, w, b);
}

// out[r][tid] = bias[tid] + sum_k wt[k][tid] * in[r][k]   for all SR rows (K = 64, 256 outputs)
__device__ __forceinline__ void st_proj_64_to_256(const float* __restrict__ wt, float bias, const float (*in)[64], int tid,
                                                  float* acc) {
#pragma unroll
  for (int t = 0; t < SR; ++t) acc[t] = bias;
#pragma unroll 4
  for (int k = 0; k < 64; k += 4) {
    float w0 = wt[(k + 0) * 256 + tid], w1 = wt[(k + 1) * 256 + tid];
    float w2 = wt[(k + 2) * 256 + tid], w3 = wt[(k + 3) * 256 + tid];
#pragma unroll
    for (int t = 0; t < SR; ++t) {
      float4 x4 = *reinterpret_cast<const float4*>(&in[t][k]);
      acc[t] = lr_fma(w0, x4.x, acc[t]);
      acc[t] = lr_fma(w1, x4.y, acc[t]);
      acc[t] = lr_fma(w2, x4.z, acc[t]);
      acc[t] = lr_fma(w3, x4.w, acc[t]);
    }
  }
}

// acc[tt] = bias[lane] + sum_k wt[k][lane] * in[4*wave+tt][k]   (K = 256, 64 outputs per row)
__device__ __forceinline__ void st_proj_256_to_64(const float* __restrict__ wt, float bias, const float (*in)[256], int wave,
                                                  int lane, float* acc) {
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) acc[tt] = bias;
#pragma unroll 8
  for (int k = 0; k < 256; k += 4) {
    float w0 = wt[(k + 0) * 64 + lane], w1 = wt[(k + 1) * 64 + lane];
    float w2 = wt[(k + 2) * 64 + lane], w3 = wt[(k + 3) * 64 + lane];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      float4 h4 = *reinterpret_cast<const float4*>(&in[4 * wave + tt][k]);
      acc[tt] = lr_fma(w0, h4.x, acc[tt]);
      acc[tt] = lr_fma(w1, h4.y, acc[tt]);
      acc[tt] = lr_fma(w2, h4.z, acc[tt]);
      acc[tt] = lr_fma(w3, h4.w, acc[tt]);
    }
  }
}

// A block's tail for all SR rows: bu holds h, xs the block's input; leaves the block's output in xs.
// Re(W_out h + b_out) + x -> LN -> GELU(W1 y + b1) -> W2 a + b2 + y -> LN. Every thread of the workgroup calls it; bu and
// xs must be complete (a barrier behind their last write), and it ends behind a barrier.
__device__ __forceinline__ void st_block_tail(const float* img, const LrLruBlockLayout& BL, float (*xs)[64], float (*bu)[256],
                                              float (*ys)[64], int tid, int wave, int lane) {
  float a4[4], acc[SR];
  st_proj_256_to_64(img + BL.out_wt, img[BL.out_b + lane], bu, wave, lane, a4);
  {
    float w = img[BL.ln1_w + lane], bb = img[BL.ln1_b + lane];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      float y0 = a4[tt] + xs[4 * wave + tt][lane];
      ys[4 * wave + tt][lane] = st_wave_layer_norm(y0, w, bb);
    }
  }
  __syncthreads();
  st_proj_64_to_256(img + BL.w1t, img[BL.b1 + tid], ys, tid, acc);
#pragma unroll
  for (int t = 0; t < SR; ++t) bu[t][tid] = lr_gelu_tab(acc[t], st_erf_tab);
  __syncthreads();
  st_proj_256_to_64(img + BL.w2t, img[BL.b2 + lane], bu, wave, lane, a4);
  {
    float w = img[BL.ln2_w + lane], bb = img[BL.ln2_b + lane];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      float z0 = a4[tt] + ys[4 * wave + tt][lane];
      xs[4 * wave + tt][lane] = st_wave_layer_norm(z0, w, bb);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void lru_state_advance_kernel(StateParams p) {
  __shared__ __attribute__((aligned(16))) float xs[SR][64];   // block input x (per user)
  __shared__ __attribute__((aligned(16))) float bu[SR][256];  // gamma*(W_in x+b) -> h -> FFN hidden
  __shared__ __attribute__((aligned(16))) float ys[SR][64];   // after the LRU layer's LayerNorm
  __shared__ __attribute__((aligned(16))) float xl[SR][64];   // the last block's input at the row's last consumed token
  __shared__ int s_slot[SR];   // the row's slot, -1: no such user or a slot outside the table (the row is inert)
  __shared__ int s_live[SR];   // tokens since reset, before the current column
  __shared__ int s_seen[SR];   // 1: the row consumed a token in this call
  __shared__ int s_row[SR];    // the current column's embedding row, -1: the row sits this column out

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u0 = blockIdx.x * SR;
  const int nb = p.lay.num_blocks;
  const float* img = p.img;
  const int q_off = nb * 2 * LR_H, live_off = q_off + 64;  // in floats from the start of a table row

  if (tid < SR) {
    const int u = u0 + tid;
    int slot = -1, live = 0;
    if (u < p.B) {
      const int s = p.slots ? p.slots[u] : u;
      if (s >= 0 && s < p.num_slots) {
        slot = s;
        live = reinterpret_cast<const int*>(p.states + (size_t)s * p.row_bytes)[live_off];
      }
    }
    s_slot[tid] = slot;
    s_live[tid] = live;
    s_seen[tid] = 0;
  }
  __syncthreads();

  const float eln_w = img[p.lay.emb_ln_w + lane], eln_b = img[p.lay.emb_ln_b + lane];

  for (int j = 0; j < p.Ln; ++j) {
    int take = 0;
    if (tid < SR) {
      int row = -1;
      if (s_slot[tid] >= 0) {
        long long id = p.new_ids[(size_t)(u0 + tid) * p.Ln + j];
        if (id > 0) row = id > p.lay.num_items ? 0 : (int)id;  // ids <= 0 are skipped; past the catalog: the encoder's row 0
      }
      s_row[tid] = row;
      take = row >= 0;
    }
    if (!__syncthreads_or(take)) continue;  // workgroup-uniform

    // ---- embedding gather + LayerNorm: wave w owns rows 4w..4w+3, lane = feature
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int r = 4 * wave + tt, row = s_row[r];
      float v = 0.0f;
      if (row >= 0) v = st_wave_layer_norm(img[p.lay.item_emb + (size_t)row * 64 + lane], eln_w, eln_b);
      xs[r][lane] = v;
    }
    __syncthreads();

#pragma unroll
    for (int b = 0; b < LR_MAX_LRU_BLOCKS; ++b) {
      if (b < nb) {
        const LrLruBlockLayout& BL = p.lay.blk[b];
        if (b == nb - 1) {  // what the call's one tail of the last block adds back and normalises
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) {
            const int r = 4 * wave + tt;
            if (s_row[r] >= 0) xl[r][lane] = xs[r][lane];
          }
        }
        {  // ---- in_proj (complex, input imag == 0) and gamma
          float acc[SR];
          st_proj_64_to_256(img + BL.in_wt, img[BL.in_b + tid], xs, tid, acc);
          float g = img[BL.gamma + (tid & 127)];
#pragma unroll
          for (int t = 0; t < SR; ++t) bu[t][tid] = acc[t] * g;
        }
        __syncthreads();
        {  // ---- one recurrence step per (row, channel): thread -> channel tid & 127 of rows (tid >> 7) + 2 i
          const int c = tid & 127;
          const float lr_ = img[BL.lam_re + c], li = img[BL.lam_im + c];
#pragma unroll
          for (int i = 0; i < SR / 2; ++i) {
            const int r = (tid >> 7) + 2 * i;
            if (s_row[r] >= 0) {
              float* hrow = reinterpret_cast<float*>(p.states + (size_t)s_slot[r] * p.row_bytes) + b * 2 * LR_H;
              float h_r = bu[r][c], h_i = bu[r][128 + c];
              if (s_live[r] != 0) {  // not for a reset row's first token: there h = bu, as the encoder starts a history
                const float pr = hrow[c], pi = hrow[128 + c];
                const float nr = lr_fma(lr_, pr, lr_fma(-li, pi, h_r));
                const float ni = lr_fma(lr_, pi, lr_fma(li, pr, h_i));
                h_r = nr;
                h_i = ni;
              }
              hrow[c] = h_r;
              hrow[128 + c] = h_i;
              bu[r][c] = h_r;
              bu[r][128 + c] = h_i;
            }
          }
        }
        __syncthreads();
        if (b < nb - 1) st_block_tail(img, BL, xs, bu, ys, tid, wave, lane);
      }
    }
    if (tid < SR && s_row[tid] >= 0) {
      if (s_live[tid] < 0x7fffffff) s_live[tid] += 1;
      s_seen[tid] = 1;
    }
    __syncthreads();
  }

  // ---- the last block's tail, once, for the rows that consumed a token; the others keep their stored q
  if (__syncthreads_or(tid < SR && s_seen[tid])) {
    const LrLruBlockLayout& BL = p.lay.blk[nb - 1];
    const int c = tid & 127;
#pragma unroll
    for (int i = 0; i < SR / 2; ++i) {  // h of the last block: each thread reads back the elements it wrote
      const int r = (tid >> 7) + 2 * i;
      float h_r = 0.0f, h_i = 0.0f;
      if (s_seen[r]) {
        const float* hrow = reinterpret_cast<const float*>(p.states + (size_t)s_slot[r] * p.row_bytes) + (nb - 1) * 2 * LR_H;
        h_r = hrow[c];
        h_i = hrow[128 + c];
      }
      bu[r][c] = h_r;
      bu[r][128 + c] = h_i;
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int r = 4 * wave + tt;
      xs[r][lane] = s_seen[r] ? xl[r][lane] : 0.0f;
    }
    __syncthreads();
    st_block_tail(img, BL, xs, bu, ys, tid, wave, lane);
  }

#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    const int r = 4 * wave + tt, u = u0 + r;
    if (u < p.B) {
      float q = 0.0f;  // an inert row answers zeros
      if (s_slot[r] >= 0) {
        float* row = reinterpret_cast<float*>(p.states + (size_t)s_slot[r] * p.row_bytes);
        if (s_seen[r]) {
          q = xs[r][lane];
          row[q_off + lane] = q;
        } else {
          q = row[q_off + lane];
        }
      }
      if (p.out_q) p.out_q[(size_t)u * 64 + lane] = q;
    }
  }
  if (tid < SR && s_seen[tid])
    reinterpret_cast<int*>(p.states + (size_t)s_slot[tid] * p.row_bytes)[live_off] = s_live[tid];
}

// One workgroup per listed slot: zero the row (an all-zero row IS the reset state). Slots outside the table are skipped.
__global__ __launch_bounds__(256) void lru_state_reset_kernel(char* states, size_t row_bytes, int num_slots,
                                                              const int32_t* slots) {
  const int s = slots[blockIdx.x];
  if (s < 0 || s >= num_slots) return;
  uint32_t* row = reinterpret_cast<uint32_t*>(states + (size_t)s * row_bytes);
  for (int i = threadIdx.x; i < (int)(row_bytes / 4); i += 256) row[i] = 0u;
}

// ---- states seeded by the batched encoder (lru_encoder_mfma.hip, EXPORT) ----------------------------------------------
// The encoder's pass over whole histories has every block's recurrence state at each user's last row: blocks 0 .. nb-2 in
// the export buffers, one float4 per lane of the scan (lane l holds re of channels sc_k, sc_k + 2, then their im, with
// sc_k = (l >> 5) * 64 + 4 * (l & 15) + ((l >> 4) & 1)), the last block in Ul in channel order. One workgroup per user of
// the chunk writes the table row: h in the table's channel order (the lane permutation is undone here), q from the call's
// out_q row, live from em_live_kernel's count. A history whose LAST id is <= 0 is outside the states' contract (the
// encoder embeds that pad as a token, a state skips it): its row is written as the reset state. The slot guard is the
// advance kernel's.
struct SeedParams {
  char* states;
  size_t row_bytes;
  int num_slots;
  const int32_t* slots;  // [users] of this chunk or null: user u -> slot slot0 + u
  int slot0;
  const int64_t* ids;    // [users][L] of this chunk
  int users, L, nb;
  const int* n;          // [users] live tokens
  const float* exp;      // [nb - 1] blocks of exp_block_floats, [users][256] each, lane order
  size_t exp_block_floats;
  const float* Ul;       // [users][256] the last block's state, channel order
  const float* q;        // [users][64]
};

__global__ __launch_bounds__(256) void lru_state_seed_kernel(SeedParams p) {
  const int u = blockIdx.x, tid = threadIdx.x;
  const int s = p.slots ? p.slots[u] : p.slot0 + u;
  if (s < 0 || s >= p.num_slots) return;
  float* row = reinterpret_cast<float*>(p.states + (size_t)s * p.row_bytes);
  const bool ok = p.ids[(size_t)u * p.L + (p.L - 1)] > 0;
  const int c = tid & 127;  // element tid of h[b] = re (tid < 128) or im of channel c
  const int src = 4 * ((c >> 6) * 32 + (c & 1) * 16 + ((c & 63) >> 2)) + ((c >> 1) & 1) + 2 * (tid >> 7);
  for (int b = 0; b < p.nb; ++b) {
    float v = 0.0f;
    if (ok) v = b < p.nb - 1 ? p.exp[(size_t)b * p.exp_block_floats + (size_t)u * 256 + src] : p.Ul[(size_t)u * 256 + tid];
    row[b * 2 * LR_H + tid] = v;
  }
  const int q_off = p.nb * 2 * LR_H;
  if (tid < 64) row[q_off + tid] = ok ? p.q[(size_t)u * 64 + tid] : 0.0f;
  else if (tid == 64) reinterpret_cast<int*>(row)[q_off + 64] = ok ? p.n[u] : 0;
}

int lr_launch_lru_state_seed(const lr_lru* h, void* states, int num_slots, const int32_t* slots, int slot0, const int64_t* ids,
                             int users, int L, const int* n, const float* exp, size_t exp_block_floats, const float* Ul,
                             const float* q, hipStream_t st) {
  if (users <= 0) return LR_OK;
  SeedParams p;
  p.states = (char*)states;
  p.row_bytes = lr_lru_state_row_bytes(h->lay.num_blocks);
  p.num_slots = num_slots;
  p.slots = slots;
  p.slot0 = slot0;
  p.ids = ids;
  p.users = users;
  p.L = L;
  p.nb = h->lay.num_blocks;
  p.n = n;
  p.exp = exp;
  p.exp_block_floats = exp_block_floats;
  p.Ul = Ul;
  p.q = q;
  hipLaunchKernelGGL(lru_state_seed_kernel, dim3(users), dim3(256), 0, st, p);
  LR_CHECK_LAUNCH("lru_state_seed_kernel");
  return LR_OK;
}

int lr_launch_lru_state_reset(const lr_lru* h, void* states, int num_slots, const int32_t* slots, int B, hipStream_t st) {
  const size_t row_bytes = lr_lru_state_row_bytes(h->lay.num_blocks);
  if (!slots) {
    LR_CHECK_HIP(hipMemsetAsync(states, 0, (size_t)num_slots * row_bytes, st));
    return LR_OK;
  }
  if (B <= 0) return LR_OK;
  hipLaunchKernelGGL(lru_state_reset_kernel, dim3(B), dim3(256), 0, st, (char*)states, row_bytes, num_slots, slots);
  LR_CHECK_LAUNCH("lru_state_reset_kernel");
  return LR_OK;
}

int lr_launch_lru_state_advance(const lr_lru* h, void* states, int num_slots, const int32_t* slots, const int64_t* new_ids,
                                int B, int Ln, float* out_q, hipStream_t st) {
  if (B <= 0) return LR_OK;
  StateParams p;
  p.img = h->img;
  p.lay = h->lay;
  p.states = (char*)states;
  p.row_bytes = lr_lru_state_row_bytes(h->lay.num_blocks);
  p.num_slots = num_slots;
  p.slots = slots;
  p.new_ids = new_ids;
  p.B = B;
  p.Ln = new_ids ? Ln : 0;
  p.out_q = out_q;
  LrProfScope prof(LR_PROF_LRU_ENCODE, (double)B, st);  // the profiler's encoder kind: this is the encoder's step form
  hipLaunchKernelGGL(lru_state_advance_kernel, dim3((B + SR - 1) / SR), dim3(256), 0, st, p);
  LR_CHECK_LAUNCH("lru_state_advance_kernel");
  return LR_OK;
}
