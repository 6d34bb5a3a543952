// llama_attn_cached.hip -- causal varlen attention whose query rows and key rows are different sets (ranker sessions,
// DESIGN 16): segment b has q_len[b] query rows of THIS call at prompt positions cached_len[b] .. cached_len[b] + q_len[b] - 1
// and reads its kv_len[b] = cached_len[b] + q_len[b] keys and values from the user's cache slot, whose row p is
// [K rotated | V] of position p (width 2 nkv hd: the row format of the one-query-row kernels). Query row i sees keys
// 0 .. cached_len[b] + i. The call's own K | V rows are copied into the slot first (kv_cache_write_kernel), so the attention
// has one K / V source.
//
//  kv_cache_meta_kernel        : per new row its position (and, on request, its cache row's offset); per prompt its last row
//                                 and that row's position
//  kv_cache_write_kernel       : K | V columns of the call's packed rows -> slot rows cached_len[b] ..
//  attn_cached_generic_kernel  : any head_dim <= 256, GQA, one wave per (query row, head): the text attn_generic_kernel
//                                 (llama_attn.hip) runs, attn_generic_row of llama_attn_generic_body.h, on the slot's rows
//  attn_cached128_kernel       : head_dim 128: the body attn_mfma128_kernel (llama_attn.hip) runs, attn_hd128_body of
//                                 llama_attn_hd128_body.h, with the K / V source and the row ownership its own: query tiles
//                                 and 64-key blocks stay aligned to positions inside the prompt, a key block's LDS image
//                                 (swizzles, zero rows past the prompt's end) is the one that kernel builds, and the body runs
//                                 the same lines on it. That is why a row's bits equal the whole-prompt kernel's. LASTQ = its
//                                 one-query-row mode: one row per prompt, the query at position kv_len - 1 (the pruned last
//                                 layer).
// The two bodies are instantiated here, in a translation unit of their own: the whole-prompt code object holds no cached kernel.
#include "llama_attn_generic_body.h"
#include "llama_attn_hd128_body.h"


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

// row_off (optional, with slots): the element offset of row r's cache row inside a layer of the table, slots[b] * slot_elems +
// position * kv_w -- what kv_cache_write_kernel computes per layer, once per call for the reduce pass that writes the cache
// (LrGemmKvScatter)
__global__ __launch_bounds__(256) void kv_cache_meta_kernel(const int32_t* cu, const int32_t* cached_len, int B, int n,
                                                            int32_t* tok_pos, int32_t* last_rows, int32_t* last_pos,
                                                            const int32_t* slots, long long slot_elems, int kv_w,
                                                            long long* row_off) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n) {
    const int b = kc_segment_of(cu, B, r);
    const int pos = cached_len[b] + r - cu[b];
    tok_pos[r] = pos;
    if (row_off) row_off[r] = (long long)slots[b] * slot_elems + (long long)pos * kv_w;
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
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);  // (query row, head)
  if (item >= n_rows * nh) return;
  // q_rows (optional): only these packed rows are evaluated and the output is compact [n_rows][nh * hd]
  const int orow = item / nh, h = item % nh;
  const int tok = q_rows ? q_rows[orow] : orow;
  const int kvh = h / (nh / nkv);
  const int b = kc_segment_of(cu, B, tok);
  const u16* kbase = kv + (size_t)slots[b] * slot_elems + kvh * hd;   // the row of position p is row p of the slot
  attn_generic_row(q + (size_t)tok * q_ld + h * hd, kbase, kbase + nkv * hd, 2 * nkv * hd, cached_len[b] + tok - cu[b], hd,
                   1.0f / sqrtf((float)hd), 0.f, 0, out + (size_t)orow * nh * hd + h * hd, nullptr);
}

// =============================================================================================
// MFMA, head_dim 128 (the body: llama_attn_hd128_body.h)
// =============================================================================================
// grid (query tiles of the call's longest new part, nh, B). A workgroup's tile is tile cached_len / 128 + (its x from the
// end: heavy tiles first) of the prompt's positions; rows of the tile at positions < cached_len (they are cached, not this
// call's) or >= kv_len are computed on a clamped row and not stored. LASTQ: grid (1, nh, B), q / out hold one row per prompt.
template <bool LASTQ>
__global__ __launch_bounds__(256, 2) void attn_cached128_kernel(const u16* __restrict__ q, int q_ld, u16* out,
                                                                const u16* __restrict__ kv, long long slot_elems,
                                                                const int32_t* slots, const int32_t* cached_len,
                                                                const int32_t* cu, int nh, int nkv) {
  const int seg = blockIdx.z, h = blockIdx.y;
  const int q0 = cu[seg];
  const int c = cached_len[seg];          // keys [0, c) were cached by earlier calls
  const int T = c + cu[seg + 1] - q0;     // sequence length, cached part included
  int qb;
  if (LASTQ) {
    qb = (T - 1) / FA_QROWS;
  } else {
    qb = c / FA_QROWS + ((int)gridDim.x - 1 - (int)blockIdx.x);
    if (qb * FA_QROWS >= T) return;  // no query row of this prompt in the tile
  }
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const FaSeg sg{q0, c, T, q0 - c};   // the call's packed row of position p >= c is q0 - c + p
  const u16* kbase = kv + (size_t)slots[seg] * (size_t)slot_elems + kvh * FA_HD;   // the row of position p is row p of the slot
  const FaKV rows{kbase, kbase + nkv * FA_HD, nullptr, nullptr, 2 * nkv * FA_HD};
  // Every block is fetched through a per-block buffer descriptor: base = the block's first K (V) row in the slot,
  // num_records = the bytes up to the end of row T - 1, so rows past the sequence end -- slot rows an earlier, longer prompt
  // may have left behind -- are range-checked to ZERO by the hardware, as the whole-prompt kernel's are (those keys are
  // causally masked for every stored query row: P = 0 exactly).
  auto stage = [&](int kb, char* base, const unsigned (&koff)[4], const unsigned (&voff)[4]) {
    fa_stage_block<false, FA_HD, FA_KB, 4, FA_TILE_BYTES>(base, rows, sg, kb, koff, voff, nullptr);   // (no row's home to ask for)
  };

  Fa128Src src;
  src.T = T; src.P = c; src.qb = qb; src.h = h; src.nh = nh;
  src.kv_stride = rows.stride;
  src.q = q;
  src.q_ld = q_ld;
  src.out = out;
  src.lse = nullptr;
  src.row0 = LASTQ ? seg : sg.vtok0;
  attn_hd128_body<false, LASTQ>(src, stage, Fa128Stamps{});
}

// =============================================================================================
// launchers (declared in llama_kernels.h)
// =============================================================================================
int lr_launch_kv_cache_meta(const int32_t* cu, const int32_t* cached_len, int B, int n, int32_t* tok_pos, int32_t* last_rows,
                            int32_t* last_pos, hipStream_t st, const int32_t* slots, long long slot_elems, int kv_w,
                            long long* row_off) {
  if (n <= 0 || B <= 0) return LR_OK;
  if (row_off && (!slots || kv_w % 4 != 0 || slot_elems % 4 != 0))
    LR_FAIL(LR_EINVAL, "kv cache meta: row offsets need the slots and rows of 8-byte pieces (kv_w %d)", kv_w);
  LrProfScope prof(LR_PROF_ELEMENTWISE, 0, st);
  const int rows = n > B ? n : B;
  hipLaunchKernelGGL(kv_cache_meta_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, cu, cached_len, B, n, tok_pos, last_rows,
                     last_pos, slots, slot_elems, kv_w, row_off);
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
    const int tiles = ((int)T - 1) / FA_QROWS - (int)c / FA_QROWS + 1;
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
    LR_RUN(lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_cached128_kernel<true>), FA_LDS_BYTES, lds_set_last));
    hipLaunchKernelGGL(attn_cached128_kernel<true>, dim3(1, nh, B), dim3(256), FA_LDS_BYTES, st, a.q, a.q_ld, a.out, a.kv,
                       a.slot_elems, a.slots, a.cached_len, a.cu, nh, nkv);
    LR_CHECK_LAUNCH("attn_cached128_kernel<last>");
  } else {
    LR_RUN(lr_ensure_dynamic_lds(reinterpret_cast<const void*>(attn_cached128_kernel<false>), FA_LDS_BYTES, lds_set));
    hipLaunchKernelGGL(attn_cached128_kernel<false>, dim3(max_tiles, nh, B), dim3(256), FA_LDS_BYTES, st, a.q, a.q_ld, a.out,
                       a.kv, a.slot_elems, a.slots, a.cached_len, a.cu, nh, nkv);
    LR_CHECK_LAUNCH("attn_cached128_kernel");
  }
  return LR_OK;
}
