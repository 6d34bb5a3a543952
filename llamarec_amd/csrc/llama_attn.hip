// llama_attn.hip -- varlen causal self-attention over packed prompts on gfx950.
//
// Replaces flash-attn 2.5.8's CUDA varlen kernel (train_ranker.py:61, attn_implementation=
// "flash_attention_2") / HF eager attention inside LlamaModel (reached from model/llm.py:89-100).
// Packed (unpadded) execution is legal because padding is on the left and masked
// (SURVEY.md 8(a) a15); positions restart at 0 in every prompt.
//
//  attn_generic_kernel : any head_dim <= 256, GQA, one wave per (token, head). Test models. A row's arithmetic is
//    attn_generic_row (llama_attn_generic_body.h), shared with attn_cached_generic_kernel (llama_attn_cached.hip).
//  attn_mfma128_kernel : head_dim = 128, flash-style online softmax on v_mfma_f32_16x16x32_bf16 (attention variant 2 and its
//    one-query-row mode). Everything from the Q fragments to the store is attn_hd128_body (llama_attn_hd128_body.h: the
//    transposed products, the LDS layout and the softmax are described there), shared with attn_cached128_kernel
//    (llama_attn_cached.hip). Here stand the prologue (workgroup -> segment, head, query tile), where the rows of Q and out
//    are, and the staging of a key block.
//    Shared prompt prefix (prefix_len = P > 0): segment 0 of the packed batch holds the P tokens every prompt
//    starts with (the template text, dataloader/utils.py:24-40), segment s >= 1 the rest of prompt s-1 at
//    positions P.. . Such a segment's keys [0, P) are read from segment 0's rows; query tiles and key blocks stay
//    aligned to ABSOLUTE positions, so every row executes exactly the instruction sequence of the unshared run.
#include <stdlib.h>

#include "llama_attn_generic_body.h"
#include "llama_attn_hd128_body.h"

// =============================================================================================
// generic
// =============================================================================================
__global__ __launch_bounds__(256) void attn_generic_kernel(const u16* qkv, u16* out, const int32_t* cu, int B,
                                                           int n_tok, int nh, int nkv, int hd,
                                                           const int32_t* q_rows, float* lse, float scale_arg, float cap,
                                                           int window) {
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);  // (token, head)
  if (item >= n_tok * nh) return;
  // q_rows (optional): only these query tokens are evaluated and the output is compact [n_tok][nh*hd]
  const int orow = item / nh, h = item % nh;
  const int tok = q_rows ? q_rows[orow] : orow;
  const int kvh = h / (nh / nkv);
  const int stride = (nh + 2 * nkv) * hd;
  int lo = 0, hi = B;  // prompt index: largest b with cu[b] <= tok
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (cu[mid] <= tok) lo = mid; else hi = mid;
  }
  const int s0 = cu[lo];
  const u16* kbase = qkv + (size_t)s0 * stride + (nh + kvh) * hd;
  const float scale = scale_arg > 0.f ? scale_arg : 1.0f / sqrtf((float)hd);   // 0: the head_dim's own
  attn_generic_row(qkv + (size_t)tok * stride + h * hd, kbase, kbase + nkv * hd, stride, tok - s0, hd, scale, cap, window,
                   out + (size_t)orow * nh * hd + h * hd, lse ? lse + (size_t)orow * nh + h : nullptr);
}

// =============================================================================================
// MFMA, head_dim 128 (the body: llama_attn_hd128_body.h)
// =============================================================================================
__device__ unsigned long long g_attn_stamps[64 * 8];
#ifdef LR_EXPERIMENTS
__device__ unsigned long long g_attn_wg[FA_WG_TRACE * 8];
#else
__device__ unsigned long long g_attn_wg[8];   // never written: the stamped instantiation exists in experiment builds only
#endif

// LASTQ (the pruned last layer, api_llama.hip): only each prompt's LAST query row is evaluated. `qkv` is then the
// [rows][2 * nkv * hd] K | V projection of every row, `q_last` holds one rotated query row per prompt ([prompt][nh * hd]),
// a workgroup = one (prompt, head) walks all the prompt's key blocks, and `out` receives one row per prompt
// ([prompt][nh * hd]).
template <bool STAMP, bool LASTQ = false>
__global__ __launch_bounds__(256, 2) void attn_mfma128_kernel(const u16* __restrict__ qkv, u16* out,
                                                              const int32_t* cu, int prefix_len, int nh, int nkv,
                                                              int max_qblocks, int n_pairs,
                                                              const u16* __restrict__ q_rows_last, float* lse) {
  Fa128Stamps sp;
  sp.acc_out = g_attn_stamps;
  sp.wg_out = g_attn_wg;
  FA_RT(sp.rt_entry)
  if (STAMP) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(sp.t_prev)::"memory");
  const int hd = FA_HD;
  // ---- workgroup -> (segment, head, query tile). A (segment, head) PAIR is bound to one of 8 dispatch streams
  // (blocks b and b + 8 are observed to share an XCD: speed only, never correctness), so the 3..12 query tiles that
  // re-read one pair's K/V hit that XCD's L2; inside a stream the pairs' heavy tiles (qb >= 2, heaviest first) run pair
  // after pair, and the two lightest tiles of every pair are kept for the end, where they fill the tail of the launch
  // (a causal tile costs ~ its key-block count 2 qb + 2: launched last, a heavy tile would leave most CUs idle).
  int seg, h, qb;
  if (LASTQ) {
    const int id = blockIdx.x, stream = id & 7, pl = id >> 3;
    const int pair = pl * 8 + stream;
    if (pair >= n_pairs) return;
    seg = __builtin_amdgcn_readfirstlane(pair / nh);
    h = __builtin_amdgcn_readfirstlane(pair - seg * nh);
    if (prefix_len > 0 && seg == 0) return;   // segment 0 is the shared prefix, not a prompt
    qb = 0;                                    // set below, once T is known
  } else {
    int pair;
    fa_tile_of_workgroup(n_pairs, max_qblocks, pair, qb);
    if (pair >= n_pairs) return;
    // the integer divisions above run on the vector ALU (there is no scalar divide): hand the wave-uniform results
    // back to scalar registers, or every buffer descriptor built from them is wrapped in a waterfall loop
    seg = __builtin_amdgcn_readfirstlane(pair / nh);
    h = __builtin_amdgcn_readfirstlane(pair - seg * nh);
    qb = __builtin_amdgcn_readfirstlane(qb);
  }
  const int tok0 = cu[seg];
  const int P = (prefix_len > 0 && seg > 0) ? prefix_len : 0;  // keys [0, P) live in segment 0's rows [0, P)
  const int T = P + cu[seg + 1] - tok0;                        // sequence length, prefix included
  if (LASTQ) qb = (T - 1) / FA_QROWS;
  if (qb * FA_QROWS >= T || (qb + 1) * FA_QROWS <= P) return;  // no query row of this segment in the tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kvh = __builtin_amdgcn_readfirstlane(h / (nh / nkv));
  const int stride = LASTQ ? 2 * nkv * hd : (nh + 2 * nkv) * hd;
  const int koff0 = LASTQ ? kvh * hd : (nh + kvh) * hd, voff0 = koff0 + nkv * hd;
  const int vtok0 = tok0 - P;  // the row of position p >= P is vtok0 + p (tok0 >= P: segment 0 precedes it)
  const u16* kbase = qkv + (size_t)vtok0 * stride + koff0;
  const u16* vbase = qkv + (size_t)vtok0 * stride + voff0;
  const u16* pkbase = qkv + koff0;        // prefix rows start at packed row 0
  const u16* pvbase = qkv + voff0;

  // A block that lies inside the segment's own rows is fetched through a per-block buffer descriptor: base = the
  // block's first K (V) row, num_records = the bytes up to the end of the segment's last row, so rows past the sequence
  // end are range-checked to ZERO by the hardware (those keys are causally masked for every stored query row: P = 0
  // exactly, whatever finite bytes K and V hold -- same bits as fetching a clamped row). Descriptor, LDS base (M0) and
  // block offset are scalar work; the per-lane offsets koff / voff are block-invariant: no vector ALU in the staging.
  const int prow = lane >> 4, ppos = lane & 15;
  auto stage = [&](int kb, char* base, const unsigned (&koff)[4], const unsigned (&voff)[4]) {
    if (kb * FA_KB >= P) {
      const size_t blk_off = (size_t)kb * FA_KB * stride * 2;
      const int records = ((T - 1 - kb * FA_KB) * stride + hd) * 2;  // bytes from the block's first K (V) element
      const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
      const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa_dma16(rk, base + i * 1024, koff[i]);
        fa_dma16(rv, base + FA_TILE_BYTES + i * 1024, voff[i]);
      }
    } else {  // the block holds shared-prefix keys: rows < P come from segment 0 (per-lane addresses)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 4 + prow;
        const int key = min(kb * FA_KB + row, T - 1);
        const int kchunk = ppos ^ (row & 15);
        const int vchunk = ppos ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const u16* kr = key < P ? pkbase : kbase;
        const u16* vr = key < P ? pvbase : vbase;
        fa_glds16(kr + (size_t)key * stride + kchunk * 8, base + i * 1024);
        fa_glds16(vr + (size_t)key * stride + vchunk * 8, base + FA_TILE_BYTES + i * 1024);
      }
    }
  };

  Fa128Src src;
  src.T = T; src.P = P; src.qb = qb; src.h = h; src.nh = nh;
  src.kv_stride = stride;
  src.q = LASTQ ? q_rows_last : qkv;
  src.q_ld = LASTQ ? nh * hd : stride;
  src.out = out;
  src.lse = lse;
  src.row0 = LASTQ ? (prefix_len > 0 ? seg - 1 : seg) : vtok0;
  attn_hd128_body<STAMP, LASTQ>(src, stage, sp);
}

#ifdef LR_EXPERIMENTS
extern "C" int lr_debug_attn_wg_trace(unsigned long long* out, int n) {
  if (!out || n < 1 || n > FA_WG_TRACE * 8) LR_FAIL(LR_EINVAL, "lr_debug_attn_wg_trace: bad arguments");
  LR_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_wg), (size_t)n * sizeof(unsigned long long)));
  return LR_OK;
}
extern "C" int lr_debug_attn_stamps(unsigned long long* out, int n) {
  if (!out || n < 1 || n > 64 * 8) LR_FAIL(LR_EINVAL, "lr_debug_attn_stamps: bad arguments");
  LR_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_stamps), (size_t)n * sizeof(unsigned long long)));
  return LR_OK;
}
#endif

// attention for a list of query tokens only (the last layer needs just each prompt's last token)
int lr_launch_attention_rows(const u16* qkv, u16* out, const int32_t* cu, int B, const int32_t* q_rows,
                             int n_rows, int nh, int nkv, int hd, hipStream_t st, float scale, float cap, int window) {
  if (n_rows <= 0) return LR_OK;
  if (window < 0) LR_FAIL(LR_EINVAL, "attention: window %d", window);
  if (hd > 256) LR_FAIL(LR_EUNSUPPORTED, "attention: head_dim %d > 256", hd);
  const int items = n_rows * nh;
  hipLaunchKernelGGL(attn_generic_kernel, dim3((items + 3) / 4), dim3(256), 0, st, qkv, out, cu, B, n_rows,
                     nh, nkv, hd, q_rows, (float*)nullptr, scale, cap, window);
  LR_CHECK_LAUNCH("attn_generic_kernel(rows)");
  return LR_OK;
}

// =============================================================================================
// the table in llama_kernels.h
int lr_resolve_attention(const LrAttnRequest& r, LrAttnKernel* kernel) {
  const int hd = r.hd;
  if (r.cap > 0.f) {   // the short table of llama_kernels.h
    if (r.want_lse) LR_FAIL(LR_EINVAL, "attention: no lse with a soft cap");
    // variants 7 and 8 are a kernel at head_dim 96 only, variant 9 at head_dim 256 only: elsewhere a capped request for them
    // stays the unknown variant it was (LR_EINVAL)
    if (r.variant == 2 || r.variant == 3 || r.variant == 5 || r.variant == 6 || ((r.variant == 7 || r.variant == 8) && hd == 96) ||
        (r.variant == 9 && hd == 256))
      LR_FAIL(LR_EUNSUPPORTED, "attention variant %d has no soft-capped form (0 / 4 at head_dim 256, 1 generic)", r.variant);
    if (r.variant != 0 && r.variant != 1 && r.variant != 4) LR_FAIL(LR_EINVAL, "attention: unknown variant %d", r.variant);
    if (r.variant != 1 && hd == 256 && r.cap <= LR_SOFTCAP_MFMA_MAX) {
      *kernel = LR_ATTN_HD256;
      return LR_OK;
    }
    if (r.prefix_len > 0) LR_FAIL(LR_EUNSUPPORTED, "attention: the generic kernel reads no shared prefix (soft cap, head_dim %d)", hd);
    *kernel = LR_ATTN_GENERIC;
    return LR_OK;
  }
  switch (r.variant) {
    case 0:
      if (hd == 128) *kernel = (r.have_items_ws && !r.prefill) ? LR_ATTN_ROWS256 : LR_ATTN_MFMA128;
      else if (hd == 256 && (r.prefill || r.lora || r.prefix_len > 0)) *kernel = LR_ATTN_HD256;   // lora: with lse, the pair 9 / 9
      else if (hd == 96 && (r.prefill || r.lora || r.prefix_len > 0)) *kernel = LR_ATTN_HD96;   // lora: with lse, the pair 8 / 8
      else *kernel = (hd == 64 && (r.prefill || r.lora || r.prefix_len > 0)) ? LR_ATTN_HD64 : LR_ATTN_GENERIC;
      if (r.prefix_len > 0 && *kernel == LR_ATTN_GENERIC)
        LR_FAIL(LR_EUNSUPPORTED, "attention: no kernel reads a shared prefix at head_dim %d", hd);
      if (r.prefix_len > 0 && r.want_lse && hd != 128)
        LR_FAIL(LR_EINVAL, "attention: no lse with a shared prefix at head_dim %d", hd);
      return LR_OK;
    case 1:
      if (r.prefix_len > 0) LR_FAIL(LR_EUNSUPPORTED, "attention variant 1 (generic) reads no shared prefix");
      *kernel = LR_ATTN_GENERIC;
      return LR_OK;
    case 2: *kernel = LR_ATTN_MFMA128; return LR_OK;
    case 3:
      if (!r.have_items_ws)
        LR_FAIL(LR_EINVAL, "attention variant 3 (256-row tiles) is not available here: it takes an item workspace "
                "(lr_attention_varlen_ws, the prefill)");
      if (hd != 128) LR_FAIL(LR_EUNSUPPORTED, "attention variant 3 needs head_dim 128 (got %d)", hd);
      *kernel = r.prefix_len <= 64 ? LR_ATTN_ROWS256 : LR_ATTN_MFMA128;
      return LR_OK;
    case 4:
      if (r.want_lse) LR_FAIL(LR_EINVAL, "attention variant 4 (head_dim-256 MFMA) writes no lse");
      if (r.prefill && hd != 256) LR_FAIL(LR_EUNSUPPORTED, "attention variant 4 needs head_dim 256 (got %d)", hd);
      *kernel = LR_ATTN_HD256;
      return LR_OK;
    case 5:
      if (r.want_lse) LR_FAIL(LR_EINVAL, "attention variant 5 (head_dim-64 MFMA) writes no lse");
      if (hd != 64) LR_FAIL(LR_EUNSUPPORTED, "attention variant 5 needs head_dim 64 (got %d)", hd);
      *kernel = LR_ATTN_HD64;
      return LR_OK;
    case 6:   // the training pair: variant 5's kernel, with lse when wanted; its backward is llama_attn_bwd_hd64.hip
      if (hd != 64) LR_FAIL(LR_EUNSUPPORTED, "attention variant 6 needs head_dim 64 (got %d)", hd);
      if (r.want_lse && r.prefix_len > 0) LR_FAIL(LR_EINVAL, "attention variant 6 writes no lse with a shared prefix");
      *kernel = LR_ATTN_HD64;
      return LR_OK;
    case 7:
      if (r.want_lse) LR_FAIL(LR_EINVAL, "attention variant 7 (head_dim-96 MFMA) writes no lse");
      if (hd != 96) LR_FAIL(LR_EUNSUPPORTED, "attention variant 7 needs head_dim 96 (got %d)", hd);
      *kernel = LR_ATTN_HD96;
      return LR_OK;
    case 8:   // the training pair: variant 7's kernel, with lse when wanted; its backward is llama_attn_bwd_hd96.hip
      if (hd != 96) LR_FAIL(LR_EUNSUPPORTED, "attention variant 8 needs head_dim 96 (got %d)", hd);
      if (r.want_lse && r.prefix_len > 0) LR_FAIL(LR_EINVAL, "attention variant 8 writes no lse with a shared prefix");
      *kernel = LR_ATTN_HD96;
      return LR_OK;
    case 9:   // the training pair: variant 4's kernel, with lse when wanted; its backward is llama_attn_bwd_hd256.hip
      if (hd != 256) LR_FAIL(LR_EUNSUPPORTED, "attention variant 9 needs head_dim 256 (got %d)", hd);
      if (r.want_lse && r.prefix_len > 0) LR_FAIL(LR_EINVAL, "attention variant 9 writes no lse with a shared prefix");
      *kernel = LR_ATTN_HD256;
      return LR_OK;
  }
  LR_FAIL(LR_EINVAL, "attention: unknown variant %d (0 auto, 1 generic, 2 = head_dim-128 MFMA, 3 = 256-row tiles, "
          "4 = head_dim-256 MFMA, 5 = head_dim-64 MFMA, 6 = head_dim-64 MFMA for training, 7 = head_dim-96 MFMA, "
          "8 = head_dim-96 MFMA for training, 9 = head_dim-256 MFMA for training)", r.variant);
}

int lr_launch_attention(const LrAttnArgs& a, LrAttnKernel kernel, hipStream_t st) {
  const int32_t* cu_host = a.cu_host;
  const int B = a.S, n_tok = a.n_tok, nh = a.nh, nkv = a.nkv, hd = a.hd, prefix_len = a.prefix_len;
  if (n_tok <= 0 || B <= 0) return LR_OK;
  if (a.cap < 0.f || a.scale < 0.f || a.cap != a.cap || a.scale != a.scale)
    LR_FAIL(LR_EINVAL, "attention: scale %g cap %g", (double)a.scale, (double)a.cap);
  if (a.cap > 0.f && kernel != LR_ATTN_HD256 && kernel != LR_ATTN_GENERIC)
    LR_FAIL(LR_EUNSUPPORTED, "attention: kernel %d has no soft-capped form", (int)kernel);
  if (a.window < 0) LR_FAIL(LR_EINVAL, "attention: window %d", a.window);
  if (a.window > 0 && ((kernel != LR_ATTN_HD256 && kernel != LR_ATTN_GENERIC) || prefix_len != 0 || a.lse || a.cap > 0.f))
    LR_FAIL(LR_EUNSUPPORTED, "attention: a sliding window runs on the head_dim-256 MFMA kernel or the generic one, without a "
            "shared prefix, lse or a soft cap (kernel %d, prefix %d)", (int)kernel, prefix_len);
  if (kernel == LR_ATTN_ROWS256) return lr_launch_attention256(a, st);
  if (nh % nkv != 0) LR_FAIL(LR_EINVAL, "attention: num_heads %d not a multiple of num_kv_heads %d", nh, nkv);
  if (kernel == LR_ATTN_HD256) {
    if (prefix_len < 0 || (a.lse && (prefix_len > 0 || a.cap > 0.f)))
      LR_FAIL(LR_EINVAL, "attention: the head_dim-256 MFMA kernel writes no lse with a shared prefix or a soft cap (prefix %d)",
              prefix_len);
    if (a.cap > 0.f) return lr_launch_attention_hd256_softcap(a, st);
    if (a.window > 0) return lr_launch_attention_hd256_window(a, st);
    return prefix_len > 0 ? lr_launch_attention_hd256_prefix(a, st) : lr_launch_attention_hd256(a, st);
  }
  if (kernel == LR_ATTN_HD64) {
    if (prefix_len < 0) LR_FAIL(LR_EINVAL, "attention: shared prefix of %d tokens", prefix_len);
    return prefix_len > 0 ? lr_launch_attention_hd64_prefix(a, st) : lr_launch_attention_hd64(a, st);
  }
  if (kernel == LR_ATTN_HD96) {
    if (prefix_len < 0 || (prefix_len > 0 && a.lse))
      LR_FAIL(LR_EINVAL, "attention: the head_dim-96 MFMA kernel writes no lse with a shared prefix (prefix %d)", prefix_len);
    return prefix_len > 0 ? lr_launch_attention_hd96_prefix(a, st) : lr_launch_attention_hd96(a, st);
  }
  if (prefix_len < 0 || (prefix_len > 0 && (kernel != LR_ATTN_MFMA128 || cu_host[1] - cu_host[0] != prefix_len)))
    LR_FAIL(LR_EINVAL, "attention: shared prefix of %d tokens needs the head_dim-128 MFMA kernel and segment 0 = the prefix",
            prefix_len);
  if (kernel == LR_ATTN_MFMA128) {   // (layout = nullptr: the check above is this kernel's own)
    const char* needs = "attention variant 2 needs head_dim 128";
#ifdef LR_EXPERIMENTS
    const char* stamp_env = getenv("LR_ATTN_STAMPS");
    if (stamp_env && stamp_env[0] == '1') {
      // LR_ATTN_ONE_PER_CU=1: ask for 104 KiB of LDS so that only ONE workgroup fits a CU (what a block costs a lone wave per
      // SIMD). One setting per process: the kernel's dynamic-LDS limit is set once per launcher instantiation.
      const char* one_env = getenv("LR_ATTN_ONE_PER_CU");
      if (one_env && one_env[0] == '1')
        return lr_attn_launch_tiles<attn_mfma128_kernel<true>, FA_HD, FA_QROWS, 256, 104 * 1024, true>(
            "attn_mfma128_kernel", needs, nullptr, nullptr, nullptr, a, st, (const u16*)nullptr, a.lse);
      return lr_attn_launch_tiles<attn_mfma128_kernel<true>, FA_HD, FA_QROWS, 256, FA_LDS_BYTES, true>(
          "attn_mfma128_kernel", needs, nullptr, nullptr, nullptr, a, st, (const u16*)nullptr, a.lse);
    }
#endif
    return lr_attn_launch_tiles<attn_mfma128_kernel<false>, FA_HD, FA_QROWS, 256, FA_LDS_BYTES, true>(
        "attn_mfma128_kernel", needs, nullptr, nullptr, nullptr, a, st, (const u16*)nullptr, a.lse);
  }
  LrProfScope prof(LR_PROF_ATTN_GENERIC, lr_attn_plan(cu_host, B, 0, nh, hd, FA_QROWS, nh).work, st);   // (its work sum only)
  if (hd > 256) LR_FAIL(LR_EUNSUPPORTED, "attention: head_dim %d > 256", hd);
  const int items = n_tok * nh;
  hipLaunchKernelGGL(attn_generic_kernel, dim3((items + 3) / 4), dim3(256), 0, st, a.qkv, a.out, a.cu, B,
                     n_tok, nh, nkv, hd, (const int32_t*)nullptr, a.lse, a.scale, a.cap, a.window);
  LR_CHECK_LAUNCH("attn_generic_kernel");
  return LR_OK;
}

// The pruned last layer (head_dim 128 here, 64, 96 and 256 in the _prefix files of their kernels): kv = [n_tok][2 * nkv * hd] (K | V of every row), q_last = [prompts][nh * hd] rotated query rows
// of each prompt's last token, out_last = [prompts][nh * hd]. cu / cu_host / prefix_len as lr_launch_attention.
int lr_launch_attention_last(const u16* kv, const u16* q_last, u16* out_last, const int32_t* cu, const int32_t* cu_host,
                             int S, int n_tok, int nh, int nkv, int hd, hipStream_t st, int prefix_len, float scale, float cap,
                             int window) {
  if (n_tok <= 0 || S <= 0) return LR_OK;
  if (window < 0) LR_FAIL(LR_EINVAL, "attention (last rows): window %d", window);
  if (window > 0) {
    if (hd != 256 || nkv < 1 || nh % nkv != 0 || prefix_len != 0 || cap > 0.f)
      LR_FAIL(LR_EUNSUPPORTED, "attention (last rows, window): head_dim 256 and nh %% nkv == 0 only, no shared prefix, no cap");
    return lr_launch_attention_hd256_window_last(kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv, window, st);
  }
  if (cap > 0.f) {
    if (hd != 256 || nkv < 1 || nh % nkv != 0)
      LR_FAIL(LR_EUNSUPPORTED, "attention (last rows, soft cap): head_dim 256 and nh %% nkv == 0 only");
    return lr_launch_attention_hd256_softcap_last(kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv, prefix_len, scale, cap, st);
  }
  if ((hd != 128 && hd != 64 && hd != 96 && hd != 256) || nkv < 1 || nh % nkv != 0)
    LR_FAIL(LR_EUNSUPPORTED, "attention (last rows): head_dim 64, 96, 128 or 256 and nh %% nkv == 0 only");
  if (hd == 96) return lr_launch_attention_hd96_last(kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv, prefix_len, st);
  if (hd == 64) return lr_launch_attention_hd64_last(kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv, prefix_len, st);
  if (hd == 256) return lr_launch_attention_hd256_last(kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv, prefix_len, st);
  if (prefix_len < 0 || (prefix_len > 0 && cu_host[1] - cu_host[0] != prefix_len))
    LR_FAIL(LR_EINVAL, "attention (last rows): segment 0 must be the %d-token shared prefix", prefix_len);
  if ((long long)n_tok * 2 * nkv * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention: packed kv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  // (layout = nullptr: the two checks above are this kernel's own.) Its workgroups map to pairs through the dispatch stream
  // id & 7, so the grid is a multiple of 8.
  return lr_attn_launch_last<attn_mfma128_kernel<false, true>, FA_HD, 256, FA_LDS_BYTES, 8>(
      "attn_mfma128_kernel<last>", nullptr, kv, q_last, out_last, cu, cu_host, S, n_tok, nh, nkv, prefix_len, st, (float*)nullptr);
}
