// llama_kernels.h -- internal launcher declarations and bf16 helpers for the stage-2 kernels.
#ifndef LLAMA_KERNELS_H
#define LLAMA_KERNELS_H

#include "lr_common.h"
#include "lr_profile.h"

__device__ __forceinline__ float bf2f(unsigned short b) {
  return __builtin_bit_cast(float, (unsigned int)b << 16);
}
// round-to-nearest-even (v_cvt_pk_bf16_f32 on gfx950; NaN stays NaN)
__device__ __forceinline__ unsigned short f2bf(float f) {
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}
// HF: down_proj(act_fn(gate) * up) with bf16 tensors: gate/up already bf16-valued floats here;
// silu output is rounded to bf16, then the product is rounded to bf16.
// The quotient is g * v_rcp_f32(1 + exp(-g)) (1 ulp, like the v_exp_f32 under __expf): the IEEE division sequence costs
// ten vector instructions per value, 128 values per lane in a gate-up tile's epilogue.
__device__ __forceinline__ unsigned short swiglu_bf16(float g, float u) {
  float s = bf2f(f2bf(g * __builtin_amdgcn_rcpf(1.0f + __expf(-g))));
  return f2bf(s * u);
}

// Gemma's MLP: down_proj(gelu_pytorch_tanh(gate) * up) at swiglu_bf16's rounding points: bf16(gate) in, the activation
// rounded to bf16, the product rounded to bf16. gelu(g) = 0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3))), fp32 (torch's
// bf16 GELU computes in fp32 and rounds once).
__device__ __forceinline__ unsigned short geglu_bf16(float g, float u) {
  const float t = tanhf(0.7978845608028654f * (g + 0.044715f * g * g * g));
  float s = bf2f(f2bf(0.5f * g * (1.0f + t)));
  return f2bf(s * u);
}
// RMSNorm of one value: Llama (style 0) bf16(w * bf16(x * rstd)); Gemma (style 1) bf16(x * rstd * (1 + w)) in fp32
template <int NS>
__device__ __forceinline__ unsigned short rms_apply(unsigned short w, unsigned short x, float rstd) {
  if (NS == 0) return f2bf(bf2f(w) * bf2f(f2bf(bf2f(x) * rstd)));
  return f2bf(bf2f(x) * rstd * (1.0f + bf2f(w)));
}

// epilogue modes of the GEMMs
#define LR_EPI_STORE 0     // C = bf16(acc)
#define LR_EPI_RESIDUAL 1  // C = bf16( bf16(acc) + R )      (R may alias C)
#define LR_EPI_SWIGLU 2    // C[M][N/2] = swiglu over interleaved gate/up 16-column groups
#define LR_EPI_ROPE 3      // C = bf16(acc) with rotary embedding on the pair-interleaved q/k columns
#define LR_EPI_PARTIAL 4   // internal (split-K): fp32 partial sums to the workspace, real epilogue in the reduce pass
#define LR_EPI_GEGLU 5     // as LR_EPI_SWIGLU with the tanh-approximate GELU (Gemma)
#define LR_EPI_IS_GATED(e) ((e) == LR_EPI_SWIGLU || (e) == LR_EPI_GEGLU)
#define LR_SPLITK_WS_BYTES ((size_t)64 << 20)  // splits x tiles <= 256 tiles of 256 x 256 fp32

// packed-layout metadata (llama_elem.hip): prefix_len = P > 0 lays the batch out as [P shared prefix rows][rest of
// prompt 0]...[rest of prompt B-1]; seg_start (optional) receives the B + 1 (P = 0: B) + 1 segment starts, tok_src
// (optional) the index of every internal row in the caller's packed ids, last_rows (optional) each prompt's last row,
// last_pos (optional) the position of that token inside its prompt
int lr_launch_token_meta(const int32_t* cu, int B, int prefix_len, int32_t* seg_start, int32_t* tok_pos,
                         int32_t* tok_src, int32_t* last_rows, hipStream_t st, int32_t* last_pos = nullptr,
                         const int32_t* ids = nullptr /* with prefix_bad: verify the shared-prefix promise */,
                         int32_t* prefix_bad = nullptr /* device word: zeroed, then set if a prompt's first P ids differ */);
int lr_launch_gather_rows(const unsigned short* x, const int32_t* rows, int n_rows, int d, unsigned short* out,
                          hipStream_t st);
// scale / cap: as LrAttnArgs below (0 / 0 = head_dim^-0.5 and no soft cap: the kernel's path is then what it was)
// window: as LrAttnArgs below (0 = the plain causal range)
int lr_launch_attention_rows(const unsigned short* qkv, unsigned short* out, const int32_t* cu, int B,
                             const int32_t* q_rows, int n_rows, int nh, int nkv, int hd, hipStream_t st, float scale = 0.f,
                             float cap = 0.f, int window = 0);
int lr_launch_embed(const int32_t* ids, const int32_t* tok_src /*nullptr: identity*/, const unsigned short* table,
                    int vocab, int d, unsigned short* out, int n, hipStream_t st,
                    float scale = 1.0f /* != 1: rows bf16(e * scale) (Gemma's embedding scale) */);
// norm_style (here and below): 0 = Llama's RMSNorm, 1 = Gemma's (rms_apply)
int lr_launch_rmsnorm(const unsigned short* x, const unsigned short* w, unsigned short* out, int rows, int d,
                      float eps, const int32_t* row_map, hipStream_t st, int norm_style = 0);
int lr_launch_rope_table(float* cs, int T, int hd, float theta, hipStream_t st,
                         unsigned* cs16 = nullptr /* [T][hd/2] (cos | sin << 16) as bf16 pairs, optional */,
                         const LrRopeScaling* scaling = nullptr /* nullptr or kind 0: plain RoPE (the plain kernel) */);
// LR_OK, or LR_EINVAL with the reason recorded, for the words of an LrRopeScaling (nullptr is valid: plain RoPE)
int lr_check_rope_scaling(const LrRopeScaling* s, const char* who);
int lr_launch_head(const unsigned short* x, const int32_t* rows /*[B]; nullptr: x holds one row per prompt*/,
                   const unsigned short* norm_w,
                   const unsigned short* lm_head, const int32_t* class_ids, int B, int C, int d, float eps,
                   float* out, int vocab, hipStream_t st,
                   const int32_t* poison = nullptr /* device word: non-zero -> every score of the call is NaN */,
                   int norm_style = 0,
                   float final_softcap = 0.f /* > 0 (Gemma-2, norm_style 1): cap * tanh(logit / cap) at HF's bf16 steps */);
// Gemma-2's sandwich norm, one workgroup per row (llama_elem.hip): x <- bf16(x + bf16(gemmanorm(h, w_out))) in place and,
// with w_next, xn = bf16(gemmanorm(x, w_next)). xn may alias h (a workgroup reads its row of h before it writes any of xn).
int lr_launch_residual_postnorm(unsigned short* x, const unsigned short* h, const unsigned short* w_out,
                                const unsigned short* w_next, unsigned short* xn, int rows, int d, float eps, hipStream_t st);
// Qwen3's per-head RMSNorm of q and k followed by the rotary embedding, in place on a plain-stored (LR_EPI_STORE) QKV product
// (llama_elem.hip): buf [rows][ld] holds nq + nk heads of hd columns from column 0 on in the packed pair-interleaved order;
// columns behind them are not touched. q_norm / k_norm: bf16 [hd] in that order, 16-byte aligned; either group may be empty.
// hd: a power of two from 16 to 256 (lr_qk_norm_head_dim_ok), anything else LR_EUNSUPPORTED before any launch.
bool lr_qk_norm_head_dim_ok(int hd);
// norm_style 1 (Gemma-3): the norm is rms_apply<1>, bf16(x * rstd * (1 + w)) in fp32 with one rounding; the rotation is the same.
int lr_launch_qk_norm_rope(unsigned short* buf, int rows, int ld, int nq, int nk, int hd, const unsigned short* q_norm,
                           const unsigned short* k_norm, float eps, const int32_t* tok_pos, const float* rope_cs,
                           hipStream_t st, int norm_style = 0);

// C[M][N] (+epilogue) = A[M][K] * B[N][K]^T. Call sites name what they pass (designated initialisers); a member left
// out is absent. variant: 0 auto, 1 generic, 4 = 256x256x64 MFMA tile, 5 = variant 4 with split-K when the tiles alone
// would leave most CUs idle (needs splitk), 6 = auto, with the 256-tile body on a ragged last column tile where N % 64 == 0
// but N % 256 != 0 (llama_gemm.hip, lr_launch_gemm), 7 = variant 5 with the split fixed by the weight's shape (N, K) alone and
// the rows launched in chunks the split-K workspace holds: a row's arithmetic does not depend on the launch's row count (the
// online mode: ranker sessions; many serial launches at a large M). A width off the 256 tile is LR_EINVAL under 7.
struct LrGemmRope {                 // LR_EPI_ROPE only
  const int32_t* tok_pos = nullptr; // [M] position of each row inside its prompt
  const float* cs = nullptr;        // lr_launch_rope_table's fp32 table
  const unsigned* cs16 = nullptr;   // the same table as packed bf16 pairs (optional): lets the 256-tile kernel stage a tile's
                                    // (cos, sin) rows through LDS instead of 262 KB of half-line loads
  int head_dim = 0, rot_cols = 0;   // columns [0, rot_cols) are q and k heads
};
struct LrGemmSplitK { float* ws = nullptr; size_t bytes = 0; };  // fp32 partial planes for variant 5
// Residual epilogue only: the caller runs RMSNorm(C) with weight w into out next. If the product is split over K, its
// reduce pass does that too (same bits) and *done is set; otherwise *done is left false and the caller launches
// lr_launch_rmsnorm itself.
struct LrGemmThenNorm {
  const unsigned short* w = nullptr;
  unsigned short* out = nullptr;
  float eps = 0.f;
  int style = 0;
  bool* done = nullptr;
};
// Rope epilogue of a product that splits over K (variants 5 / 7) only, anything else is LR_EINVAL: the reduce pass stores
// columns < col0 to C as always and columns >= col0 (K rotated | V of a QKV product) to kv_layer + row_off[row] + (col - col0),
// the rows' places in a K / V cache (ranker sessions). col0 = 0: every column is scattered and C is not written.
struct LrGemmKvScatter {
  unsigned short* kv_layer = nullptr;   // the cache table at the layer's row offset (16-byte aligned); nullptr: absent
  const long long* row_off = nullptr;   // DEVICE [M] element offsets of the rows' cache rows, multiples of 4
  int col0 = 0;                         // a multiple of 4
};
struct LrGemmArgs {
  const unsigned short *A, *B;
  unsigned short* C;
  const unsigned short* R = nullptr;  // residual epilogue: the rows added (may alias C)
  int M, N, K;
  int epi = LR_EPI_STORE, variant = 0;
  LrGemmRope rope;
  const float* row_scale = nullptr;  // rope / swiglu epilogues: accumulator row m times row_scale[m] (folded RMSNorm)
  // store / rope epilogues: bf16 bias[N] by output column (8-byte aligned), x = bf16(acc + bias) in front of the rotation
  const unsigned short* bias = nullptr;
  LrGemmSplitK splitk;
  LrGemmThenNorm then_norm;
  LrGemmKvScatter kv_scatter;
};
int lr_launch_gemm(const LrGemmArgs& g, hipStream_t st);
// What lr_launch_gemm does with a variant-5 / 7 product (host only): *splits = the K splits (1 = not split), *rows_per_launch =
// the rows of one launch (variant 5 and unsplit products: M). LR_EWORKSPACE where lr_launch_gemm would return it.
int lr_gemm_splitk_plan_of(int variant, int M, int N, int K, size_t workspace_bytes, int* splits, int* rows_per_launch);
// split-K reduce (S fp32 planes of M x N) + residual + RMSNorm of the result in one pass (llama_elem.hip)
bool lr_reduce_residual_rmsnorm_fits(int N);
int lr_launch_reduce_residual_rmsnorm(const float* part, int S, unsigned short* C, const unsigned short* R, int M, int N,
                                      const unsigned short* norm_w, unsigned short* norm_out, float eps, hipStream_t st,
                                      int norm_style = 0);
// rstd[m] = 1 / sqrt(mean(x[m][:]^2) + eps), fp32 (the statistic of HF's LlamaRMSNorm)
int lr_launch_rms_rstd(const unsigned short* x, float* rstd, int rows, int d, float eps, hipStream_t st);
// out[j][k] = bf16(w[j][k] * norm_w[k]): an RMSNorm weight folded into the following projection's [out][in] matrix
int lr_launch_fold_norm(const unsigned short* w, const unsigned short* norm_w, unsigned short* out, size_t rows, int cols,
                        hipStream_t st);

// The segment rule of every attention entry point and prompt batch (include/llamarec_mi355x.h, cu_seqlens_host):
// cu_host[0] == 0 and cu_host strictly increasing -- every segment holds at least one row. The kernels derive work items,
// tile counts and buffer offsets from segment lengths, so an empty or negative segment must be refused here, before any
// launch. shortest / longest (optional) receive the extreme segment lengths.
static inline int lr_check_segments(const int32_t* cu_host, int S, const char* who, int* shortest = nullptr,
                                    int* longest = nullptr) {
  if (!cu_host || S < 1) LR_FAIL(LR_EINVAL, "%s: %d segments", who, S);
  if (cu_host[0] != 0) LR_FAIL(LR_EINVAL, "%s: cu_seqlens[0] = %d (must be 0)", who, cu_host[0]);
  int lo = 0x7fffffff, hi = 0;
  for (int b = 0; b < S; ++b) {
    const int t = cu_host[b + 1] - cu_host[b];
    if (t < 1) LR_FAIL(LR_EINVAL, "%s: segment %d is empty or negative (cu_seqlens %d -> %d)", who, b, cu_host[b], cu_host[b + 1]);
    lo = t < lo ? t : lo;
    hi = t > hi ? t : hi;
  }
  if (shortest) *shortest = lo;
  if (longest) *longest = hi;
  return LR_OK;
}

// Shared checks of the shared-prefix and last-row launchers at head_dim 64 / 256: segment 0 = the prefix with a prompt behind
// it, and the packed rows fit what one buffer descriptor addresses with 64 rows to spare (the per-lane offsets of the block
// that straddles the prefix's end reach up to 63 rows past the prompt's end and must not wrap back into range).
static inline int lr_check_prefix_layout(const char* who, const int32_t* cu_host, int S, int n_tok, int row_elems,
                                         int prefix_len) {
  if (prefix_len < 0 || (prefix_len > 0 && (S < 2 || cu_host[1] - cu_host[0] != prefix_len)))
    LR_FAIL(LR_EINVAL, "%s: segment 0 must be the %d-token shared prefix and a prompt must follow it", who, prefix_len);
  if (((long long)n_tok + 64) * row_elems * 2 > 0xffffffffLL)
    LR_FAIL(LR_EUNSUPPORTED, "%s: %d packed rows exceed the 4 GiB a buffer descriptor addresses", who, n_tok);
  return LR_OK;
}

// The launch plan of the tiled MFMA attention kernels (MFMA128, HD64, HD256 and the shared-prefix forms) from the host copy of
// the segment starts. prefix_len = P > 0: every segment but segment 0 continues the P keys of segment 0. A launcher hands
// `work` to its LrProfScope and then asks lr_attn_check_grid; which 4 GiB test applies is the launcher's own business.
struct LrAttnPlan {
  double work = 0;                  // causal QK^T + PV flops of the rows each segment owns
  int maxT = 0, mq = 0;             // longest sequence (prefix included) and the query tiles it needs
  long long n_pairs = 0, grid = 0;  // (segment, head or head group) pairs and workgroups; both fit an int once the grid is checked
};
// q_rows = query rows per tile; pairs_per_prompt = nh, or nh / 2 with two heads per workgroup. The grid is that of
// fa_tile_of_workgroup (lr_attn_util.h): a pair per dispatch stream, 8 * ceil(pairs / 8) * mq workgroups.
static inline LrAttnPlan lr_attn_plan(const int32_t* cu_host, int S, int prefix_len, int nh, int hd, int q_rows,
                                      int pairs_per_prompt) {
  LrAttnPlan p;
  for (int b = 0; b < S; ++b) {
    const double P = (prefix_len > 0 && b > 0) ? prefix_len : 0, T = P + cu_host[b + 1] - cu_host[b];
    p.work += 4.0 * nh * hd * (T * (T + 1) / 2 - P * (P + 1) / 2);
    p.maxT = p.maxT > (int)T ? p.maxT : (int)T;
  }
  p.mq = (p.maxT + q_rows - 1) / q_rows;
  p.n_pairs = (long long)S * pairs_per_prompt;
  p.grid = 8 * ((p.n_pairs + 7) / 8) * p.mq;
  return p;
}
// The last-row mode: one query row per prompt (segment 0 is no prompt when it is the prefix), one workgroup per (segment, head),
// the grid rounded up to a multiple of grid_multiple
static inline LrAttnPlan lr_attn_plan_last(const int32_t* cu_host, int S, int prefix_len, int nh, int hd, int grid_multiple) {
  LrAttnPlan p;
  for (int b = (prefix_len > 0 ? 1 : 0); b < S; ++b)
    p.work += 4.0 * nh * hd * (double)((prefix_len > 0 ? prefix_len : 0) + cu_host[b + 1] - cu_host[b]);
  p.n_pairs = (long long)S * nh;
  p.grid = grid_multiple * ((p.n_pairs + grid_multiple - 1) / grid_multiple);
  return p;
}
static inline int lr_attn_check_grid(const LrAttnPlan& p) {
  if (p.grid > 0x7fffffffLL) LR_FAIL(LR_EUNSUPPORTED, "attention: %lld workgroups exceed the grid limit", p.grid);
  return LR_OK;
}

// ---- varlen causal attention over packed qkv (RoPE applied) ----------------------------------------------------------------
// The kernels (a requested variant 1 .. 5 asks for the kernel of the same number, 6 for HD64 with lse allowed, 7 for HD96,
// 8 for HD96 with lse allowed, 9 for HD256 with lse allowed, 0 = auto):
//   GENERIC  any head_dim <= 256, scalar                                  (llama_attn.hip; its text: llama_attn_generic_body.h)
//   MFMA128  head_dim 128, 128-row query tiles, reads a shared prefix     (llama_attn.hip; one body, llama_attn_hd128_body.h,
//            shared with the cached kernels of llama_attn_cached.hip)
//   ROWS256  head_dim 128, 256-row query tiles over a device-built item list, shared prefix <= 64 (llama_attn256.hip)
//   HD256    head_dim 256; one body (llama_attn_hd256_body.h) instantiated without a shared prefix in llama_attn_hd256.hip,
//            with lse (variant 9, no prefix) in llama_attn_hd256_lse.hip, with a shared prefix in llama_attn_hd256_prefix.hip
//            and with soft-capped scores in llama_attn_hd256_softcap.hip; the sliding-window form (LrAttnArgs.window) is a body
//            of its own in llama_attn_hd256_window.hip
//   HD64     head_dim 64; one body (llama_attn_hd64_body.h) instantiated without a shared prefix in llama_attn_hd64.hip, with
//            lse (variant 6, no prefix) in llama_attn_hd64_lse.hip and with a shared prefix in llama_attn_hd64_prefix.hip
//   HD96     head_dim 96; one body (llama_attn_hd96_body.h) instantiated without a shared prefix in llama_attn_hd96.hip, with
//            lse (variant 8, no prefix) in llama_attn_hd96_lse.hip and with a shared prefix in llama_attn_hd96_prefix.hip
// MFMA128, HD256, HD64 and HD96 also have a one-query-row mode (lr_launch_attention_last, the pruned last layer): one more
// instantiation of the body, at HD256, HD64 and HD96 in the _prefix file. The four bodies hold what differs per head
// size; what they share is lr_attn_body.h on the device side and lr_attn_launch_tiles / _last (below) on the host side.
enum LrAttnKernel {
  LR_ATTN_GENERIC = 1, LR_ATTN_MFMA128 = 2, LR_ATTN_ROWS256 = 3, LR_ATTN_HD256 = 4, LR_ATTN_HD64 = 5, LR_ATTN_HD96 = 7
};

// Which kernel a request runs on -- the one place that decides it, for the five routes
//   prefill    run_body (api_llama.hip): lse never wanted, the handle's workspace always has room for an item list
//   varlen     lr_attention_varlen: no lse, no workspace
//   varlen_ws  lr_attention_varlen_ws: lse and workspace optional
//   train      lr_attention_varlen_lse: lse wanted, no workspace
//   lora       the LoRA forward (api_llama_train.hip): lse wanted, no workspace; its backward follows the same choice
//              (variant 0 at head_dim 64 -> lr_launch_attention_bwd variant 6, at head_dim 96 -> variant 8, at head_dim 256
//              -> variant 9)
// prefix_len is 0 outside prefill and lr_attention_varlen_prefix (which resolves as a prefill request without item workspace).
// Prefill drops a shared prefix (runs every prompt whole) unless lr_attention_reads_prefix: variant 1, a head_dim other than
// 64 / 96 / 128 / 256, variant 2 / 3 off head_dim 128 and the like -- and with a single prompt. First matching row:
//
//   variant  head_dim  prefix  lse  item ws  route        result
//   0        128       0       any  yes      varlen_ws    ROWS256
//   0        128       any     any  any      any          MFMA128  (prefill has the item workspace and still takes this one: on
//                                                                   its prompts of 460 .. 1 125 tokens two 128-row workgroups
//                                                                   per CU are ahead of the 256-row kernel)
//   0        256       any     no   any      prefill      HD256    (prefix > 0: its shared-prefix kernel)
//   0        64        any     no   any      prefill      HD64     (faster than GENERIC on every shape of DESIGN 10; prefix > 0:
//                                                                   its shared-prefix kernel)
//   0        96        any     no   any      prefill      HD96     (as at 64: 10 x GENERIC and more from 600 tokens, DESIGN 12;
//                                                                   prefix > 0: its shared-prefix kernel)
//   0        64, 96, 256  > 0  yes  any      any          LR_EINVAL  (no lse with a shared prefix off head_dim 128)
//   0        64        0       yes  no       lora         HD64     (with lse; the pair 6 / backward 6)
//   0        96        0       yes  no       lora         HD96     (with lse; the pair 8 / backward 8)
//   0        256       0       yes  no       lora         HD256    (with lse; the pair 9 / backward 9)
//   0        other     > 0     any  any      any          LR_EUNSUPPORTED  (GENERIC reads no shared prefix)
//   0        any       0       any  any      any          GENERIC  (head_dim 256, 96 and 64 too outside prefill and the LoRA
//                                                                   route: the entry points' auto is older than HD256 / HD64 /
//                                                                   HD96 and its results are kept, lr_attention_varlen_lse /
//                                                                   _bwd at head_dim 64, 96 and 256 included)
//   1        any       > 0     any  any      any          LR_EUNSUPPORTED
//   1        any       0       any  any      any          GENERIC
//   2        any       any     any  any      any          MFMA128
//   3        any       0       any  no       varlen, train  LR_EINVAL  (no item workspace exists on these routes)
//   3        != 128    any     any  yes      any          LR_EUNSUPPORTED
//   3        128       <= 64   any  yes      any          ROWS256
//   3        128       > 64    no   yes      prefill      MFMA128  (only a 256-row tile's block 0 may hold shared-prefix keys)
//   4        any       any     yes  any      any          LR_EINVAL  (variant 4 writes no statistics: 9 does)
//   4        != 256    any     no   yes      prefill      LR_EUNSUPPORTED
//   4        256       > 0     no   any      any          HD256    (its shared-prefix kernel)
//   4        any       0       no   any      any          HD256    (outside prefill a head_dim other than 256 is refused by
//                                                                   the launcher, LR_EUNSUPPORTED, behind its
//                                                                   num_heads % num_kv_heads check, LR_EINVAL, as before)
//   5        any       any     yes  any      any          LR_EINVAL  (HD64 writes no statistics)
//   5        != 64     any     no   any      any          LR_EUNSUPPORTED
//   5        64        any     no   any      any          HD64     (prefix > 0: its shared-prefix kernel)
//   6        != 64     any     any  any      any          LR_EUNSUPPORTED
//   6        64        > 0     yes  any      any          LR_EINVAL  (no lse with a shared prefix)
//   6        64        any     any  any      any          HD64     (writes lse when wanted; without lse variant 5's bits, with
//                                                                   a shared prefix too)
//   7        any       any     yes  any      any          LR_EINVAL  (variant 7 writes no statistics: 8 does)
//   7        != 96     any     no   any      any          LR_EUNSUPPORTED
//   7        96        any     no   any      any          HD96     (prefix > 0: its shared-prefix kernel)
//   8        != 96     any     any  any      any          LR_EUNSUPPORTED
//   8        96        > 0     yes  any      any          LR_EINVAL  (no lse with a shared prefix)
//   8        96        any     any  any      any          HD96     (writes lse when wanted; without lse variant 7's bits, with
//                                                                   a shared prefix too)
//   9        != 256    any     any  any      any          LR_EUNSUPPORTED
//   9        256       > 0     yes  any      any          LR_EINVAL  (no lse with a shared prefix)
//   9        256       any     any  any      any          HD256    (writes lse when wanted; without lse variant 4's bits, with
//                                                                   a shared prefix too)
//   other                                                 LR_EINVAL
//
// With a soft cap (LrAttnRequest.softcap: Gemma-2, lr_attention_varlen_softcap) the table is a short one. No lse anywhere
// (LR_EINVAL), and first matching row:
//
//   variant        head_dim  cap                     prefix  result
//   2, 3, 5, 6     any       any                     any     LR_EUNSUPPORTED  (those kernels have no capped form)
//   7, 8           96        any                     any     LR_EUNSUPPORTED  (nor has HD96; off head_dim 96 a capped variant 7
//                                                                     or 8 stays LR_EINVAL, the last row, as before HD96 existed)
//   9              256       any                     any     LR_EUNSUPPORTED  (the training pair has no capped form; off head_dim
//                                                                     256 a capped variant 9 stays LR_EINVAL, the last row)
//   0, 4           256       <= LR_SOFTCAP_MFMA_MAX  any     HD256    (the SOFTCAP instantiations of llama_attn_hd256_softcap.hip,
//                                                                     on every route)
//   0, 1, 4        any       any                     > 0     LR_EUNSUPPORTED  (GENERIC reads no shared prefix. The prefill never
//                                                                     gets here: plan_batch asks lr_attention_reads_prefix WITH the
//                                                                     cap, which answers true for the HD256 row above only, so a
//                                                                     capped handle at head_dim 64 / 128 runs every prompt whole)
//   0, 1, 4        any       any                     0       GENERIC  (slow but correct: gemma-2-27b's head_dim 128 lands here, and
//                                                                     so does a cap above LR_SOFTCAP_MFMA_MAX at head_dim 256)
//   other                                                    LR_EINVAL
//
// With a sliding window (LrAttnArgs.window > 0: Gemma-3, lr_attention_varlen_window) the kernel is resolved WITHOUT the window
// and lr_launch_attention / lr_launch_attention_last then take HD256's windowed kernels or GENERIC with the window; a resolved
// MFMA128, ROWS256, HD64 or HD96, a shared prefix, lse or a cap with a window is LR_EUNSUPPORTED there (the prefill sends a
// windowed layer of such a handle to GENERIC itself, api_llama.hip).
//
// LR_SOFTCAP_MFMA_MAX: the MFMA kernels evaluate the capped score as c2 - 2 c2 rcp(1 + exp2(a s)) with c2 = cap log2(e), whose
// absolute error is about two ulps of 1 times c2 (1.7e-7 cap in the exp2 domain, at small a s as well: there 1 + exp2(a s)
// rounds a s to an ulp of 2). At cap 256 that is 4e-5, a hundredth of a bf16 step of P; the generic kernel's tanhf keeps a
// RELATIVE error whatever the cap, so larger caps (where the cap hardly acts) go there. Gemma-2 uses 50.
#define LR_SOFTCAP_MFMA_MAX 256.0f
// varlen_ws counts a variant-3 request as "item ws yes" whatever it was given: the item-list builder then reports a missing
// or short workspace as LR_EWORKSPACE. lr_launch_attention still refuses what the resolved kernel cannot take: GENERIC above
// head_dim 256 and MFMA128 off head_dim 128 (LR_EUNSUPPORTED; a one-layer pruned prefill launches neither, so these checks
// cannot move up here), lse with a shared prefix on HD64, HD96 and HD256, lse with a soft cap, a segment 0 that is not the
// prefix.
// cap > 0 (soft-capped scores): only HD256's capped instantiations read a shared prefix (the short table above)
static inline bool lr_attention_reads_prefix(int variant, int hd, float cap = 0.f) {
  if (cap > 0.f) return hd == 256 && (variant == 0 || variant == 4) && cap <= LR_SOFTCAP_MFMA_MAX;
  if (hd == 128) return variant != 1;
  if (hd == 64) return variant == 0 || variant == 5 || variant == 6;
  if (hd == 96) return variant == 0 || variant == 7 || variant == 8;
  if (hd == 256) return variant == 0 || variant == 4 || variant == 9;
  return false;
}
// The resolved kernel has a one-query-row (LASTQ) mode behind lr_launch_attention_last
static inline bool lr_attention_has_last_row_mode(int kernel, int hd) {
  return (hd == 128 && kernel != 1 /* LR_ATTN_GENERIC */) || kernel == 4 /* LR_ATTN_HD256 */ || kernel == 5 /* LR_ATTN_HD64 */ ||
         kernel == 7 /* LR_ATTN_HD96 */;
}
struct LrAttnRequest {
  int variant, hd, prefix_len = 0;
  bool want_lse = false, have_items_ws = false, prefill = false, lora = false;
  float cap = 0.f;        // > 0: the scores are soft-capped (LrAttnArgs.cap): the short table
};
int lr_resolve_attention(const LrAttnRequest& r, LrAttnKernel* kernel);

// cu / cu_host = segment starts [S + 1] in packed rows; prefix_len = P > 0: segment 0 is the shared prefix (P rows) the
// other segments continue. lse (optional) = [n_tok][nh] log-sum-exp output; items_ws = lr_launch_attn256_items' output for
// the same (cu, S, nh, prefix_len), read by ROWS256 only.
struct LrAttnArgs {
  const unsigned short* qkv;
  unsigned short* out;
  float* lse = nullptr;
  const int32_t *cu, *cu_host;
  int S, n_tok, nh, nkv, hd, prefix_len = 0;
  void* items_ws = nullptr;
  // cap > 0: scores cap * tanh(q.k * scale / cap) (HD256's SOFTCAP instantiations and GENERIC only), scale > 0 then required
  // by HD256; GENERIC takes scale = 0 as head_dim^-0.5. Both 0: the kernels' own head_dim^-0.5 and no cap.
  float scale = 0.f, cap = 0.f;
  // window = W > 0 (Gemma-3's sliding layers): query i sees keys i - W < j <= i. HD256 (its windowed kernels,
  // llama_attn_hd256_window.hip) and GENERIC only, without a shared prefix, lse or cap. 0: the plain causal range.
  int window = 0;
};
int lr_launch_attention(const LrAttnArgs& a, LrAttnKernel kernel, hipStream_t st);
// The pruned last layer (MFMA128's, HD64's, HD96's or HD256's last-row kernel by head_dim): one query row per (prompt, head) over the prompt's keys
int lr_launch_attention_last(const unsigned short* kv, const unsigned short* q_last, unsigned short* out_last,
                             const int32_t* cu, const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int hd,
                             hipStream_t st, int prefix_len, float scale = 0.f, float cap = 0.f /* > 0: head_dim 256 only */,
                             int window = 0 /* > 0: head_dim 256 only, no prefix, no cap */);
// ROWS256's item list for (cu, S, nh, prefix_len) into items_ws (lr_attn256_ws_bytes), built once per call; any number of
// lr_launch_attention calls over the same segments may follow (one per layer)
size_t lr_attn256_ws_bytes(int n_tok, int S, int nh);
int lr_launch_attn256_items(const int32_t* cu, int S, int n_tok, int nh, int prefix_len, void* items_ws, size_t ws_bytes,
                            hipStream_t st);
// the per-file launchers behind lr_launch_attention
int lr_launch_attention256(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd256(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd256_lse(const LrAttnArgs& a, hipStream_t st);   // a.lse != nullptr: lr_launch_attention_hd256 sends it here
int lr_launch_attention_hd64(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd64_lse(const LrAttnArgs& a, hipStream_t st);   // a.lse != nullptr: lr_launch_attention_hd64 sends it here
// HD64 / HD256 with a.prefix_len > 0 (llama_attn_hd64_prefix.hip, llama_attn_hd256_prefix.hip) and their last-row modes
int lr_launch_attention_hd64_prefix(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd256_prefix(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd64_last(const unsigned short* kv, const unsigned short* q_last, unsigned short* out_last,
                                  const int32_t* cu, const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int prefix_len,
                                  hipStream_t st);
int lr_launch_attention_hd256_last(const unsigned short* kv, const unsigned short* q_last, unsigned short* out_last,
                                   const int32_t* cu, const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int prefix_len,
                                   hipStream_t st);
// HD96 (llama_attn_hd96.hip), with a.prefix_len > 0 and its last-row mode (llama_attn_hd96_prefix.hip)
int lr_launch_attention_hd96(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd96_lse(const LrAttnArgs& a, hipStream_t st);   // a.lse != nullptr: lr_launch_attention_hd96 sends it here
int lr_launch_attention_hd96_prefix(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd96_last(const unsigned short* kv, const unsigned short* q_last, unsigned short* out_last,
                                  const int32_t* cu, const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int prefix_len,
                                  hipStream_t st);
// HD256 with soft-capped scores (llama_attn_hd256_softcap.hip): whole prompts or a shared prefix by a.prefix_len, and the
// last-row mode
int lr_launch_attention_hd256_softcap(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd256_softcap_last(const unsigned short* kv, const unsigned short* q_last, unsigned short* out_last,
                                           const int32_t* cu, const int32_t* cu_host, int S, int n_tok, int nh, int nkv,
                                           int prefix_len, float scale, float cap, hipStream_t st);
// HD256 with a sliding window (llama_attn_hd256_window.hip): whole prompts (a.window >= 1, no shared prefix) and the last-row mode
int lr_launch_attention_hd256_window(const LrAttnArgs& a, hipStream_t st);
int lr_launch_attention_hd256_window_last(const unsigned short* kv, const unsigned short* q_last, unsigned short* out_last,
                                          const int32_t* cu, const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int window,
                                          hipStream_t st);

// ---- the launch sequence of the MFMA128 / HD64 / HD96 / HD256 kernels, once --------------------------------------------------
// Every lr_launch_attention_hd* above, and MFMA128's two launches in llama_attn.hip, is one call of lr_attn_launch_tiles or
// lr_attn_launch_last with its kernel (a template
// argument: the dynamic-LDS flag is per kernel), head_dim, threads and dynamic LDS bytes per workgroup. The kernels' argument
// lists are (qkv, out, cu, [prefix_len,] nh, nkv, max_qblocks, n_pairs, tail...): `tail` is passed through.
template <auto KERNEL, int BLOCK, int LDS_BYTES, class... Args>
static inline int lr_attn_launch_kernel(const LrAttnPlan& pl, const char* kernel_name, hipStream_t st, Args... args) {
  static bool lds_set[LR_MAX_DEVICES] = {};
  LR_RUN(lr_ensure_dynamic_lds(reinterpret_cast<const void*>(KERNEL), LDS_BYTES, lds_set));
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)pl.grid), dim3(BLOCK), LDS_BYTES, st, args...);
  LR_CHECK_LAUNCH(kernel_name);
  return LR_OK;
}
// Whole query tiles of QROWS rows, HPW heads per workgroup. needs = "<who> needs head_dim <HD>" for the head_dim refusal;
// no_lse = the refusal of a.lse (nullptr: the kernel writes it, or the caller has dealt with it); extra = a check of the
// caller's own behind those (the soft cap's). PREFIX_ARG: the kernel takes a.prefix_len and reads a shared prefix. layout = the
// name lr_check_prefix_layout reports under; nullptr: that check is not made (whole prompts, or MFMA128, whose caller has made
// its own) and the packed rows must fit one buffer descriptor. No rows, no launch.
template <auto KERNEL, int HD, int QROWS, int BLOCK, int LDS_BYTES, bool PREFIX_ARG, int HPW = 1, class... Tail>
static inline int lr_attn_launch_tiles(const char* kernel_name, const char* needs, const char* no_lse,
                                       int (*extra)(const LrAttnArgs&), const char* layout, const LrAttnArgs& a, hipStream_t st,
                                       Tail... tail) {
  const int S = a.S, n_tok = a.n_tok, nh = a.nh, nkv = a.nkv, hd = a.hd, P = a.prefix_len;
  if (n_tok <= 0 || S <= 0) return LR_OK;
  if (hd != HD) LR_FAIL(LR_EUNSUPPORTED, "%s (got %d)", needs, hd);
  if (nh < 1 || nkv < 1 || nh % nkv != 0)
    LR_FAIL(LR_EINVAL, "attention: num_heads %d not a multiple of num_kv_heads %d", nh, nkv);
  if (no_lse && a.lse) LR_FAIL(LR_EINVAL, "%s", no_lse);
  if (extra) LR_RUN(extra(a));
  if (layout) LR_RUN(lr_check_prefix_layout(layout, a.cu_host, S, n_tok, (nh + 2 * nkv) * hd, P));
  const LrAttnPlan pl = lr_attn_plan(a.cu_host, S, PREFIX_ARG ? P : 0, nh, hd, QROWS / HPW, nh / HPW);
  LrProfScope prof(LR_PROF_ATTN_MFMA, pl.work, st);
  if (HPW == 2 && (nh / nkv) % 2 != 0) LR_FAIL(LR_EINVAL, "attention: two heads per workgroup need an even nh / nkv");
  if (pl.mq == 0) return LR_OK;
  LR_RUN(lr_attn_check_grid(pl));
  if (!layout && (long long)n_tok * (nh + 2 * nkv) * hd * 2 > 0x7fffffffLL * 2)
    LR_FAIL(LR_EUNSUPPORTED, "attention: packed qkv of %d tokens exceeds the 4 GiB a buffer descriptor addresses", n_tok);
  if constexpr (PREFIX_ARG)
    return lr_attn_launch_kernel<KERNEL, BLOCK, LDS_BYTES>(pl, kernel_name, st, a.qkv, a.out, a.cu, P, nh, nkv, pl.mq,
                                                            (int)pl.n_pairs, tail...);
  else
    return lr_attn_launch_kernel<KERNEL, BLOCK, LDS_BYTES>(pl, kernel_name, st, a.qkv, a.out, a.cu, nh, nkv, pl.mq,
                                                            (int)pl.n_pairs, tail...);
}
// The pruned last layer (lr_launch_attention_last): kv = [n_tok][2 nkv hd], q_last / out_last = [prompts][nh hd], one workgroup
// per (segment, head), the grid rounded up to a multiple of GRID_MULTIPLE. layout as above.
template <auto KERNEL, int HD, int BLOCK, int LDS_BYTES, int GRID_MULTIPLE = 1, class... Tail>
static inline int lr_attn_launch_last(const char* kernel_name, const char* layout, const unsigned short* kv,
                                      const unsigned short* q_last, unsigned short* out_last, const int32_t* cu,
                                      const int32_t* cu_host, int S, int n_tok, int nh, int nkv, int prefix_len, hipStream_t st,
                                      Tail... tail) {
  if (layout) LR_RUN(lr_check_prefix_layout(layout, cu_host, S, n_tok, 2 * nkv * HD, prefix_len));
  const LrAttnPlan pl = lr_attn_plan_last(cu_host, S, prefix_len, nh, HD, GRID_MULTIPLE);
  LrProfScope prof(LR_PROF_ATTN_MFMA, pl.work, st);
  LR_RUN(lr_attn_check_grid(pl));
  return lr_attn_launch_kernel<KERNEL, BLOCK, LDS_BYTES>(pl, kernel_name, st, kv, out_last, cu, prefix_len, nh, nkv, 0,
                                                          (int)pl.n_pairs, q_last, tail...);
}

// ---- attention over a per-user K / V cache (llama_attn_cached.hip; ranker sessions) -------------------------------
// A slot of the caller's table is [num_layers][max_tokens] rows of [K rotated | V] (2 nkv hd bf16), a row per prompt position.
// Prompt b of a call owns the packed rows cu[b] .. cu[b + 1] - 1, which sit at positions
// cached_len[b] .. of slot slots[b].
// tok_pos[r] = the position of packed row r, last_rows[b] / last_pos[b] = prompt b's last packed row and its position
// row_off (optional, with slots): [n] element offsets slots[b] * slot_elems + position * kv_w of the rows' cache rows in a layer
int lr_launch_kv_cache_meta(const int32_t* cu, const int32_t* cached_len, int B, int n, int32_t* tok_pos, int32_t* last_rows,
                            int32_t* last_pos, hipStream_t st, const int32_t* slots = nullptr, long long slot_elems = 0,
                            int kv_w = 0, long long* row_off = nullptr);
// columns [col0, col0 + kv_w) of src [n][ld] -> the rows' slot rows in dst (the table at the layer's row offset)
int lr_launch_kv_cache_write(const unsigned short* src, int ld, int col0, int kv_w, const int32_t* cu, const int32_t* cached_len,
                             const int32_t* slots, int B, long long slot_elems, unsigned short* dst, int n, hipStream_t st);
// Query row i of prompt b (position cached_len[b] + i) over keys 0 .. cached_len[b] + i of the slot, whose rows up to the
// prompt's last position are written. q [rows][q_ld] with head h at column h * hd; out [rows][nh hd]. kv = the table at the
// layer's row offset, slot_elems = elements from one slot to the next.
//   last     : one query row per prompt, the one at its last position. The MFMA kernel then reads q as one compact row per
//              prompt ([B][q_ld]); the generic kernel reads the packed rows q_rows[b] (= last_rows). out is [B][nh hd].
//   generic  : the scalar kernel (any head_dim <= 256); otherwise the head_dim-128 MFMA kernel
struct LrAttnCachedArgs {
  const unsigned short* q;
  int q_ld;
  unsigned short* out;
  const unsigned short* kv;
  long long slot_elems;
  const int32_t *slots, *cached_len, *cu;       // DEVICE [B], [B], [B + 1]
  const int32_t *cached_len_host, *cu_host;     // the same values on the host (launch geometry)
  int B, nh, nkv, hd;
  bool last = false, generic = false;
  const int32_t* q_rows = nullptr;
};
int lr_launch_attention_cached(const LrAttnCachedArgs& a, hipStream_t st);

#endif
