// llama_train.h -- internal launcher declarations of the ranker's LoRA training step (llama_train.hip,
// llama_attn_bwd.hip, api_llama_train.hip).
#ifndef LLAMA_TRAIN_H
#define LLAMA_TRAIN_H

#include "llama_kernels.h"

#define LT_RP 16  // LoRA rank padded to one MFMA column tile per projection (r <= 16)

int lr_launch_transpose_bf16(const unsigned short* src, int rows, int cols, unsigned short* dst, hipStream_t st);
int lr_launch_prep_lora(const float* aq, const float* bq, const float* av, const float* bv, int r, int d, int qcols,
                        int vcols, int hd, unsigned short* a_cat, unsigned short* bq_t, unsigned short* bv_t,
                        hipStream_t st);
int lr_launch_skinny(const unsigned short* X, int ldx, int n, int K, const unsigned short* W, int nt, unsigned short* out,
                     int ldo, int ocol, float scale, uint32_t drop_stream, float drop_p, hipStream_t st);
// Qwen3's q / k norms in the LoRA forward sweep: bf16 [hd] weights in a head's packed column order, and xsave
// [n][qcols + kcols], which receives the pre-norm q | k values (delta included) for lr_launch_qk_norm_bwd. q_norm null: no norm.
struct LrQkNormFwd {
  const unsigned short *q_norm = nullptr, *k_norm = nullptr;
  float eps = 0.f;
  unsigned short* xsave = nullptr;
};
int lr_launch_lora_rope_fwd(unsigned short* qkv, int n, int qw, int qcols, int kcols, int hd, const unsigned short* t,
                            const unsigned short* bq_t, const unsigned short* bv_t, int r, float scaling,
                            const int32_t* tok_pos, const float* rope_cs, hipStream_t st,
                            const unsigned short* tk = nullptr, int ldtk = 0, int tkcol = 0,
                            const unsigned short* bk_t = nullptr,  // bk_t: k_proj's adapter, t from tk [n][ldtk] column tkcol
                            const LrQkNormFwd& qkn = {});  // the norm between "add the delta" and "rotate"
// backward of the q / k norms, in place on the q and k columns of dqkv [rows][ld] (nq + nk heads from column 0 on): the
// gradient w.r.t. the normed unrotated q / k becomes the gradient w.r.t. the pre-norm values x [rows][ldx] (the forward's
// xsave). The norm weights are frozen: no weight gradient. One owner per element, no atomics.
int lr_launch_qk_norm_bwd(unsigned short* dqk, int rows, int ld, const unsigned short* x, int ldx, int nq, int nk, int hd,
                          const unsigned short* q_norm, const unsigned short* k_norm, float eps, hipStream_t st);
int lr_launch_rope_bwd(unsigned short* dqkv, int n, int qw, int rot_cols, int hd, const int32_t* tok_pos,
                       const float* rope_cs, hipStream_t st);
int lr_launch_lora_db(const unsigned short* dqkv, int n, int qw, int qcols, int kcols, int hd, const unsigned short* t,
                      int r, float scaling, float* dbq, float* dbv, hipStream_t st, float* det_part = nullptr);
int lr_launch_lora_da(const unsigned short* xn, int n, int d, const unsigned short* dt, int r, uint32_t drop_stream,
                      float drop_p, float* daq, float* dav, hipStream_t st, float* det_part = nullptr);
// adapters on any Linear: launch_tn exposed (layouts: llama_train.hip), one module's working copies, the expand-add sweep.
// det_part (here and in _db / _da above) != nullptr selects the deterministic form of the token reductions: per-chunk partial
// tiles stored there (lr_lora_tn_partial_floats floats, the largest any batch of at most n tokens needs) and folded in chunk
// order. Launches that may run at the same time need separate partials.
size_t lr_lora_tn_partial_floats(int nj, int n, int cols, int r, int layout);
int lr_launch_lora_tn(int nj, const unsigned short* T, int ldt, int tcol, const unsigned short* X, int ldx, int n, int cols,
                      float scale, float* out0, float* out1, int r, int layout, int hd, uint32_t drop_stream, float drop_p,
                      hipStream_t st, float* det_part = nullptr);
int lr_launch_prep_module(const float* a, const float* b, int r, int in, int out, int perm, int hd, unsigned short* a_w,
                          unsigned short* b_t, int ldb, hipStream_t st);
int lr_launch_lora_expand(unsigned short* Y, int ldy, int n, int cols, const unsigned short* T, int ldt, int tcol,
                          const unsigned short* W, int r, float s, uint32_t drop_stream, float drop_p, hipStream_t st);
int lr_launch_swiglu_fwd(const unsigned short* gu, unsigned short* h, int n, int f, hipStream_t st);
int lr_launch_swiglu_lora_fwd(unsigned short* gu, unsigned short* h, int n, int f, const unsigned short* t, int ldt, int tcol,
                              const unsigned short* W, int r, float s, hipStream_t st);
int lr_launch_swiglu_bwd(unsigned short* gu, const unsigned short* dh, int n, int f, hipStream_t st);
int lr_launch_rmsnorm_bwd(const unsigned short* dy, const unsigned short* x, const unsigned short* w,
                          const unsigned short* res, unsigned short* out, int rows, int d, float eps,
                          const int32_t* out_rows, const unsigned short* dt, const unsigned short* a_cat, int r,
                          uint32_t drop_stream, float drop_p, hipStream_t st, int ldt = 2 * LT_RP);  // ldt: row stride of dt
// deterministic: scal is [2 + m] floats (1: rows without a token id, 2 + i: row i's loss) and the sum is taken in row order
int lr_launch_ce_bf16(unsigned short* logits, int m, int V, const int32_t* targets, float gscale, float* scal,
                      hipStream_t st, bool deterministic = false);
int lr_launch_finish_loss(const float* scal, int m, float* out, hipStream_t st, bool deterministic = false);
int lr_launch_rowdot(const unsigned short* o, const unsigned short* d_o, int n, int nh, int hd, float* out,
                     hipStream_t st);
int lr_launch_lora_adamw(float* p, float* g, float* m, float* v, size_t n, float* scratch, int* ctr, float lr,
                         float max_grad_norm, float beta1, float beta2, float eps, float wd, float* out_norm,
                         hipStream_t st, bool deterministic = false);  // deterministic: the norm summed in a fixed order
uint32_t lr_lora_drop_stream(uint64_t seed, uint32_t pass, uint32_t layer);

// backward of lr_launch_attention with the softmax statistics kept (lse[n][nh], natural log; llama_attn_bwd.hip).
// dqkv [n][(nh+2nkv)*hd], fully written: the gradient w.r.t. the rotated q, k and v -- or, when rope_cs / tok_pos are
// given, w.r.t. the UNROTATED ones (the inverse rotation is pair-local in the packed layout and rides in the MFMA
// passes' epilogues). dsum: [n][nh] fp32 scratch, dkv32: [n][2*nkv*hd] fp32 scratch (generic path only).
// deterministic: the generic path computes dK / dV per owner instead of adding them atomically (dkv32 unused); the head_dim-128
// passes have no atomics either way, nor have variant 6's head_dim-64, variant 8's head_dim-96 and variant 9's head_dim-256
// passes.
// variant: 0 / 3 = auto (2 at head_dim 128, else 1), 1 generic, 2 = head_dim-128 MFMA passes, 6 = head_dim-64 MFMA passes
// (LR_EUNSUPPORTED off head_dim 64), 8 = head_dim-96 MFMA passes (LR_EUNSUPPORTED off head_dim 96), 9 = head_dim-256 MFMA
// passes (LR_EUNSUPPORTED off head_dim 256); 4, 5 and 7 are forward-only kernels: LR_EINVAL.
int lr_launch_attention_bwd(const unsigned short* qkv, const unsigned short* out, const unsigned short* d_out,
                            const float* lse, unsigned short* dqkv, float* dsum, float* dkv32, const int32_t* cu,
                            const int32_t* cu_host, int B, int n_tok, int nh, int nkv, int hd, int variant,
                            hipStream_t st, const int32_t* tok_pos = nullptr, const float* rope_cs = nullptr,
                            bool deterministic = false);
// Variants 6, 8 and 9 are one text of the two passes (lr_attn_bwd_body.h, lr_attn_bwd_dq_body.h, lr_attn_bwd_dkv_body.h) and
// one launcher (lr_attn_bwd_launch); a unit holds its head size's geometry, the two kernels and the launcher's one call.
// variant 6's two passes (llama_attn_bwd_hd64.hip): head_dim 64 only, dsum = rowsum(dO .* O) already computed; one owner per
// element of dqkv, no atomics, no dkv32
int lr_launch_attention_bwd_hd64(const unsigned short* qkv, const unsigned short* d_out, const float* lse, const float* dsum,
                                 unsigned short* dqkv, const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh,
                                 int nkv, int hd, hipStream_t st, const float* rope_cs);
// variant 8's two passes (llama_attn_bwd_hd96.hip): the same at head_dim 96
int lr_launch_attention_bwd_hd96(const unsigned short* qkv, const unsigned short* d_out, const float* lse, const float* dsum,
                                 unsigned short* dqkv, const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh,
                                 int nkv, int hd, hipStream_t st, const float* rope_cs);
// variant 9's two passes (llama_attn_bwd_hd256.hip): the same at head_dim 256
int lr_launch_attention_bwd_hd256(const unsigned short* qkv, const unsigned short* d_out, const float* lse, const float* dsum,
                                  unsigned short* dqkv, const int32_t* cu, const int32_t* cu_host, int B, int n_tok, int nh,
                                  int nkv, int hd, hipStream_t st, const float* rope_cs);

#endif
