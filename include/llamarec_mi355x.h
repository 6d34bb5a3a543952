/* llamarec_mi355x.h -- C ABI of libllamarec_mi355x.so (MI355X / gfx950).
 *
 * Drop-in boundary for the two-stage retrieve-then-rerank scoring path of GarciaLnk/LlamaRec.
 * The reference has no FFI: its seams are Python nn.Module.forward calls. Each entry point below
 * names the reference call site it replaces (paths are into the reference tree).
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / C++ types cross the boundary.
 *  - the CALLER owns every buffer (weights, workspaces, inputs, outputs; normally torch tensors);
 *    the library owns nothing but small host-side handles. No entry point allocates device
 *    memory or synchronises the device, so every call is hipGraph-capturable.
 *  - all device work is enqueued on the caller's hipStream_t (passed as void*); the caller
 *    synchronises.
 *  - return value: 0 = LR_OK, negative = LR_E*; lr_last_error() gives a thread-local message.
 *  - re-entrant across handles; one in-flight call per handle+workspace.
 */
#ifndef LLAMAREC_MI355X_H
#define LLAMAREC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LR_OK 0
#define LR_EINVAL (-1)   /* bad argument (null pointer, shape out of range) */
#define LR_EUNSUPPORTED (-2) /* configuration outside what the kernels implement */
#define LR_EHIP (-3)     /* HIP runtime error (launch failure, wrong device, ...) */
#define LR_EWORKSPACE (-4) /* caller-provided workspace too small */

#define LR_MAX_LRU_BLOCKS 4
#define LR_MAX_TOPK 64

const char* lr_last_error(void);
/* "llamarec_mi355x <semver> gfx950" */
const char* lr_version(void);

/* ------------------------------------------------------------------------------------------
 * Stage 1: LRURec retriever  (model/lru.py:8-175, trainer/lru.py:30-42,44-138)
 * ------------------------------------------------------------------------------------------ */

/* One LRUBlock's tensors exactly as in the reference state_dict (model/lru.py:89-175);
 * complex64 tensors are passed as interleaved (re,im) float pairs (torch.view_as_real). */
typedef struct LrLruBlockWeights {
  const float* params_log;  /* [3][128]      lru_layer.params_log (nu_log, theta_log, gamma_log) */
  const float* in_proj_w;   /* [128][64][2]  lru_layer.in_proj.weight  (complex64) */
  const float* in_proj_b;   /* [128][2]      lru_layer.in_proj.bias    (complex64) */
  const float* out_proj_w;  /* [64][128][2]  lru_layer.out_proj.weight (complex64) */
  const float* out_proj_b;  /* [64][2]       lru_layer.out_proj.bias   (complex64) */
  const float* ln1_w;       /* [64]          lru_layer.layer_norm.weight */
  const float* ln1_b;       /* [64]          lru_layer.layer_norm.bias */
  const float* ffn_w1;      /* [256][64]     feed_forward.w_1.weight */
  const float* ffn_b1;      /* [256]         feed_forward.w_1.bias */
  const float* ffn_w2;      /* [64][256]     feed_forward.w_2.weight */
  const float* ffn_b2;      /* [64]          feed_forward.w_2.bias */
  const float* ln2_w;       /* [64]          feed_forward.layer_norm.weight */
  const float* ln2_b;       /* [64]          feed_forward.layer_norm.bias */
} LrLruBlockWeights;

/* LRURec state_dict (SURVEY.md 8(a) a-W). All pointers are HOST pointers, fp32. */
typedef struct LrLruWeightsDesc {
  int32_t num_items;        /* V; the item table has V+1 rows (row 0 = pad id, a learned row) */
  int32_t hidden;           /* bert_hidden_units; must be 64 */
  int32_t num_blocks;       /* bert_num_blocks; 1..LR_MAX_LRU_BLOCKS */
  int32_t reserved;
  const float* item_emb;    /* [V+1][64]  embedding.token.weight (tied output table) */
  const float* item_bias;   /* [V+1]      model.bias */
  const float* emb_ln_w;    /* [64]       embedding.layer_norm.weight */
  const float* emb_ln_b;    /* [64]       embedding.layer_norm.bias */
  LrLruBlockWeights blocks[LR_MAX_LRU_BLOCKS];
} LrLruWeightsDesc;

typedef struct lr_lru lr_lru_t;

/* Bytes of the packed device image for a model with num_items = V, num_blocks blocks. */
size_t lr_lru_packed_bytes(int32_t num_items, int32_t num_blocks);

/* Host-side packer: state_dict layout -> the kernels' device layout (transposed projection
 * matrices, split re/im, recurrence coefficients lambda/gamma derived once). Pure CPU; writes
 * lr_lru_packed_bytes() bytes to host_out. The caller then copies the image to the GPU. */
int lr_lru_pack(const LrLruWeightsDesc* desc, void* host_out, size_t host_out_bytes);

/* Bind a handle to a packed image resident in DEVICE memory (kept alive by the caller).
 * Replaces LRURec.__init__ + load_state_dict (model/lru.py:8-14, trainer/base.py:158-161). */
int lr_lru_create(const void* packed_dev, size_t packed_bytes, int32_t num_items, int32_t num_blocks,
                  lr_lru_t** out);
void lr_lru_destroy(lr_lru_t* h);

/* Diagnostic switch: 1 (default) runs the encoder's LRU layer on the software-pipelined kernel (two 64-row tiles in
 * flight, role-split waves), 0 on the one-tile-at-a-time kernel. Both produce the same bits (tests/test_gpu_lru.py
 * compares them); the switch exists for that test and for A/B timing. No counterpart in the reference. */
int lr_lru_set_encoder_pipeline(lr_lru_t* h, int32_t enable);

/* Workspace (device) bytes needed by lr_lru_retrieve_topk / lr_lru_scores_last for up to
 * max_users histories of up to max_len ids per call (q rows, per-chunk partial top-K lists,
 * sorted history ids for the mask, the bound pre-pass's scratch for catalogs it serves). h must be a live handle
 * (the size depends on the catalog; NULL returns 0 and sets lr_last_error). The size is monotone in every argument:
 * a workspace sized for (max_users, max_k, max_len) serves every call with B <= max_users, K <= max_k, L <= max_len. */
size_t lr_lru_workspace_bytes(const lr_lru_t* h, int32_t max_users, int32_t max_k, int32_t max_len);

/* Encode B histories and return the hidden state of the LAST position, q[B][64] (fp32).
 * Replaces LRURec.forward up to (not including) the item GEMM, last position only
 * (model/lru.py:38-41,57-60,73-83; consumers slice [:, -1, :]: trainer/lru.py:33,67,105,
 * demo/inference.py:48).
 *   ids: DEVICE int64 [B][L] row-major, 0 = pad (left padded by the reference's datasets,
 *        dataloader/lru.py:142-151; zeros anywhere are honoured: mask = ids > 0).
 *   workspace: with at least lr_lru_workspace_bytes(h, B, 1, L) bytes the batched MFMA encoder runs (live
 *        tokens of all users packed into one row matrix); with less (or NULL) a one-workgroup-per-user
 *        kernel that needs no scratch -- same bits either way. */
int lr_lru_encode_last(lr_lru_t* h, const int64_t* ids, int32_t B, int32_t L, float* out_q,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* Fused retrieve: encode -> item GEMM on the last position -> optional history/pad mask
 * (-1e9, trainer/lru.py:35-38,72-74,110-112) -> ordered top-K.
 * Replaces `model(seqs)[:, -1, :]` + masking loop + torch.topk / argsort
 * (trainer/lru.py:33-38,67-84,105-126).
 *   out_idx  : DEVICE int32 [B][K], score descending, ties -> lower item id first
 *   out_score: DEVICE fp32  [B][K] (may be NULL)
 *   K <= LR_MAX_TOPK. The [B][V+1] score matrix is never written to memory. */
int lr_lru_retrieve_topk(lr_lru_t* h, const int64_t* ids, int32_t B, int32_t L, int32_t K,
                         int32_t exclude_history, int32_t* out_idx, float* out_score,
                         void* workspace, size_t workspace_bytes, void* hip_stream);

/* Diagnostic: which path the LAST lr_lru_retrieve_topk call with exactly these (B, L, K, exclude_history) on this
 * workspace took -- *out_path = 0: the exact f32 pass over every item (catalogs and history lengths the bound does not
 * serve), 1: bf16 bound -> candidates -> exact rescoring, 2: that path overflowed a candidate list and the exact pass
 * redid the call (results are correct either way; 2 is a performance cliff the tests watch for). Synchronises the
 * stream. No counterpart in the reference (it materialises every score, model/lru.py:85). */
int lr_lru_topk_path(const lr_lru_t* h, int32_t B, int32_t L, int32_t K, int32_t exclude_history,
                     const void* workspace, size_t workspace_bytes, int32_t* out_path, void* hip_stream);

/* Compatibility path: materialise last-position scores [B][V+1] (fp32), optionally masked.
 * Replaces `self.model(seqs)[:, -1, :]` for callers that need the full score row
 * (trainer/lru.py:33, demo/inference.py:48). */
int lr_lru_scores_last(lr_lru_t* h, const int64_t* ids, int32_t B, int32_t L,
                       int32_t exclude_history, float* out_scores, void* workspace,
                       size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * LRURec user states: append ids to a stored recurrence state instead of re-encoding the history.
 * No counterpart in the reference (it re-runs LRURec.forward on the whole sequence, demo/inference.py:46-53).
 * ------------------------------------------------------------------------------------------
 * The encoder's recurrence h_t = lambda * h_{t-1} + bu_t is a sequential scan and everything around it is per position,
 * so (h_re, h_im) of every block after t tokens summarises the history. A caller-owned DEVICE table keeps one row per
 * user ("slot"); a row of a model with nb blocks is
 *     float   h[nb][2][128]   re | im per block, channel order of the packed image's lam_re / lam_im
 *     float   q[64]           the last hidden state written (what lr_lru_encode_last returns for the history so far)
 *     int32_t live            tokens since reset, saturating at INT32_MAX; only `== 0` is read
 *     padding to a multiple of 256 bytes      (lr_lru_user_state_row_bytes(nb) = nb * 1024 + 512)
 * at byte offset slot * row_bytes; the table pointer must be 4-byte aligned. An all-zero row IS the reset state, so
 * hipMemset resets. A table copied to the host and back (or into another table of the same model) continues with the same
 * bits: that is the persistence story, there is no file format.
 *
 * CONTRACT. For a row that was reset and then advanced by ANY chunking of a history of ids >= 1, in any batch, through
 * any slot, q has the bits lr_lru_encode_last returns for that history (left padded to any length), and the top-K from
 * the state with exclude_ids = that history has the indices and scores of lr_lru_retrieve_topk.
 * The state sees EVERYTHING since reset. A caller that truncates a history to its last L ids, as the reference's datasets
 * do (dataloader/lru.py:142-151), gets a different, longer-memory answer from the state once the history exceeds L.
 *
 *   slots   : DEVICE int32 [B], row u of the call -> table row; NULL: 0..B-1 (reset: every slot, B ignored). Distinct
 *             values are the caller's duty. A value outside [0, num_slots) makes the kernel skip that row: nothing is read
 *             or written for it and its out_q row is zero.
 *   new_ids : DEVICE int64 [B][Ln], consumed left to right per user. Ids <= 0 are SKIPPED, they do not cut the history
 *             (they are the left padding that lets one call append different counts per user; only a reset cuts). Ids
 *             above num_items are embedded as row 0, as the encoder embeds them. A reset row's first live id starts the
 *             history as the encoder starts it (h = bu). NULL with Ln = 0: nothing is consumed.
 *   out_q   : DEVICE fp32 [B][64] (may be NULL): the last block's output at the user's last consumed token, also stored
 *             in the row. A user with no live id in the call keeps its state and returns its stored q; a never-advanced
 *             row returns zeros.
 * Argument checks run before any device work (LR_EINVAL / LR_EWORKSPACE with an lr_last_error text); B = 0 is LR_OK and
 * launches nothing. */

/* Pure CPU. 0 for num_blocks outside 1..LR_MAX_LRU_BLOCKS. */
size_t lr_lru_user_state_row_bytes(int32_t num_blocks);

/* Zero the listed rows (slots NULL: the whole table). Ordered on hip_stream. */
int lr_lru_user_state_reset(lr_lru_t* h, void* states, int32_t num_slots, const int32_t* slots, int32_t B,
                            void* hip_stream);

/* Append new_ids to the users' states. Needs no workspace. */
int lr_lru_user_state_advance(lr_lru_t* h, void* states, int32_t num_slots, const int32_t* slots,
                              const int64_t* new_ids, int32_t B, int32_t Ln, float* out_q, void* hip_stream);

/* lr_lru_user_state_advance, then the item GEMM and ordered top-K of lr_lru_retrieve_topk on the resulting q.
 *   new_ids NULL with Ln = 0: query only.
 *   exclude_ids: DEVICE int64 [B][Lx], the caller's history for the -1e9 mask (ids and the pad id 0, as
 *             lr_lru_retrieve_topk masks with exclude_history = 1), Lx <= 8192; NULL with Lx = 0: nothing is masked.
 *   workspace: lr_lru_workspace_bytes(h, B, K, max(Lx, 1)) bytes. */
int lr_lru_retrieve_topk_user_state(lr_lru_t* h, void* states, int32_t num_slots, const int32_t* slots,
                                    const int64_t* new_ids, int32_t B, int32_t Ln, const int64_t* exclude_ids,
                                    int32_t Lx, int32_t K, int32_t* out_idx, float* out_score, void* workspace,
                                    size_t workspace_bytes, void* hip_stream);

/* States seeded from WHOLE histories by the batched encoder's own pass: one call encodes ids[B][L] (q as
 * lr_lru_encode_last, same bits) and leaves every listed row ready for lr_lru_user_state_advance -- the encoder's
 * recurrence already holds each block's state at each user's last row; these calls write it to the table instead of
 * dropping it. Day-one users of a deployed system, or users whose state was lost, need no bootstrap through advance.
 *
 * CONTRACT ADDED. For a history ending in an id >= 1 the row has the bytes (h, q, the `live == 0` test) that reset plus
 * lr_lru_user_state_advance of the same LIVE ids leaves, so every later advance / retrieve_topk_user_state on it returns
 * the bits of lr_lru_encode_last / lr_lru_retrieve_topk on the concatenated history.
 *   - The state written is that of the live tokens the encoder processed: the ids behind the last id <= 0 among the first
 *     L-1 positions. A pad in the middle CUTS (the state equals reset + advance of what follows the cut); ids above
 *     num_items are embedded as row 0, as everywhere.
 *   - A history whose LAST id is <= 0 (the all-pad row included) is outside the states' contract: the encoder embeds that
 *     pad as a token, a state skips it. Its table row is written as the reset state (zeros in h, q, live); its out_q row
 *     stays the encoder's.
 *   - The call OVERWRITES h, q and live of each listed row (padding bytes are left alone); no reset is needed first.
 *   - A slot outside [0, num_slots): nothing of the table is read or written for that user. Its out_q row is still the
 *     encoder's (the history is in the call) -- unlike advance, which answers zeros. Distinct slots are the caller's duty.
 *   - These calls need the batched MFMA encoder: a workspace that is NULL or smaller than
 *     lr_lru_user_state_encode_workspace_bytes(h, B, K, L) is LR_EWORKSPACE (there is no scratch-free form).
 * Argument checks run before any device work, with lr_last_error texts; B = 0 is LR_OK and launches nothing. */

/* lr_lru_workspace_bytes(h, max_users, max_k, max_len) plus the export buffers of blocks 0 .. nb-2:
 * (nb - 1) * min(max_users, users per encoder chunk at max_len) * 1 KB, 256-byte aligned; nothing more for nb = 1.
 * NULL h returns 0 and sets lr_last_error. Monotone like lr_lru_workspace_bytes. For lr_lru_user_state_encode pass
 * max_k = 1. */
size_t lr_lru_user_state_encode_workspace_bytes(const lr_lru_t* h, int32_t max_users, int32_t max_k, int32_t max_len);

/* lr_lru_encode_last on ids[B][L] that also writes the users' table rows. out_q: DEVICE fp32 [B][64], may be NULL. */
int lr_lru_user_state_encode(lr_lru_t* h, void* states, int32_t num_slots, const int32_t* slots, const int64_t* ids,
                             int32_t B, int32_t L, float* out_q, void* workspace, size_t workspace_bytes,
                             void* hip_stream);

/* lr_lru_retrieve_topk (same top-K plan, same bits in out_idx / out_score) whose encoder pass also writes the users'
 * table rows. */
int lr_lru_retrieve_topk_seed_user_state(lr_lru_t* h, void* states, int32_t num_slots, const int32_t* slots,
                                         const int64_t* ids, int32_t B, int32_t L, int32_t K, int32_t exclude_history,
                                         int32_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes,
                                         void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Ranking metrics  (trainer/utils.py:43-90 with preprocessed ranks)
 * ------------------------------------------------------------------------------------------ */

/* Rank histogram (integer work on the GPU, exact and order-independent):
 *   ranked: DEVICE int32 [B][Kmax] ids best-first (item ids for stage 1, class ids 0..C-1 for
 *           stage 2); labels: DEVICE int64 [B]; hist: DEVICE int64 [Kmax+1].
 *   hist[p] += number of rows whose label sits at rank p (0-based); hist[Kmax] += rows whose
 *   label is not among the Kmax ranked ids. The caller zeroes hist first. Data-parallel ranks
 *   all-reduce (sum) the histogram: every metric below is a function of it. */
int lr_rank_histogram(const int32_t* ranked, int32_t Kmax, const int64_t* labels, int32_t B,
                      int64_t* hist, void* hip_stream);

/* Full descending ranking of C <= 64 class scores per row (ties -> lower class id first).
 * Replaces `(-scores).argsort(dim=1)` (trainer/utils.py:55) for the reranker's [N][20]
 * verbalizer scores (trainer/llm.py:63-72). scores: DEVICE fp32 [B][C]; out: DEVICE int32 [B][C].
 * items (DEVICE int32 [B][C], may be NULL): when given, out[b][rank] = items[b][class] -- the
 * candidate item ids in reranked order -- instead of the class id. */
int lr_rank_classes(const float* scores, int32_t B, int32_t C, const int32_t* items,
                    int32_t* out_ranked, void* hip_stream);

/* Pure CPU: Recall@k / MRR@k / NDCG@k NUMERATORS (sums over users, float64) from a HOST
 * histogram: sums[3*j+0..2] for k = ks[j]. One relevant item per user, so Recall's denominator
 * min(k, 1) and the ideal DCG are 1 (trainer/utils.py:63-88). Divide by the user count for the
 * reference's batch-mean (trainer/utils.py:68,76,87) / per-user average (trainer/lru.py:134-137). */
int lr_metrics_from_histogram(const int64_t* hist, int32_t Kmax, const int32_t* ks, int32_t nk,
                              double* sums);

/* ------------------------------------------------------------------------------------------
 * Stage 2: Llama-2 ranker -- single prefill + verbalizer gather
 * (model/llm.py:35-145, HF LlamaModel, trainer/verb.py:524-544, trainer/llm.py:63-72)
 * ------------------------------------------------------------------------------------------ */

typedef struct LrLlamaConfig {
  int32_t vocab_size;
  int32_t hidden_size;
  int32_t intermediate_size;
  int32_t num_layers;
  int32_t num_heads;
  int32_t num_kv_heads;          /* == num_heads for Llama-2-7b; GQA is supported */
  int32_t head_dim;              /* hidden_size / num_heads */
  int32_t max_positions;         /* RoPE table length (>= llm_max_text_len = 1536) */
  float rms_eps;
  float rope_theta;
} LrLlamaConfig;

/* All pointers are DEVICE pointers to bf16 (uint16) row-major [out][in] matrices, as stored
 * by HF (nn.Linear.weight). LoRA adapters must be merged into q_proj/v_proj beforehand
 * (W + (alpha/r) B A; config.py:257-260, train_ranker.py:71-79). */
typedef struct LrLlamaLayerWeights {
  const uint16_t* input_norm;    /* [hidden]                input_layernorm.weight */
  const uint16_t* wqkv;          /* [(nh+2*nkv)*hd][hidden] q_proj;k_proj;v_proj stacked; inside every q and
                                    k head the rows are pair-interleaved for the fused rotary epilogue:
                                    row 2i = HF row i, row 2i+1 = HF row i + hd/2 (lr_llama_pack_qkv).
                                    q.k dot products are unchanged by this permutation. */
  const uint16_t* wo;            /* [hidden][nh*hd]         o_proj */
  const uint16_t* post_norm;     /* [hidden]                post_attention_layernorm.weight */
  const uint16_t* wgu;           /* [2*inter][hidden]       gate_proj / up_proj, interleaved in
                                    blocks of 16 rows: rows [32t,32t+16) = gate[16t..16t+16),
                                    rows [32t+16,32t+32) = up[16t..16t+16)  (lr_llama_pack_gate_up) */
  const uint16_t* wdown;         /* [hidden][inter]         down_proj */
} LrLlamaLayerWeights;

typedef struct LrLlamaWeightsDesc {
  const uint16_t* embed;         /* [vocab][hidden]  model.embed_tokens.weight */
  const uint16_t* final_norm;    /* [hidden]         model.norm.weight */
  const uint16_t* lm_head;       /* [vocab][hidden]  lm_head.weight */
  const LrLlamaLayerWeights* layers; /* HOST array [num_layers] of device pointers */
} LrLlamaWeightsDesc;

typedef struct lr_llama lr_llama_t;

int lr_llama_create(const LrLlamaConfig* cfg, const LrLlamaWeightsDesc* w, lr_llama_t** out);
void lr_llama_destroy(lr_llama_t* h);

/* Backbone arithmetic of a family that shares Llama's layer structure (rotate-half RoPE, gated MLP, RMSNorm, GQA/MQA)
 * but rounds differently. All zeros except embed_scale = 1 is Llama (lr_llama_create). Gemma v1 (the reference's
 * GemmaForCausalLMPatched, model/llm.py:354-456, over HF GemmaModel) is {1, 1, bf16(sqrt(hidden_size))}:
 *   norm_style 1: RMSNorm = bf16(x * rstd * (1 + w)), all in fp32 (HF GemmaRMSNorm; Llama: bf16(w * bf16(x * rstd)))
 *   mlp_act 1   : gated MLP with tanh-approximate GELU (gelu_pytorch_tanh) instead of SiLU, same bf16 rounding points
 *   embed_scale : embedding rows multiplied by it, bf16(bf16(e) * embed_scale) (HF casts the scale to the weight dtype:
 *                 45.25 for hidden 2048)
 * A Gemma handle scores (prefill, verbalizer, last logits); it has no folded norms and no LoRA fine-tuning
 * (lr_llama_set_folded_norms and lr_llama_lora_create return LR_EUNSUPPORTED). The tied lm_head is passed as
 * LrLlamaWeightsDesc.lm_head = embed (unscaled). */
typedef struct LrLlamaArch {
  int32_t norm_style;    /* 0 = Llama, 1 = Gemma */
  int32_t mlp_act;       /* 0 = SiLU, 1 = GELU (tanh approximation) */
  float embed_scale;     /* 1 = none */
  int32_t reserved[5];   /* must be zero */
} LrLlamaArch;

/* lr_llama_create with an explicit arch (NULL = Llama). lr_llama_create(c, w, out) == lr_llama_create_ex(c, NULL, w, out). */
int lr_llama_create_ex(const LrLlamaConfig* cfg, const LrLlamaArch* arch, const LrLlamaWeightsDesc* w, lr_llama_t** out);

/* Kernel selection: 0 = auto (default), 1 = generic kernels (any shape; the in-library cross-check of the fast
 * ones), attention 2 = head_dim-128 MFMA flash attention (K/V by LDS-DMA, 128 query rows per workgroup),
 * attention 3 = head_dim-128 flash attention on 256-row tiles, one wave per SIMD, persistent workgroups (shared prefix of at
 * most 64 tokens, falls back to 2 otherwise; ahead of 2 on long prompts -- thousands of tokens -- and behind it on this
 * path's 460 .. 1 125-token prompts, so auto keeps 2),
 * attention 4 = head_dim-256 MFMA flash attention (Gemma; 8 waves x 16 query rows per workgroup, K/V by LDS-DMA; a
 * shared prefix and the pruned last layer's one-query-row mode run on its kernels of llama_attn_hd256_prefix.hip, with the
 * same bits); auto takes it in the prefill for head_dim 256, and any other head_dim is LR_EUNSUPPORTED,
 * attention 5 = head_dim-64 MFMA flash attention (Llama-3.2-1B; 4 waves x 32 query rows per workgroup, K/V by LDS-DMA, no
 * lse; a shared prefix and the one-query-row mode as for 4, llama_attn_hd64_prefix.hip); auto takes it in the prefill for head_dim 64, and any other head_dim is LR_EUNSUPPORTED,
 * attention 6 = head_dim-64 MFMA flash attention for training: variant 5's forward, optionally writing lse (without lse
 * the same bits as 5), and the head_dim-64 MFMA backward (two passes, one owner per gradient element, no atomics); the
 * LoRA step's auto takes the pair at head_dim 64, and any other head_dim is LR_EUNSUPPORTED. A LoRA engine on a base set to
 * 4, 5 or 7 fails (those kernels write no lse),
 * attention 7 = head_dim-96 MFMA flash attention (Phi-3-mini; 4 waves x 32 query rows per workgroup, K/V by LDS-DMA, no lse and
 * no backward; a shared prefix and the one-query-row mode as for 5, llama_attn_hd96_prefix.hip); auto takes it in the prefill
 * for head_dim 96, and any other head_dim is LR_EUNSUPPORTED,
 * attention 8 = head_dim-96 MFMA flash attention for training: variant 7's forward, optionally writing lse (without lse
 * the same bits as 7, with a shared prefix and in the one-query-row mode too), and the head_dim-96 MFMA backward (two passes,
 * one owner per gradient element, no atomics); the LoRA step's auto takes the pair at head_dim 96, and any other head_dim is
 * LR_EUNSUPPORTED,
 * attention 9 = head_dim-256 MFMA flash attention for training: variant 4's forward, optionally writing lse (without lse
 * the same bits as 4, with a shared prefix and in the one-query-row mode too; no soft-capped form: LR_EUNSUPPORTED on a handle
 * with attn_logit_softcapping), and the head_dim-256 MFMA backward (two passes, one owner per gradient element, no atomics);
 * the LoRA step's auto takes the pair at head_dim 256, and any other head_dim is LR_EUNSUPPORTED,
 * gemm 4 = the ping-pong pipelined 256x256x64 MFMA GEMM (an error if a shape does not fit).
 * gemm 5 = LATENCY MODE for the online single-user path (demo/inference.py:56-76):
 * variant 4 plus split-K wherever the output tiles alone would leave most CUs idle (a 460-token prompt
 * gives o_proj / down_proj 32 tiles for 256 CUs); shapes that do not fit fall back as in auto. The
 * split-K summation order depends on the token count, so unlike the default a prompt's scores are
 * then reproducible only for the same packed batch size (bf16-level differences otherwise).
 * gemm 6 = auto with a RAGGED LAST COLUMN TILE: a product with N % 64 == 0 but N % 256 != 0 (K % 64 == 0, at least 128 rows,
 * store / residual / rope epilogue, no folded norm) runs variant 4's 256x256x64 body on ceil(N / 256) column tiles instead of
 * the generic kernel -- same arithmetic, rows of B and columns of C past N never addressed. Every other product goes where
 * auto sends it, with auto's bits. For models whose widths miss the tile (Qwen2-0.5B: hidden 896, qkv 1152);
 * llamarec_amd.llm makes it the default of a qwen2 ranker.
 * gemm 7 = ROW-INVARIANT LATENCY MODE, the online mode of ranker sessions: variant 5 with the number of splits fixed by the
 * weight's shape alone -- what variant 5 chooses at one row tile (lr_gemm_splitk_plan) -- and the rows launched in chunks of
 * as many 256-row tiles as the split-K workspace holds. A row's arithmetic then does not depend on how many rows the launch
 * has: a prompt's scores are reproducible in any batch, lr_llama_extend_verbalize runs it and carries the bits of the
 * whole-prompt call in this mode, and up to 256 rows it is variant 5 bit for bit. It names that one route: a product whose
 * widths miss the 256 tile (N % 256 != 0 or K % 64 != 0) is LR_EINVAL under 7, where variant 5 falls back as auto does; a
 * product too short to split runs as variant 4, which is row-invariant too. The price is paid at large M: a 32 k-row batch
 * is many serial launches. Bulk scoring stays on auto. */
int lr_llama_set_variants(lr_llama_t* h, int32_t gemm_variant, int32_t attention_variant);

/* RoPE frequency scaling (Llama-3.1 / 3.2: rope_scaling.rope_type = "llama3" in config.json). Per frequency j of the rotary
 * table, inv = theta^(-2j/head_dim) and wavelen = 2 pi / inv, all in fp32:
 *   wavelen > original_max_positions / low_freq_factor  : inv / factor
 *   wavelen < original_max_positions / high_freq_factor : inv
 *   otherwise s = (original_max_positions / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor),
 *             inv = (1 - s) * inv / factor + s * inv
 * (HF's _compute_llama3_parameters; the attention factor is 1). The rule acts at EVERY position, not only past
 * original_max_positions. LR_EINVAL for an unknown kind, a non-zero reserved word, factor < 1, original_max_positions < 1
 * or anything but 0 < low_freq_factor < high_freq_factor. */
typedef struct LrRopeScaling {
  int32_t kind;                    /* 0 = none (plain RoPE), 1 = llama3, 2 = linear: inv / factor at every frequency (reads
                                    * factor only, finite and > 0; the three llama3 words must be zero, LR_EINVAL otherwise;
                                    * Gemma-3's global layers) */
  float factor, low_freq_factor, high_freq_factor;
  int32_t original_max_positions;
  int32_t reserved[3];             /* must be zero */
} LrRopeScaling;
/* The handle's prefill, and the forward and backward of every LoRA engine created from it, build their rotary table with
 * these words from then on. NULL or kind 0: plain RoPE (the default). */
int lr_llama_set_rope_scaling(lr_llama_t* h, const LrRopeScaling* s);

/* Gemma-2 (model_type "gemma2") on a handle created with the Gemma arch (norm_style 1, mlp_act 1, embed_scale
 * bf16(sqrt(hidden))). What it adds to Gemma v1's layer, per HF Gemma2Model:
 *   attention   scores * attn_scale (query_pre_attn_scalar^-0.5: a config value, 1/16 for gemma-2-2b / 9b and 1/12 for 27b,
 *               not derived from head_dim), then attn_softcap * tanh(. / attn_softcap) in fp32, then the causal mask and softmax
 *   sandwich    h = attn(input_norm(x));  x = x + attn_out_norm(h);   h = mlp(post_norm(x));  x = x + mlp_out_norm(h)
 *               -- all Gemma norms. NAMES: LrLlamaLayerWeights.post_norm stays the norm IN FRONT of the MLP, which is HF's
 *               pre_feedforward_layernorm for Gemma-2; HF's post_attention_layernorm is attn_out_norm here and
 *               post_feedforward_layernorm is mlp_out_norm.
 *   head        final_softcap * tanh(logit / final_softcap) on the bf16 logit (HF's three bf16 steps), then fp32
 * Sliding-window layers are NOT windowed: a caller keeps prompts within sliding_window tokens, where the window is the plain
 * causal mask (llamarec_amd.llm refuses longer ones).
 * Routing: with attn_softcap > 0, attention variants 0 and 4 at head_dim 256 run the soft-capped MFMA kernels (whole prompts,
 * shared prefix, pruned last layer: same bits in all three); any other head_dim, or variant 1, runs the generic kernel with
 * the cap (slow but correct: gemma-2-27b's head_dim 128); variants 2, 3, 5, 6 make the prefill return LR_EUNSUPPORTED.
 * The MFMA kernels take caps up to 256 (their tanh has an ABSOLUTE error of about 1.7e-7 cap; Gemma-2's caps are 50 and 30); a
 * larger attn_softcap runs the generic kernel at head_dim 256 too. With a cap, a shared prefix is kept only where the capped
 * MFMA kernels run; everywhere else every prompt runs whole (same scores).
 * LR_EINVAL, handle unchanged: a negative or non-finite cap or scale, a non-zero reserved word, one norm array without the
 * other, a null layer pointer. LR_EUNSUPPORTED: any extension on a handle whose norm_style is not Gemma's (so no LoRA engine
 * can exist on a handle that takes one); an attn_scale other
 * than head_dim^-0.5 without an attn_softcap (the uncapped MFMA kernels have their scale compiled in). With an extension set,
 * lr_llama_set_folded_norms (non-NULL) and lr_llama_lora_create return LR_EUNSUPPORTED. NULL: back to the plain layer. */
typedef struct LrGemma2Ext {
  float attn_softcap;        /* 0 = none */
  float final_softcap;       /* 0 = none */
  float attn_scale;          /* 0 = head_dim^-0.5 */
  int32_t reserved[5];       /* must be zero */
  const uint16_t* const* attn_out_norm;  /* HOST array [num_layers] of DEVICE bf16 [hidden], or NULL with mlp_out_norm */
  const uint16_t* const* mlp_out_norm;   /* HOST array [num_layers] of DEVICE bf16 [hidden] */
} LrGemma2Ext;
int lr_llama_set_gemma2(lr_llama_t* h, const LrGemma2Ext* ext);

/* Qwen2 (model_type "qwen2"): Llama's layer with a bias on q_proj, k_proj and v_proj. bqkv: HOST array [num_layers] of DEVICE
 * bf16 [(num_heads + 2 num_kv_heads) * head_dim], 8-byte aligned, in wqkv's row order (q and k pair-interleaved per head like
 * lr_llama_pack_qkv's rows, v plain); the caller keeps the arrays alive. Every product of the prefill that reads wqkv -- the
 * whole-prompt QKV product, the pruned last layer's K/V and Q products, the shared-prefix path, latency mode -- adds the
 * matching slice in its epilogue: x = bf16(fp32 acc + fp32(bias[col])), one rounding, in front of the rotation.
 * NULL: back to no bias. LR_EINVAL, handle unchanged: a null or misaligned entry. LR_EUNSUPPORTED: a handle with folded
 * norms. With a bias set, lr_llama_set_folded_norms (non-NULL) and lr_llama_lora_create[_ex] return LR_EUNSUPPORTED (the
 * live-adapter forward rotates in a kernel that knows no bias). */
int lr_llama_set_qkv_bias(lr_llama_t* h, const uint16_t* const* bqkv);

/* Qwen3 (model_type "qwen3"): Llama's layer with an RMSNorm over head_dim on every q head and every k head, between the
 * projection and the rotation (HF's Qwen3RMSNorm: bf16(w * bf16(x * rsqrt(mean(x^2) + rms_eps))), fp32 statistics). q_norm /
 * k_norm: HOST arrays [num_layers] of DEVICE bf16 [head_dim], 16-byte aligned, permuted like a head's rows of wq / wk
 * (entry 2i = HF's weight i, 2i + 1 = HF's weight i + head_dim / 2); the caller keeps the arrays alive. With norms set every
 * product of the prefill that reads wqkv -- the whole-prompt QKV product, the pruned last layer's K/V and Q products, the
 * shared-prefix path, latency mode -- stores plainly, and one sweep (lr_qk_norm_rope_bf16's kernel) norms and rotates its q / k
 * columns in place; the LoRA step (lr_llama_lora_create[_ex] accepts such a handle) norms in its own forward sweep and
 * differentiates through the norm (lr_qk_norm_bwd_bf16's kernel; the norm weights are frozen).
 * NULL, NULL: back to Llama's layer. LR_EINVAL, handle unchanged: one array without the other, a null or misaligned entry.
 * LR_EUNSUPPORTED: a handle with folded norms, a Gemma-2 extension or q/k/v biases (lr_llama_set_folded_norms (non-NULL),
 * lr_llama_set_gemma2 (non-NULL) and lr_llama_set_qkv_bias (non-NULL) refuse a handle with q/k norms likewise), or a head_dim
 * that is not a power of two from 16 to 256. */
int lr_llama_set_qk_norm(lr_llama_t* h, const uint16_t* const* q_norm, const uint16_t* const* k_norm);

/* Gemma-3 (model_type "gemma3_text") on a handle created with the Gemma arch (norm_style 1, mlp_act 1, embed_scale
 * bf16(sqrt(hidden))). What it adds to Gemma v1's layer, per HF Gemma3TextModel:
 *   sandwich    as Gemma-2 (LrGemma2Ext above, same NAMES: post_norm stays the norm in front of the MLP)
 *   q/k norm    a Gemma norm over head_dim on every q head and every k head between the projection and the rotation:
 *               bf16(x * rsqrt(mean(x^2) + rms_eps) * (1 + w)) in fp32, one rounding (lr_qk_norm_rope_ex_bf16, norm_style 1)
 *   layer kinds layer l is sliding when layer_is_sliding[l] == 1, global when 0
 *   window      a sliding layer's query at position i sees keys j with i - sliding_window < j <= i (sliding_window keys, itself
 *               included); a global layer the plain causal range
 *   rotation    sliding layers: base rope_theta_local, unscaled. Global layers: LrLlamaConfig.rope_theta, every inverse
 *               frequency divided by global_linear_factor (LrRopeScaling kind 2). The handle builds both tables per call and
 *               every product that rotates -- the whole-prompt QKV sweep, the pruned last layer's K/V and Q sweeps, latency
 *               mode -- reads the one of its layer. lr_llama_set_rope_scaling's words are not read by such a handle.
 *   scores      q.k * head_dim^-0.5, no soft cap anywhere. attn_scale = 0 means that; any other value than head_dim^-0.5 is
 *               LR_EUNSUPPORTED (the uncapped MFMA kernels have their scale compiled in, as for Gemma-2 without a cap).
 * Routing: when every prompt of a call is within sliding_window tokens the window is the plain causal mask and the call runs
 * exactly the kernels a Gemma handle with these norms would run, shared prefix and last-row mode included. When a prompt is
 * longer, the sliding layers run the windowed head_dim-256 MFMA kernels (attention variants 0, 4 and 9 at head_dim 256; whole
 * prompts and the pruned last layer's one-row mode: same bits) or, for any other head_dim or variant, the generic kernel with
 * the window; the global layers run what they ran; and prefix_len is treated as 0 -- every prompt runs whole (same scores): no
 * windowed kernel reads a shared prefix.
 * q_norm / k_norm: bf16 [head_dim] permuted like a head's rows of wq / wk (entry 2i = HF's weight i, 2i + 1 = HF's weight
 * i + head_dim / 2). All four weight arrays: HOST arrays [num_layers] of DEVICE pointers, 16-byte aligned; the caller keeps the
 * device arrays alive (the host arrays are copied).
 * LR_EINVAL, handle unchanged: sliding_window < 1, a layer kind other than 0 / 1, a non-finite or non-positive rope_theta_local, a
 * non-finite or negative global_linear_factor or attn_scale, a null array, a null or misaligned entry, a non-zero reserved word.
 * LR_EUNSUPPORTED, handle unchanged: a handle whose norm_style is not Gemma's, or one with folded norms, a Gemma-2 extension,
 * q/k/v biases or Qwen3 norms; a head_dim that is not a power of two from 16 to 256. With the extension set,
 * lr_llama_set_gemma2 (non-NULL), lr_llama_set_qkv_bias (non-NULL), lr_llama_set_qk_norm, lr_llama_set_folded_norms (non-NULL)
 * and lr_llama_lora_create[_ex] return LR_EUNSUPPORTED. NULL: back to the plain Gemma layer. */
typedef struct LrGemma3Ext {
  int32_t sliding_window;           /* >= 1 */
  float rope_theta_local;           /* the sliding layers' rotary base (rope_local_base_freq) */
  float global_linear_factor;       /* 0 or 1 = none */
  float attn_scale;                 /* 0 = head_dim^-0.5 */
  int32_t reserved[4];              /* must be zero */
  const uint8_t* layer_is_sliding;  /* HOST [num_layers]: 1 = sliding, 0 = global */
  const uint16_t* const* q_norm;         /* HOST array [num_layers] of DEVICE bf16 [head_dim], packed order */
  const uint16_t* const* k_norm;
  const uint16_t* const* attn_out_norm;  /* HOST array [num_layers] of DEVICE bf16 [hidden]: HF's post_attention_layernorm */
  const uint16_t* const* mlp_out_norm;   /* HF's post_feedforward_layernorm */
} LrGemma3Ext;
int lr_llama_set_gemma3(lr_llama_t* h, const LrGemma3Ext* ext);

/* Folded RMSNorm (optional, scoring path only). HF's layer computes  proj(norm_w * bf16(x * rstd))  with its own
 * read-and-write pass over the residual stream in front of q/k/v_proj and of gate/up_proj (LlamaRMSNorm, reached from
 * model/llm.py:89-100). Here the norm weight can be multiplied into the projection matrices once at load
 * (lr_fold_norm_bf16: out[j][k] = bf16(w[j][k] * norm_w[k]), DEVICE pointers) and handed over with
 * lr_llama_set_folded_norms (HOST arrays [num_layers] of DEVICE pointers: wqkv * diag(input_norm), wgu *
 * diag(post_norm), layouts as in LrLlamaLayerWeights; the caller keeps them alive). The prefill then reads each row
 * once for rstd = 1 / sqrt(mean(x^2) + eps) and the GEMM epilogue scales its fp32 accumulator rows by it:
 * rstd * (x . (W_j * w)) == (x * rstd * w) . W_j up to bf16 rounding points (two activation roundings fewer, one weight
 * rounding more; within the parity tolerance of tests/test_gpu_llama.py). The original matrices stay in use for the
 * last layer's B pruned rows and for LoRA fine-tuning. Passing two NULLs restores the separate RMSNorm pass. */
int lr_fold_norm_bf16(const uint16_t* w, const uint16_t* norm_w, int32_t rows, int32_t cols, uint16_t* out,
                      void* hip_stream);
int lr_llama_set_folded_norms(lr_llama_t* h, const uint16_t* const* wqkv_folded, const uint16_t* const* wgu_folded);

/* Last-layer pruning (default ON): after the final layer only each prompt's last token is consumed
 * (model/llm.py:131), so that layer computes K/V for all tokens but attention output, o_proj and the
 * MLP for B rows only. Results are unchanged up to bf16 summation order; disable for A/B tests. */
int lr_llama_set_last_layer_pruning(lr_llama_t* h, int32_t enable);

/* Device workspace bytes for up to max_tokens packed tokens and max_seqs sequences per call. */
size_t lr_llama_workspace_bytes(const lr_llama_t* h, int32_t max_tokens, int32_t max_seqs);

/* One prefill over B packed (unpadded) prompts + verbalizer gather at each prompt's last token.
 * Replaces LlamaForCausalLM.forward (patched, model/llm.py:35-145: logits[:, -1] in fp32) followed
 * by ManualVerbalizer.process_logits (trainer/verb.py:546-586 == logits[:, label_token_ids],
 * SURVEY.md 8(a) a17) -- only the C verbalizer rows of lm_head are evaluated.
 *   packed_ids     : DEVICE int32 [total_tokens]; prompt b occupies [cu_seqlens[b], cu_seqlens[b+1])
 *   cu_seqlens     : DEVICE int32 [B+1] AND the same values in host memory (cu_seqlens_host),
 *                    used only for launch geometry
 *   label_token_ids: DEVICE int32 [C]  (tokenizer.encode(chr(65+c)), trainer/verb.py:494)
 *   out_scores     : DEVICE fp32 [B][C]
 */
int lr_llama_prefill_verbalize(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                               const int32_t* cu_seqlens_host, int32_t B,
                               const int32_t* label_token_ids, int32_t C, float* out_scores,
                               void* workspace, size_t workspace_bytes, void* hip_stream);

/* The same call when every prompt of the batch starts with the same prefix_len tokens -- the template text in front
 * of the first history item (dataloader/utils.py:24-40, templates/alpaca_short.json:3; about 36 Llama-2 tokens) --
 * which is then evaluated ONCE: internally the batch is laid out as [prefix][rest of prompt 0]...[rest of prompt B-1]
 * and the attention kernel reads keys/values of positions < prefix_len from the prefix rows. Inputs are the caller's
 * ordinary packed prompts (prefix included in each). Scores are BIT-IDENTICAL to lr_llama_prefill_verbalize.
 * Preconditions: 0 <= prefix_len < the shortest prompt; ids[cu[b] + i] == ids[cu[0] + i] for all b, i < prefix_len
 * (lr_common_prefix_len computes the largest such value from host copies). The second precondition is VERIFIED on the
 * device: if any prompt's first prefix_len ids differ from prompt 0's, every score of the call is NaN (prefix rows, keys
 * and values come from prompt 0, so a stale prefix_len would otherwise score the other prompts silently wrong).
 * prefix_len = 0, B = 1, a head_dim other than 64 / 96 / 128 / 256, the generic attention variant or a variant that does not
 * belong to the head_dim run the plain path. */
int lr_llama_prefill_verbalize_prefix(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                                      const int32_t* cu_seqlens_host, int32_t B, int32_t prefix_len,
                                      const int32_t* label_token_ids, int32_t C, float* out_scores,
                                      void* workspace, size_t workspace_bytes, void* hip_stream);
/* Host helper (pure CPU): longest token prefix shared by all B prompts, capped at (shortest prompt - 1). */
int32_t lr_common_prefix_len(const int32_t* packed_ids_host, const int32_t* cu_seqlens_host, int32_t B);

/* Compatibility: full last-position logits fp32 [B][vocab] (model/llm.py:131). */
int lr_llama_last_logits(lr_llama_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                         const int32_t* cu_seqlens_host, int32_t B, float* out_logits,
                         void* workspace, size_t workspace_bytes, void* hip_stream);

/* Ranker sessions: a per-user K / V cache of the prompt prefix (the stage-2 half of the user-state work above). The demo
 * prompt numbers the history (1) .. (n) without truncating it, so when a user adds an item, or is ranked against another
 * candidate pool, everything up to the end of the old history is token for token the prompt that was just prefilled. A
 * slot keeps the rotated keys and the values of those tokens for every layer; a call prefills only the new tokens,
 * attends over cache plus new tokens and returns the verbalizer scores.
 *
 * The caller owns one DEVICE table [num_slots][slot_bytes], 16-byte aligned. A slot is
 *     [num_layers][max_tokens] rows of [K rotated | V], 2 * num_kv_heads * head_dim bf16 a row (row p = prompt position p),
 *     padded to a multiple of 256 bytes        (lr_llama_kv_cache_slot_bytes, pure CPU, 0 for a shape no handle can have)
 * with no header and no device-side length: how many rows of a slot are valid, and for which token ids, is host state.
 *
 * lr_llama_extend_verbalize: prompt b of the call continues slot slots[b] behind its first cached_len[b] tokens with the
 * packed ids new_ids[cu_new[b] .. cu_new[b+1]) at positions cached_len[b] .. . Their K / V rows are written into the slot and
 * out_scores[b][c] (DEVICE fp32 [B][C]) is the logit of label c at the prompt's last new token. slots, cached_len and cu_new
 * are given twice, DEVICE and HOST with the same values (the host copies are launch geometry and what is checked).
 * keep_host[b] in 0 .. q_len[b] is the number of leading new tokens the caller will count as cached afterwards; rows behind
 * it are scratch that the next call overwrites, so keep needs no device work: it is checked, and only defines what the
 * caller may pass as cached_len next time (at most cached_len[b] + keep[b]; lowering it rolls the slot back for free).
 * Scores are BIT-IDENTICAL to lr_llama_prefill_verbalize of the whole prompt (cached ids + new ids) on the same handle in
 * the default GEMM mode, at head_dim 128 on the MFMA attention kernel (variants 0 / 2) and at any head_dim on the generic
 * one (variant 1; auto off head_dim 128): rows are computed by row-invariant products and by attention kernels that keep
 * 64-key blocks and 128-row query tiles aligned to positions inside the prompt. A handle in gemm variant 7 (the
 * row-invariant latency mode: set it for online use) runs variant 7 here and the scores are BIT-IDENTICAL to the whole-prompt
 * call under variant 7; where its QKV product splits, the reduce pass writes K | V straight into the slot rows. A handle in
 * gemm variant 5, whose split depends on the row count, runs the default-mode products here, with the default mode's bits.
 * cached_len[b] = 0 with an empty slot is the plain call.
 * LR_EINVAL before anything is launched (out_scores and the table untouched): a null pointer, a table that is not 16-byte
 * aligned, a slot outside [0, num_slots), the same slot twice in one call, q_len[b] < 1, cached_len[b] < 0,
 * cached_len[b] + q_len[b] > max_tokens or > max_positions, keep[b] outside [0, q_len[b]], C < 1.
 * LR_EUNSUPPORTED: a handle with Gemma norms, a soft cap, a sliding window, q/k norms, q/k/v biases or folded norms, an
 * attention variant other than 0 / 1 / 2 (2 off head_dim 128), a slot layer of 2 GiB or more. LR_EWORKSPACE: fewer than
 * lr_llama_extend_workspace_bytes(h, new tokens, B, max_tokens) bytes. */
size_t lr_llama_kv_cache_slot_bytes(int32_t num_layers, int32_t num_kv_heads, int32_t head_dim, int32_t max_tokens);
size_t lr_llama_extend_workspace_bytes(const lr_llama_t* h, int32_t max_new_tokens, int32_t max_seqs, int32_t max_tokens);
int lr_llama_extend_verbalize(lr_llama_t* h, void* table, int32_t num_slots, int32_t max_tokens, const int32_t* slots,
                              const int32_t* slots_host, const int32_t* cached_len, const int32_t* cached_len_host,
                              const int32_t* new_ids, const int32_t* cu_new, const int32_t* cu_new_host,
                              const int32_t* keep_host, int32_t B, const int32_t* label_token_ids, int32_t C,
                              float* out_scores, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Host helper: stack HF q_proj/k_proj/v_proj ([nh*hd][hidden], [nkv*hd][hidden] x2, bf16) into the
 * wqkv layout above (pair-interleaved q/k head rows). Pure CPU. */
int lr_llama_pack_qkv(const uint16_t* q, const uint16_t* k, const uint16_t* v, int32_t num_heads,
                      int32_t num_kv_heads, int32_t head_dim, int32_t hidden, uint16_t* out);

/* Host helper: interleave gate_proj / up_proj rows ([inter][hidden] each, bf16) into the wgu
 * layout above. Pure CPU. */
int lr_llama_pack_gate_up(const uint16_t* gate, const uint16_t* up, int32_t inter, int32_t hidden,
                          uint16_t* out);

/* Load-time NF4 round trip  W -> dequant(quant(W))  of a frozen bf16 weight matrix (DEVICE pointers, n elements,
 * row-major blocks of 64): what the reference's forward effectively multiplies by, since it quantises every Linear
 * of the base model with BitsAndBytesConfig(load_in_4bit, nf4, double quant, bf16 compute) (train_ranker.py:49-56,
 * setup_demo.py:67-74; bitsandbytes 0.43.1 is absent here, its published algorithm is restated -- parity with it is
 * unpinned). double_quant != 0 also quantises the per-block absmax (8-bit dynamic code, blocks of 256, mean offset).
 * out may alias w. Synchronises the stream once when double_quant is set (load-time call).
 * lr_nf4_dynamic_map: the 256 sorted levels of that 8-bit code (HOST float[256]). */
size_t lr_nf4_scratch_bytes(size_t n);
int lr_nf4_roundtrip_bf16(const uint16_t* w, size_t n, int32_t double_quant, uint16_t* out, void* scratch,
                          size_t scratch_bytes, void* hip_stream);
int lr_nf4_dynamic_map(float* out256);

/* Stand-alone bf16 GEMM used by the prefill (exposed for parity tests and roofline runs):
 * C[M][N] = A[M][K] * B[N][K]^T, bf16 in, fp32 accumulate, bf16 out; all DEVICE pointers,
 * row-major, leading dimensions = K, K, N. variant: 0 = auto, 1 = generic (any shape),
 * 4 = 256x256x64 MFMA tile, ping-pong pipeline with balanced fragment reads and region-recycling DMA prefetch
 * (default for N%256==0, K%64==0, M>=128; any M: rows are bounds-checked), 5 = 4 with split-K (lr_gemm_bf16_nt_ws),
 * 6 = auto with a ragged last column tile for N%64==0, N%256!=0 (see lr_llama_set_variants), 7 = 5 with the split fixed by
 * (N, K) and the rows in chunks the workspace holds (lr_gemm_bf16_nt_ws; N%256==0 and K%64==0, anything else is LR_EINVAL). */
int lr_gemm_bf16_nt(const uint16_t* A, const uint16_t* B, uint16_t* C, int32_t M, int32_t N,
                    int32_t K, int32_t variant, void* hip_stream);
/* The same with a device workspace for variants 5 and 7 (split-K, see lr_llama_set_variants): fp32 partial
 * planes. Variant 5: at most 64 MiB (8 splits x M x N x 4 bytes, splits x tiles <= 256). Variant 7: any size from one row
 * tile's planes (splits x 256 x N x 4 bytes) up; a larger one means fewer launches, never other bits. */
int lr_gemm_bf16_nt_ws(const uint16_t* A, const uint16_t* B, uint16_t* C, int32_t M, int32_t N,
                       int32_t K, int32_t variant, void* workspace, size_t workspace_bytes, void* hip_stream);
/* What the GEMM entry points do with an M x N x K product under variant 5 or 7 and a workspace of workspace_bytes. Pure CPU.
 * *splits = the number of K splits (1 = not split: the product runs as variant 4, or, variant 5 only, on the generic kernel off
 * the 256 tile);
 * *rows_per_launch = the rows of one launch: M for variant 5 and for an unsplit product, for variant 7 the largest multiple
 * of 256 with splits * rows * N * 4 <= workspace_bytes (M rows take ceil(M / rows_per_launch) launch pairs).
 * LR_EWORKSPACE where the product would return it (variant 5: the M rows do not fit; variant 7: not even 256 do);
 * LR_EINVAL for another variant, a size < 1, a null pointer, or variant 7 with N % 256 != 0 or K % 64 != 0. Honours LR_GEMM_SPLITK_MIN_TILES as the products do. */
int lr_gemm_splitk_plan(int32_t variant, int32_t M, int32_t N, int32_t K, size_t workspace_bytes, int32_t* splits,
                        int32_t* rows_per_launch);

/* The projection GEMM with each of the prefill's fused epilogues (exposed for parity tests and per-shape timing):
 *   epilogue 0 store | 1 residual: C = bf16(bf16(acc) + R), R bf16 [M][N], may alias C | 2 SwiGLU over gate/up rows
 *   interleaved in groups of 16 (lr_llama_pack_gate_up), C is [M][N/2] | 3 rotary embedding on columns
 *   [0, rot_cols) of pair-interleaved q/k rows (lr_llama_pack_qkv), tok_pos int32 [M] (every entry < rope_positions),
 *   rope_cs / rope_positions = the buffer lr_rope_table filled and its max_positions | 5 GeGLU: as 2 with the tanh-approximate
 *   GELU (Gemma) in place of SiLU.
 * These are the epilogues of HF LlamaAttention / LlamaMLP around the Linears of model/llm.py:89-100 (reference). */
int lr_gemm_bf16_nt_epi(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M, int32_t N,
                        int32_t K, int32_t epilogue, int32_t variant, const int32_t* tok_pos, const float* rope_cs,
                        int32_t rope_positions, int32_t head_dim, int32_t rot_cols, void* workspace, size_t workspace_bytes,
                        void* hip_stream);
/* The same with a bf16 bias[N] (DEVICE, 8-byte aligned, indexed by output column; NULL = none), epilogues 0 and 3 only:
 * x = bf16(fp32 acc + fp32(bias[col])) -- one rounding, where lr_gemm_bf16_nt_epi rounds bf16(acc) -- then the rotation on
 * [0, rot_cols) and the store as before. A bias with epilogue 1, 2 or 5 is LR_EINVAL (nothing is launched). */
int lr_gemm_bf16_nt_bias_epi(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M, int32_t N,
                             int32_t K, int32_t epilogue, int32_t variant, const int32_t* tok_pos, const float* rope_cs,
                             int32_t rope_positions, int32_t head_dim, int32_t rot_cols, void* workspace,
                             size_t workspace_bytes, const uint16_t* bias, void* hip_stream);
/* o_proj / down_proj together with the RMSNorm that reads their result (exposed for parity tests):
 *   C = bf16(bf16(A B^T) + R),   norm_out = bf16(norm_w * bf16(C * rsqrt(mean(C^2) + eps)))     (C may alias R)
 * fuse != 0 lets a product that variant 5 splits over K write norm_out in its reduce pass (one launch less per product in
 * the online path); *was_fused (optional) reports whether that happened. Both outputs carry the same bits either way. */
int lr_gemm_bf16_nt_residual_rmsnorm(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M,
                                     int32_t N, int32_t K, int32_t variant, const uint16_t* norm_w, uint16_t* norm_out,
                                     float eps, int32_t fuse, int32_t* was_fused, void* workspace, size_t workspace_bytes,
                                     void* hip_stream);
/* The same with the norm of an LrLlamaArch: norm_style 1 = Gemma, norm_out = bf16(C * rsqrt(mean(C^2) + eps) * (1 + norm_w)). */
int lr_gemm_bf16_nt_residual_rmsnorm_ex(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M,
                                        int32_t N, int32_t K, int32_t variant, const uint16_t* norm_w, uint16_t* norm_out,
                                        float eps, int32_t norm_style, int32_t fuse, int32_t* was_fused, void* workspace,
                                        size_t workspace_bytes, void* hip_stream);
/* cs: DEVICE buffer of lr_rope_table_bytes(max_positions, head_dim) bytes: fp32 [max_positions][head_dim/2][2] = (cos, sin)
 * of position * theta^(-2i/head_dim), rounded to bf16 values (HF LlamaRotaryEmbedding casts cos/sin to the activations'
 * dtype), followed by the same values packed as bf16 pairs, uint32 [max_positions][head_dim/2] = cos | sin << 16. */
size_t lr_rope_table_bytes(int32_t max_positions, int32_t head_dim);
int lr_rope_table(float* cs, int32_t max_positions, int32_t head_dim, float theta, void* hip_stream);
/* The same with scaled frequencies (LrRopeScaling above). s = NULL or kind 0 writes lr_rope_table's bytes. */
int lr_rope_table_ex(float* cs, int32_t max_positions, int32_t head_dim, float theta, const LrRopeScaling* s,
                     void* hip_stream);

/* Stand-alone varlen causal attention (exposed for parity tests):
 * qkv: DEVICE bf16 [total][(nh+2*nkv)*hd] (RoPE already applied; any consistent permutation of the
 * dims inside q and k heads), out: bf16 [total][nh*hd]. variant 0 = auto (2 at head_dim 128, else 1), 1 generic,
 * 2 = head_dim-128 MFMA, 4 = head_dim-256 MFMA, 5 = head_dim-64 MFMA, 6 = the same kernel, which also serves _lse and has a
 * backward (_bwd), 7 = head_dim-96 MFMA (no lse, no backward), 8 = the same kernel, which also serves _lse and has a backward
 * (_bwd), 9 = variant 4's kernel, which also serves _lse and has a backward (_bwd; LR_EUNSUPPORTED off head_dim 256). auto keeps the generic kernels at head_dim 64, 96 and 256
 * here: these entry points' results are kept.
 * cu_seqlens_host (HOST int32 [B+1], the values of cu_seqlens): cu_seqlens_host[0] == 0 and strictly increasing, so that
 * every segment holds at least one row. lr_attention_varlen, _ws, _lse and _bwd check this on the host and return LR_EINVAL
 * before anything is launched (outputs untouched) when it does not hold. */
int lr_attention_varlen(const uint16_t* qkv, uint16_t* out, const int32_t* cu_seqlens,
                        const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads,
                        int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* hip_stream);
/* The same with a DEVICE workspace of lr_attention_workspace_bytes(total, B, num_heads) bytes, which variant 3 (and
 * auto, for head_dim 128) needs for its work-item list; lse: optional DEVICE fp32 [total][num_heads] log-sum-exp of
 * the scaled scores (NULL: not written). */
size_t lr_attention_workspace_bytes(int32_t total_tokens, int32_t B, int32_t num_heads);
int lr_attention_varlen_ws(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* cu_seqlens,
                           const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads, int32_t num_kv_heads,
                           int32_t head_dim, int32_t variant, void* workspace, size_t workspace_bytes, void* hip_stream);

/* The two modes of the prefill's MFMA attention kernels, stand-alone (exposed for parity tests). Both check on the host,
 * before anything is launched (outputs untouched): seg_starts_host[0] == 0 and strictly increasing, segment 0 exactly
 * prefix_len rows when prefix_len > 0 (and S >= 2), num_heads % num_kv_heads == 0 -- LR_EINVAL -- and the (variant, head_dim)
 * pair: 0 / 2 at head_dim 128, 0 / 5 at 64, 0 / 7 / 8 at 96, 0 / 4 / 9 at 256, anything else LR_EUNSUPPORTED.
 * qkv rows laid out as the prefill lays them out: segment 0 = the prefix_len shared rows, segments 1.. continue it (their
 * keys and values of positions < prefix_len are read from segment 0). out rows of every segment are written, each with the
 * bits lr_attention_varlen (same variant; at 64 / 96 / 256 variant 5 / 7 / 4) writes for that row of the whole prompt. */
int lr_attention_varlen_prefix(const uint16_t* qkv, uint16_t* out, const int32_t* seg_starts, const int32_t* seg_starts_host,
                               int32_t S, int32_t prefix_len, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim,
                               int32_t variant, void* hip_stream);
/* One query row per prompt: kv [n][2*nkv*hd] (K | V of every row), q_last / out_last [prompts][nh*hd] (the query at each
 * prompt's last position); prefix_len as above (0: S prompts, no prefix segment; > 0: S - 1 prompts). */
int lr_attention_last_rows(const uint16_t* kv, const uint16_t* q_last, uint16_t* out_last, const int32_t* seg_starts,
                           const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                           int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* hip_stream);

/* The attention of lr_llama_extend_verbalize alone (exposed for parity tests): qkv as lr_attention_varlen, the B segments
 * being the NEW rows of B prompts, segment b at positions cached_len[b] .. of slot slots[b] of the cache table described at
 * lr_llama_extend_verbalize (num_layers and layer place the rows inside a slot). The call first copies the K | V columns of
 * its rows into the slot rows cached_len[b] .. cached_len[b] + q_len[b] - 1 of that layer -- the only bytes of the table it
 * writes -- and then query row i of segment b attends to rows 0 .. cached_len[b] + i of the slot. out [total][nh*hd].
 * variant 0 = auto (2 at head_dim 128, else 1), 1 generic, 2 = head_dim-128 MFMA, whose rows carry the bits
 * lr_attention_varlen's variant 2 writes for the same rows of the whole prompt; anything else LR_EUNSUPPORTED. The host checks
 * of lr_llama_extend_verbalize apply (LR_EINVAL, nothing launched). */
int lr_attention_varlen_cached(const uint16_t* qkv, uint16_t* out, void* table, int32_t num_slots, int32_t max_tokens,
                               int32_t num_layers, int32_t layer, const int32_t* slots, const int32_t* slots_host,
                               const int32_t* cached_len, const int32_t* cached_len_host, const int32_t* cu_q,
                               const int32_t* cu_q_host, int32_t B, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim,
                               int32_t variant, void* hip_stream);

/* The same two with soft-capped scores, cap * tanh(q.k * scale / cap) (Gemma-2; exposed for parity tests). scale = 0 means
 * head_dim^-0.5. cap = 0 (with scale 0 or head_dim^-0.5) routes to lr_attention_varlen_prefix / lr_attention_last_rows: same
 * checks, same kernels, bit-identical results. cap > 0: the segment checks of those two, then variant 0 / 4 at head_dim 256
 * with cap <= 256 run the soft-capped MFMA kernels, variant 1, a larger cap or any other head_dim (prefix_len must be 0
 * there) the generic kernel, and
 * variants 2, 3, 5, 6 (and 7 / 8 at their head_dim 96, 9 at its head_dim 256) return LR_EUNSUPPORTED; lr_attention_last_rows_softcap needs head_dim 256 and variant 0 / 4.
 * A negative or non-finite scale or cap is LR_EINVAL. */
int lr_attention_varlen_softcap(const uint16_t* qkv, uint16_t* out, const int32_t* seg_starts, const int32_t* seg_starts_host,
                                int32_t S, int32_t prefix_len, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim,
                                float scale, float cap, int32_t variant, void* hip_stream);
int lr_attention_last_rows_softcap(const uint16_t* kv, const uint16_t* q_last, uint16_t* out_last, const int32_t* seg_starts,
                                   const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                                   int32_t num_kv_heads, int32_t head_dim, float scale, float cap, int32_t variant,
                                   void* hip_stream);
/* The same two with a sliding window (Gemma-3's sliding layers; exposed for parity tests): query i sees keys j with
 * i - window < j <= i. window <= 0, or window >= the longest sequence (prefix included), masks nothing and routes to
 * lr_attention_varlen_prefix / lr_attention_last_rows: same checks, same kernels, bit-identical results. Otherwise prefix_len
 * must be 0 (LR_EUNSUPPORTED: no windowed kernel reads a shared prefix) and, after the segment checks of those two, variants 0
 * and 4 at head_dim 256 run the windowed MFMA kernels, variant 1 -- and 0 / 4 at any other head_dim -- the generic kernel with
 * the window, and every other variant returns LR_EUNSUPPORTED; lr_attention_last_rows_window needs head_dim 256 and variant
 * 0 / 4, and writes for every prompt the bits lr_attention_varlen_window writes for that prompt's last row. */
int lr_attention_varlen_window(const uint16_t* qkv, uint16_t* out, const int32_t* seg_starts, const int32_t* seg_starts_host,
                               int32_t S, int32_t prefix_len, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim,
                               int32_t window, int32_t variant, void* hip_stream);
int lr_attention_last_rows_window(const uint16_t* kv, const uint16_t* q_last, uint16_t* out_last, const int32_t* seg_starts,
                                  const int32_t* seg_starts_host, int32_t S, int32_t prefix_len, int32_t num_heads,
                                  int32_t num_kv_heads, int32_t head_dim, int32_t window, int32_t variant, void* hip_stream);
/* Gemma-2's sandwich norm on [rows][d] bf16 DEVICE rows (exposed for parity tests), Gemma norms with fp32 statistics:
 *   x  <- bf16( float(x) + float(bf16(h * rsqrt(mean(h^2) + eps) * (1 + w_out))) )       in place
 *   xn  = bf16( x * rsqrt(mean(x^2) + eps) * (1 + w_next) )                               when w_next != NULL
 * xn may alias h; w_next and xn are both NULL or both given. d: a multiple of 8, at most 8192 (LR_EUNSUPPORTED). */
int lr_residual_postnorm_bf16(uint16_t* x, const uint16_t* h, const uint16_t* w_out, const uint16_t* w_next, uint16_t* xn,
                              int32_t rows, int32_t d, float eps, void* hip_stream);
/* The prefill's RMSNorm pass alone (exposed for parity tests and for timing the unfused form of the call above):
 * out = norm(x) over [rows][d] bf16 DEVICE rows, norm_style 0 = Llama bf16(w * bf16(x * rstd)), 1 = Gemma
 * bf16(x * rstd * (1 + w)); d a multiple of 8. lr_residual_postnorm_bf16 with w_next writes, bit for bit, what the same call
 * without w_next followed by lr_rmsnorm_bf16(x, w_next, xn, ..., 1) writes. */
int lr_rmsnorm_bf16(const uint16_t* x, const uint16_t* w, uint16_t* out, int32_t rows, int32_t d, float eps, int32_t norm_style,
                    void* hip_stream);
/* Qwen3's q/k norm + rotation sweep alone (exposed for parity tests and timing), in place on buf [rows][ld] bf16 DEVICE rows:
 * columns [col0, col0 + (nq + nk) head_dim) hold nq + nk heads in the packed pair-interleaved order the rope epilogue writes;
 * per (row, head) y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))) with w = q_norm for the first nq heads and k_norm for the
 * rest (bf16 [head_dim] in the packed order, 16-byte aligned; either group may be empty and its pointer NULL), then the
 * rotation of y by (cos, sin)[tok_pos[row]] of lr_rope_table's fp32 table, rounded once. Columns outside the range are neither
 * read nor written. head_dim: a power of two from 16 to 256, else LR_EUNSUPPORTED and nothing is launched; col0 and ld
 * multiples of 8. */
int lr_qk_norm_rope_bf16(uint16_t* buf, int32_t rows, int32_t ld, int32_t col0, int32_t nq, int32_t nk, int32_t head_dim,
                         const uint16_t* q_norm, const uint16_t* k_norm, float eps, const int32_t* tok_pos, const float* rope_cs,
                         void* hip_stream);

/* The same sweep with the norm's rounding as a trailing argument: norm_style 0 = the call above (same kernel, same bits),
 * 1 = Gemma-3's y = bf16(x * rsqrt(mean(x^2) + eps) * (1 + w)) in fp32 with one rounding; the rotation is unchanged. Any other
 * norm_style is LR_EINVAL. */
int lr_qk_norm_rope_ex_bf16(uint16_t* buf, int32_t rows, int32_t ld, int32_t col0, int32_t nq, int32_t nk, int32_t head_dim,
                            const uint16_t* q_norm, const uint16_t* k_norm, float eps, const int32_t* tok_pos,
                            const float* rope_cs, void* hip_stream, int32_t norm_style);

/* ------------------------------------------------------------------------------------------
 * The prefill's norm, head, embedding and metadata kernels alone (exposed for parity tests): what every scored prompt passes
 * through between the GEMMs and the attention passes, each behind one call with flat arguments. All pointers DEVICE, bf16 as
 * uint16_t. Every call checks on the host, before it launches anything, what its kernel assumes: LR_EINVAL (null pointer,
 * negative count, d not a multiple of 8, eps not finite or negative, a norm_style other than 0 / 1) or LR_EUNSUPPORTED (a
 * width the kernel has no path for, a pointer that is not 16-byte aligned where the kernel moves 16 bytes at a time), with a
 * message in lr_last_error and nothing written. Zero rows is LR_OK and launches nothing. What only the device can see is the
 * caller's promise: rows / tok_src name rows inside their arrays, cu_seqlens is increasing and every prompt longer than
 * prefix_len. The arithmetic, rounding points and element-wise error bounds of every call: tests/prefill_kernels_ref.py.
 * (lr_rmsnorm_bf16, lr_residual_postnorm_bf16, lr_gemm_bf16_nt_residual_rmsnorm_ex and lr_fold_norm_bf16 above belong here too.)
 * ------------------------------------------------------------------------------------------ */
/* Final norm of one row per prompt + the verbalizer's dot products: out[b][c] = float(bf16(sum_k xn[k] * lm_head[id_c][k])),
 * xn = norm(x[rows ? rows[b] : b]) with norm_w in norm_style (0 Llama, 1 Gemma), id_c = class_ids ? class_ids[c] : c; an id
 * outside [0, vocab) gives NaN in that column; *poison != 0 (optional device word) gives NaN everywhere. final_softcap > 0
 * (norm_style 1 only, else LR_EUNSUPPORTED): bf16(bf16(tanh(bf16(logit / cap))) * cap) on the bf16 logit. x [..][d], out fp32
 * [B][C]; lm_head 16-byte aligned; a d whose d * 2 bytes of LDS the kernel cannot have is LR_EUNSUPPORTED. */
int lr_llama_head_bf16(const uint16_t* x, const int32_t* rows, const uint16_t* norm_w, const uint16_t* lm_head,
                       const int32_t* class_ids, int32_t B, int32_t C, int32_t d, float eps, float* out, int32_t vocab,
                       const int32_t* poison, int32_t norm_style, float final_softcap, void* hip_stream);
/* out[t][:] = table[id][:] (scale == 1) or bf16(table[id][:] * scale), id = ids[tok_src ? tok_src[t] : t], an id outside
 * [0, vocab) reads row 0. table [vocab][d] and out [n][d] 16-byte aligned. */
int lr_llama_embed_bf16(const int32_t* ids, const int32_t* tok_src, const uint16_t* table, int32_t vocab, int32_t d,
                        uint16_t* out, int32_t n, float scale, void* hip_stream);
/* The packed batch's row map from cu_seqlens [B + 1]. prefix_len = 0: segment b = prompt b. prefix_len = P > 0: segment 0 =
 * prompt 0's first P tokens, segment b + 1 = prompt b from position P on. seg_start [segments + 1], tok_pos [rows] (position
 * inside the prompt), tok_src [rows] (index into the packed ids), last_rows / last_pos [B] (row and position of each prompt's
 * last token), *prefix_bad = 1 when some prompt's first P ids differ from prompt 0's (needs ids), else 0. */
int lr_llama_token_meta(const int32_t* cu_seqlens, int32_t B, int32_t prefix_len, const int32_t* ids, int32_t* seg_start,
                        int32_t* tok_pos, int32_t* tok_src, int32_t* last_rows, int32_t* last_pos, int32_t* prefix_bad,
                        void* hip_stream);
/* out[i][:] = x[rows[i]][:], rows of d bf16 values; x and out 16-byte aligned. */
int lr_gather_rows_bf16(const uint16_t* x, const int32_t* rows, int32_t n_rows, int32_t d, uint16_t* out, void* hip_stream);
/* rstd[m] = 1 / sqrt(mean(x[m][:]^2) + eps) in fp32, the statistic of the folded RMSNorm; x [rows][d] 16-byte aligned. */
int lr_rms_rstd_f32(const uint16_t* x, float* rstd, int32_t rows, int32_t d, float eps, void* hip_stream);
/* lr_gemm_bf16_nt_epi with the folded RMSNorm's row scale: epilogues 2 and 3 multiply the fp32 accumulator of row m by
 * row_scale[m] (fp32 [M]) in front of their first rounding. row_scale = NULL is lr_gemm_bf16_nt_epi bit for bit; a row scale
 * with epilogue 0, 1 or 5 is LR_EINVAL (nothing is launched). */
int lr_gemm_bf16_nt_rowscale_epi(const uint16_t* A, const uint16_t* B, uint16_t* C, const uint16_t* R, int32_t M, int32_t N,
                                 int32_t K, int32_t epilogue, int32_t variant, const int32_t* tok_pos, const float* rope_cs,
                                 int32_t rope_positions, int32_t head_dim, int32_t rot_cols, void* workspace,
                                 size_t workspace_bytes, const float* row_scale, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Optional in-library kernel timing (HIP events on the caller's stream). Not part of the
 * reference's surface: it exists so a benchmark can report the measured duration and the
 * algorithmic work of each kernel family over its timed region.
 *   kinds: 0 gemm 256x256x64 (work = flops), 1 generic gemm (flops), 2 MFMA attention (flops),
 *          3 generic attention (flops), 4 LRU encoder (users), 5 item GEMM + top-K (flops),
 *          6 element-wise (work = bytes moved; Gemma-2's sandwich-norm kernel)
 * lr_profile_start/stop bracket the region (start allocates events: call it outside graph
 * capture); lr_profile_collect is valid after the stream has been synchronised.
 * ------------------------------------------------------------------------------------------ */
int lr_profile_start(int32_t max_records);
int lr_profile_stop(void);
int lr_profile_collect(int32_t kind, double* total_ms, double* total_work, int64_t* launches);
/* Per-launch records of one kind, in launch order: ms[i], work[i], tag[i] for i < min(return value, max_records);
 * returns the number of records of that kind (-1 on error). GEMM tags: (epilogue << 56) | (N << 28) | K, so a caller
 * can report each projection shape separately. Pass max_records = 0 (arrays may be NULL) to count. */
int64_t lr_profile_records(int32_t kind, double* ms, double* work, int64_t* tag, int64_t max_records);

/* ===========================================================================================
 * Retriever training step
 *   replaces  LRUTrainer.calculate_loss                      trainer/lru.py:20-28
 *             loss.backward() through model/lru.py:38-175     (torch autograd)
 *             clip_gradients + AdamW.step                     trainer/base.py:106-112,201-246
 * One flat fp32 buffer holds every parameter in the reference's state_dict layouts (complex tensors as
 * interleaved (re, im) pairs = torch.view_as_real); gradients, and Adam's two moments have the same
 * layout, so a data-parallel job all-reduces ONE buffer between lr_lru_train_loss_grad and
 * lr_lru_train_apply. The caller owns the state buffer and the workspace (device memory).
 * =========================================================================================== */
typedef struct {
  float weight_decay;   /* 1e-2  config.py:123-124 (applied to names without "bias"/"layer_norm", trainer/base.py:222) */
  float beta1, beta2;   /* 0.9, 0.999 (torch.optim.AdamW defaults) */
  float eps;            /* 1e-9  config.py:181 */
  float max_grad_norm;  /* 5.0   config.py:184 */
  float dropout;        /* bert_dropout      0.2 config.py:216 (embedding, FFN activation, FFN output) */
  float attn_dropout;   /* bert_attn_dropout 0.2 config.py:217 (LRU layer output) */
  uint64_t seed;        /* dropout stream (own counter-based generator: torch's masks cannot be reproduced) */
  int32_t ce_mode;      /* item GEMM + cross-entropy: 0 = auto, 1 = store the [B*L][V+1] logits (<= 256 MB problems),
                           2 = fused, logits never stored (large catalogs) */
} LrLruTrainConfig;

typedef struct lr_lru_train lr_lru_train_t;

/* Bytes of DEVICE memory for parameters + gradients + Adam moments (+ a decay mask and scalars). */
size_t lr_lru_train_state_bytes(int32_t num_items, int32_t num_blocks);
/* init: HOST fp32 arrays in the reference's layouts (the same descriptor lr_lru_pack takes). */
int lr_lru_train_create(const LrLruWeightsDesc* init, const LrLruTrainConfig* cfg, void* state_dev,
                        size_t state_bytes, lr_lru_train_t** out);
void lr_lru_train_destroy(lr_lru_train_t* h);
size_t lr_lru_train_workspace_bytes(const lr_lru_train_t* h, int32_t B, int32_t L);
/* Forward + backward of one batch: tokens/labels DEVICE int64 [B][L], left-padded with 0, label 0 =
 * ignored (dataloader/lru.py:119-131). Fills the gradient buffer (zeroed first) and
 * out_loss[0] = mean CE over labelled positions, out_loss[1] = their count, out_loss[2] = number of labels
 * outside [0, num_items] (ignored like label 0; torch would raise) -- DEVICE float[3]. */
int lr_lru_train_loss_grad(lr_lru_train_t* h, const int64_t* tokens, const int64_t* labels, int32_t B,
                           int32_t L, float* out_loss, void* workspace, size_t workspace_bytes,
                           void* hip_stream);
/* clip_grad_norm_(max_grad_norm) + one AdamW step at learning rate lr (schedulers live with the caller;
 * max_grad_norm <= 0 = the configured limit); out_grad_norm (DEVICE float, may be null) receives the
 * pre-clipping global norm. */
int lr_lru_train_apply(lr_lru_train_t* h, float lr, float max_grad_norm, float* out_grad_norm,
                       void* hip_stream);
/* hipGraph replay: with enable != 0, lr_lru_train_loss_grad and lr_lru_train_apply capture their launch
 * sequence once per (pointers, B, L) on the caller's stream -- which must not be the default stream -- and
 * replay it afterwards (one graph launch instead of ~120 kernel launches per step). Pass the same device
 * buffers every step to stay on the replay path; any change re-captures. */
int lr_lru_train_set_graph(lr_lru_train_t* h, int32_t enable);
/* The LRU blocks of the step run as row-panel kernels (a 16-row panel of activations in LDS through every product of a
 * block: 14 launches for two blocks instead of 42). enable = 0 selects the first form, one generic GEMM launch per
 * product -- same mathematics, other summation order (the cross-check of tests/test_gpu_lru_train.py). Default 1. */
int lr_lru_train_set_fused(lr_lru_train_t* h, int32_t enable);
/* Deterministic mode (replaces nothing in the reference: torch's own scatter / index_add backward is atomic too,
 * trainer/lru.py:20-28; asked for so that two runs of a step can be compared bit for bit). With enable != 0 every fp32 atomic of
 * the pass -- the loss sum, d x behind the item GEMM, every parameter gradient summed over rows -- adds a 64-bit fixed-point
 * number into a shadow buffer instead (integer addition commutes; csrc/lr_det.h) and the pass folds the shadows back at fixed
 * points; the gradient norm of lr_lru_train_apply is summed by one workgroup. Two passes over the same batch then give the same
 * bits. Needs the row-panel kernels (lr_lru_train_set_fused(h, 1), the default) and a larger workspace: ask
 * lr_lru_train_workspace_bytes AFTER enabling it. One deterministic engine per process at a time. Default 0. */
int lr_lru_train_set_deterministic(lr_lru_train_t* h, int32_t enable);
/* Device pointers of the flat parameter / gradient buffers and their length in floats. */
int lr_lru_train_buffers(lr_lru_train_t* h, float** params, float** grads, size_t* count);
/* Offset and length (floats) of a parameter inside those buffers, by its reference state_dict name,
 * e.g. "model.lru_blocks.1.lru_layer.in_proj.weight" (complex: 2 floats per element). */
int lr_lru_train_param_range(const lr_lru_train_t* h, const char* name, size_t* offset, size_t* count);

/* The step's item GEMM + softmax cross-entropy alone, in each of its three forms (exposed for parity tests):
 *   form 0  stored logits, row-panel kernels (what a step with ce_mode 1 and lr_lru_train_set_fused(h, 1) launches)
 *   form 1  fused, logits never stored       (ce_mode 2)
 *   form 2  stored logits, one generic GEMM launch per product (ce_mode 1 with lr_lru_train_set_fused(h, 0))
 * x [R][64], E [C][64], bias [C] fp32 and labels int64 [R] are DEVICE arrays; label 0 = ignored, labels outside [0, C - 1]
 * are ignored and counted. The call starts as a step does: it counts the labels and zeroes dX [R][64]; dE [C][64] and
 * dbias [C] are ADDED into. out_scal, DEVICE float[4]: the loss SUM over the labelled rows, their count, unused, the number
 * of out-of-range labels. Gradients are those of the MEAN loss. Runs with the deterministic mode off. R >= 1, C >= 2. */
size_t lr_lru_train_ce_parity_workspace_bytes(int32_t form, int32_t R, int32_t C);
int lr_lru_train_ce_parity(int32_t form, const float* x, const float* E, const float* bias, const int64_t* labels,
                           int32_t R, int32_t C, void* workspace, size_t workspace_bytes, float* out_scal, float* dX,
                           float* dE, float* dbias, void* hip_stream);
/* The splits the launcher of a form uses at a shape (host arithmetic only). form 0: out[0..4] = item splits of the score
 * pass, item splits of the d x pass, row parts of the d E pass, 64-item super-blocks, rows padded to 16. form 1:
 * out[0..3] = item chunks, 32-item tiles per chunk, row chunks of the d E pass, 32-row tiles per chunk. form 2: zeros. */
int lr_lru_train_ce_plan(int32_t form, int32_t R, int32_t C, int32_t out[8]);

/* ------------------------------------------------------------------------------------------
 * Ranker LoRA fine-tuning step.
 * Replaces the HF Trainer loop of trainer/llm.py:103-136 over the patched LlamaForCausalLM
 * (model/llm.py:89-127: shifted CrossEntropyLoss on the tokens whose label is not -100; the
 * reference labels only the answer letter and EOS, dataloader/llm.py:55-58) with peft LoRA on
 * q_proj / v_proj (train_ranker.py:71-79, config.py:257-260: r 8, alpha 32, dropout 0.05).
 * Deviations, both documented in DESIGN.md: the frozen base is bf16 (the reference's is NF4 through
 * bitsandbytes, absent here), and the optimizer is plain fp32 AdamW with HF's defaults (the
 * reference's "adamw_bnb_8bit" keeps block-quantised moments).
 *
 * The base handle must hold the UNMERGED base weights. The data-gradient GEMMs run on transposed
 * copies of the frozen matrices (same packed row / column orders), owned by the caller and made
 * once with lr_transpose_bf16.
 * ------------------------------------------------------------------------------------------ */
typedef struct LrLlamaLayerWeightsT {
  const uint16_t* wqkv_t;   /* [hidden][(nh+2*nkv)*hd]  = wqkv^T  */
  const uint16_t* wo_t;     /* [nh*hd][hidden]          = wo^T    */
  const uint16_t* wgu_t;    /* [hidden][2*inter]        = wgu^T   */
  const uint16_t* wdown_t;  /* [inter][hidden]          = wdown^T */
} LrLlamaLayerWeightsT;

typedef struct LrLlamaWeightsTDesc {
  const LrLlamaLayerWeightsT* layers; /* HOST array [num_layers] of device pointers */
  const uint16_t* lm_head_t;          /* [hidden][vocab] = lm_head^T */
} LrLlamaWeightsTDesc;

typedef struct LrLoraTrainConfig {
  int32_t r;            /* config.py:257, 1..16 */
  float alpha;          /* config.py:258; scaling = alpha / r */
  float dropout;        /* config.py:259, on the adapters' input only */
  float beta1, beta2, eps, weight_decay; /* HF TrainingArguments defaults: 0.9, 0.999, 1e-8, 0 */
  uint64_t seed;        /* dropout stream (own counter-based generator) */
} LrLoraTrainConfig;

/* Which Linears of every decoder layer carry an adapter (the reference's --lora_target_modules, config.py:260).
 * modules: bit 0 q_proj, 1 v_proj, 2 k_proj, 3 o_proj, 4 gate_proj, 5 up_proj, 6 down_proj; at least one.
 * Unknown bits or non-zero reserved words: LR_EINVAL. */
typedef struct LrLoraTargets {
  uint32_t modules;
  uint32_t reserved[7];
} LrLoraTargets;

typedef struct lr_llama_lora lr_llama_lora_t;

/* dst[c][r] = src[r][c], bf16, DEVICE pointers. */
int lr_transpose_bf16(const uint16_t* src, int32_t rows, int32_t cols, uint16_t* dst, void* hip_stream);

/* Backward of Qwen3's q/k norm alone (exposed for parity tests), in place on dqk [rows][ld] bf16 DEVICE rows: columns
 * [col0, col0 + (nq + nk) head_dim) hold d loss / d y of the normed, unrotated heads (lr_attention_varlen_bwd_ex's output with a
 * rotary table) and receive d loss / d x. x [rows][ldx]: the pre-norm values of the same heads from column 0 on. Per (row,
 * head), with g = w .* dy and xh = x * rstd: dx = rstd * (g - xh * mean(xh .* g)), fp32 with one rounding; the norm weights are
 * frozen (no weight gradient). One owner per element and no atomics: two runs write the same bits. Arguments as for
 * lr_qk_norm_rope_bf16. */
int lr_qk_norm_bwd_bf16(uint16_t* dqk, int32_t rows, int32_t ld, int32_t col0, const uint16_t* x, int32_t ldx, int32_t nq,
                        int32_t nk, int32_t head_dim, const uint16_t* q_norm, const uint16_t* k_norm, float eps,
                        void* hip_stream);

/* DEVICE bytes for the adapters: fp32 parameters, gradients, Adam moments, bf16 working copies. */
size_t lr_llama_lora_state_bytes(const lr_llama_t* base, const LrLoraTrainConfig* cfg);
/* Gradients, moments and the step counter start at zero; the PARAMETERS are the caller's to fill
 * through lr_llama_lora_buffers (peft: A ~ kaiming-uniform, B = 0). `base` must outlive the handle. */
int lr_llama_lora_create(lr_llama_t* base, const LrLlamaWeightsTDesc* wt, const LrLoraTrainConfig* cfg,
                         void* state_dev, size_t state_bytes, void* hip_stream, lr_llama_lora_t** out);
/* The same two with the adapted modules chosen; targets == NULL means q_proj | v_proj, which is what the
 * two calls above pass. State and workspace grow only with the selected modules. */
size_t lr_llama_lora_state_bytes_ex(const lr_llama_t* base, const LrLoraTrainConfig* cfg, const LrLoraTargets* targets);
int lr_llama_lora_create_ex(lr_llama_t* base, const LrLlamaWeightsTDesc* wt, const LrLoraTrainConfig* cfg,
                            const LrLoraTargets* targets, void* state_dev, size_t state_bytes, void* hip_stream,
                            lr_llama_lora_t** out);
void lr_llama_lora_destroy(lr_llama_lora_t* h);
/* Flat fp32 DEVICE buffers of n floats each. Per layer, in the order q, v, k, o, gate, up, down with the
 * modules the handle does not adapt skipped: lora_A [r][in], lora_B [out][r] -- peft's layouts and HF's
 * (unpermuted) row order; a q|v handle: q_proj.lora_A [r][hidden], q_proj.lora_B [nh*hd][r],
 * v_proj.lora_A [r][hidden], v_proj.lora_B [nkv*hd][r]. Data-parallel training all-reduces `grads`
 * between loss_grad and apply. */
int lr_llama_lora_buffers(lr_llama_lora_t* h, float** params, float** grads, float** m, float** v, size_t* n);
/* which: 0 q_proj, 1 v_proj, 2 k_proj, 3 o_proj, 4 gate_proj, 5 up_proj, 6 down_proj (LR_EINVAL for a module
 * the handle does not adapt); ab: 0 lora_A, 1 lora_B. */
int lr_llama_lora_param_range(const lr_llama_lora_t* h, int32_t layer, int32_t which, int32_t ab,
                              size_t* offset, size_t* count);
size_t lr_llama_lora_workspace_bytes(const lr_llama_lora_t* h, int32_t max_tokens, int32_t max_seqs,
                                     int32_t max_loss_rows);
/* Default 0. With enable != 0 two calls of lr_llama_lora_loss_grad / lr_llama_lora_apply on the same inputs and the same
 * handle state give the same bits, whatever else runs on the device. Ask lr_llama_lora_workspace_bytes AFTER enabling.
 * The mode is a field of the handle and its extra memory a region of the caller's workspace: any number of
 * deterministic and other handles may be in flight at once. No fp32 atomic then decides a value: token reductions
 * store per-chunk partial tiles that one fold sums in chunk order, the loss and the gradient norm are summed in a
 * fixed order, the generic attention backward computes dK / dV per owner. Not promised: the same bits under another
 * grouping of the batch, another LR_TN_CHUNK or another world size. */
int lr_llama_lora_set_deterministic(lr_llama_lora_t* h, int32_t enable);
/* The part of a handle's persistent state that is in no buffer of lr_llama_lora_buffers: the number of
 * lr_llama_lora_apply calls so far (AdamW's bias correction reads it on the device) and the number of
 * lr_llama_lora_loss_grad calls (it selects the dropout streams). Together with params, m and v they are everything
 * a later step depends on: gradients, the bf16 working copies and the scratch scalars are rebuilt by every pass. A
 * handle that is given another handle's params / m / v and progress (same base, config and targets) continues with
 * that handle's bits. reserved: zero. */
typedef struct LrLoraProgress {
  int64_t optimizer_steps;
  int64_t passes;
  int64_t reserved[2];
} LrLoraProgress;
/* get: the values as they stand after everything already queued on hip_stream; copies on that stream and waits for
 * it. set: ordered on hip_stream before later calls, does not wait. LR_EINVAL (with a message) for a null argument
 * and, in set, a negative value, optimizer_steps > INT32_MAX or passes > UINT32_MAX (the handle's counter types) or
 * a non-zero reserved word; the handle is unchanged then. */
int lr_llama_lora_get_progress(lr_llama_lora_t* h, LrLoraProgress* out, void* hip_stream);
int lr_llama_lora_set_progress(lr_llama_lora_t* h, const LrLoraProgress* in, void* hip_stream);
/* One micro-batch: forward over the packed prompts (as lr_llama_prefill_verbalize packs them), loss
 * = mean over the m labelled rows of -log softmax(logits[loss_rows[i]])[loss_targets[i]] (row p of a
 * prompt predicts token p+1: the caller passes the rows whose NEXT token is labelled, each once),
 * backward, gradients * grad_scale ADDED to the gradient buffer (accumulate != 0) or written over it.
 * grad_scale = 1 / gradient_accumulation_steps (HF Trainer). out: DEVICE float[3] = {loss, m,
 * targets outside the vocabulary (ignored, should be 0)}. All pointers DEVICE except cu_seqlens_host. */
int lr_llama_lora_loss_grad(lr_llama_lora_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                            const int32_t* cu_seqlens_host, int32_t B, const int32_t* loss_rows,
                            const int32_t* loss_targets, int32_t m, float grad_scale, int32_t accumulate,
                            float* out, void* workspace, size_t workspace_bytes, void* hip_stream);
/* clip_grad_norm_(max_grad_norm; <= 0: none) + one AdamW step at learning rate lr. out_norm
 * (DEVICE float, optional) = gradient norm before clipping. */
int lr_llama_lora_apply(lr_llama_lora_t* h, float lr, float max_grad_norm, float* out_norm, void* hip_stream);
/* lr_llama_prefill_verbalize with the adapters as they are now (validation during training). */
size_t lr_llama_lora_eval_workspace_bytes(const lr_llama_lora_t* h, int32_t max_tokens, int32_t max_seqs);
int lr_llama_lora_prefill_verbalize(lr_llama_lora_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                                    const int32_t* cu_seqlens_host, int32_t B, const int32_t* label_token_ids,
                                    int32_t C, float* out_scores, void* workspace, size_t workspace_bytes,
                                    void* hip_stream);
/* Varlen causal attention backward (exposed for parity tests): qkv as lr_attention_varlen; out / d_out
 * bf16 [total][nh*hd]; lse fp32 [total][nh] from lr_attention_varlen_lse; dqkv bf16 like qkv.
 * scratch: DEVICE, lr_attention_bwd_scratch_bytes. variant: 0 / 1 / 2 as lr_attention_varlen, 6 = the head_dim-64 MFMA pair
 * (LR_EUNSUPPORTED at any other head_dim; its backward uses only the first, per-(token, head) part of the scratch, whose size
 * is the same for every variant), 8 = the head_dim-96 MFMA pair likewise (LR_EUNSUPPORTED off head_dim 96),
 * 9 = the head_dim-256 MFMA pair likewise (LR_EUNSUPPORTED off head_dim 256); 4, 5 and 7 write no lse and have no backward: LR_EINVAL. */
int lr_attention_varlen_lse(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* cu_seqlens,
                            const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads, int32_t num_kv_heads,
                            int32_t head_dim, int32_t variant, void* hip_stream);
size_t lr_attention_bwd_scratch_bytes(int32_t total, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim);
int lr_attention_varlen_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out, const float* lse,
                            uint16_t* dqkv, const int32_t* cu_seqlens, const int32_t* cu_seqlens_host, int32_t B,
                            int32_t num_heads, int32_t num_kv_heads, int32_t head_dim, int32_t variant,
                            void* scratch, size_t scratch_bytes, void* hip_stream);
/* lr_attention_varlen_bwd with the training step's options (the plain entry is this one with nulls and zeros).
 * rope_cs: DEVICE, the table lr_rope_table wrote for head_dim with rope_positions positions; when given, dqkv is the
 * gradient w.r.t. the UNROTATED q and k (v as before). tok_pos: DEVICE int32[total], required with rope_cs, and must hold
 * each row's position INSIDE ITS PROMPT (row - cu_seqlens[b]): the head_dim-128 MFMA passes index the table by that
 * position directly (so do variant 6's head_dim-64, variant 8's head_dim-96 and variant 9's head_dim-256 passes) and the generic path reads tok_pos, so any other content makes the two disagree. LR_EINVAL (with a
 * message, nothing launched) for rope_cs without tok_pos and for a segment longer than rope_positions.
 * deterministic != 0: the generic path (variant 1) computes dK / dV per owner instead of with fp32 atomics -- the same
 * bits on every run; the MFMA passes (variants 2, 6, 8 and 9) have no atomics either way and ignore the flag. */
int lr_attention_varlen_bwd_ex(const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out, const float* lse,
                               uint16_t* dqkv, const int32_t* cu_seqlens, const int32_t* cu_seqlens_host, int32_t B,
                               int32_t num_heads, int32_t num_kv_heads, int32_t head_dim, int32_t variant,
                               void* scratch, size_t scratch_bytes, const int32_t* tok_pos, const float* rope_cs,
                               int32_t rope_positions, int32_t deterministic, void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * The LoRA step's small kernels alone (exposed for parity tests): the row sweeps, rank-r products, token reductions, loss
 * head and optimizer that lr_llama_lora_loss_grad / lr_llama_lora_apply run between their GEMMs and attention passes, each
 * behind one call with flat arguments. All pointers DEVICE, bf16 as uint16_t, r = the adapter's rank (1..16; the bf16
 * working copies are zero-padded to 16 rows / columns). Every call checks on the host, before it launches anything, what
 * its kernel assumes about the arguments: LR_EINVAL (null pointer, negative count, a tile past the row stride, r, layout,
 * dropout outside [0, 1)) or LR_EUNSUPPORTED (a width the kernel has no path for, a pointer that is not 16-byte aligned
 * where the kernel moves 16 bytes at a time), with a message in lr_last_error and nothing written. What only the device can
 * see is the caller's promise: out_rows names distinct rows inside the output, targets may be anything (a value outside
 * [0, vocab) is "no token id"). A count of zero rows is LR_OK and launches nothing. drop_stream / drop_p: the counter-based
 * dropout mask keep(stream, row, col) of the step (kept elements are scaled by 1 / (1 - p) and rounded to bf16); p = 0: none.
 * The arithmetic, rounding points and element-wise error bounds of every call: tests/lora_kernels_ref.py.
 * ------------------------------------------------------------------------------------------ */
/* out[row][ocol + 16 t + j] = bf16(scale * sum_k drop(x)[row][k] * w[16 t + j][k]), t < nt (1 or 2): x [n][ldx], w [16 nt][K],
 * K a multiple of 64, out [n][ldo]. */
int lr_lora_skinny_bf16(const uint16_t* x, int32_t ldx, int32_t n, int32_t k, const uint16_t* w, int32_t nt, uint16_t* out,
                        int32_t ldo, int32_t ocol, float scale, uint32_t drop_stream, float drop_p, void* hip_stream);
/* Token reduction, ADDED to fp32 outputs: out_a[..] += scale * sum_tok t[tok][tcol + 16 a + j] * drop(x)[tok][c], a < nj (1 or
 * 2), j < r, c < cols (a multiple of 64). layout 0: out_a[j * cols + c]; 1: out0[c * r + j]; 2: out0[orig(c) * r + j] with the
 * rotary pair interleave of head_dim-wide heads undone; 3 (nj = 2): x = the interleaved gate / up gradient (16 gate columns,
 * 16 up columns, ...), tile 0 keeps the gate columns in out0[f_col * r + j], tile 1 the up columns in out1, either may be
 * null. det_part null: one fp32 atomic per element and token chunk. det_part given (16-byte aligned like the outputs then,
 * det_part_floats >= lr_lora_tn_det_floats(...), else LR_EWORKSPACE): per-chunk partial tiles stored there and folded in
 * chunk order, the same bits on every run. Rows of x and t that are 16-byte aligned take the LDS-staged kernel, any other
 * alignment the 2-byte gather kernel; the two give the same bits. */
size_t lr_lora_tn_det_floats(int32_t nj, int32_t n, int32_t cols, int32_t r, int32_t layout);
int lr_lora_tn_f32(int32_t nj, const uint16_t* t, int32_t ldt, int32_t tcol, const uint16_t* x, int32_t ldx, int32_t n,
                   int32_t cols, float scale, float* out0, float* out1, int32_t r, int32_t layout, int32_t head_dim,
                   uint32_t drop_stream, float drop_p, float* det_part, size_t det_part_floats, void* hip_stream);
/* y[row][c] = bf16(y + bf16(bf16(sum_j t[row][tcol + j] * w[j][c]) * s)) where keep(row, c), else unchanged: y [n][ldy] in
 * place, cols a multiple of 8, t [n][ldt] (16 columns from tcol), w [16][cols]. */
int lr_lora_expand_bf16(uint16_t* y, int32_t ldy, int32_t n, int32_t cols, const uint16_t* t, int32_t ldt, int32_t tcol,
                        const uint16_t* w, int32_t r, float s, uint32_t drop_stream, float drop_p, void* hip_stream);
/* SwiGLU on the interleaved gate / up layout gu [n][2f] (16 gate columns, 16 up columns, ...), f a multiple of 16:
 * h [n][f] = bf16(silu(gate) * up); the backward rewrites gu in place into (d gate, d up) given dh [n][f]. */
int lr_swiglu_fwd_bf16(const uint16_t* gu, uint16_t* h, int32_t n, int32_t f, void* hip_stream);
int lr_swiglu_bwd_bf16(uint16_t* gu, const uint16_t* dh, int32_t n, int32_t f, void* hip_stream);
/* RMSNorm backward over dense [rows][d] rows (d a multiple of 8, <= 8192): out[out_rows ? out_rows[i] : i] = (res ? res[i] :
 * 0) + dx[i], dx = rstd g - x rstd^3 mean(x g), g = w dy. dt non-null: dy first gets the adapters' term,
 * dy = bf16(dy + bf16(ds * sum_j dt[i][j] a_cat[j][c] + dt[i][16 + j] a_cat[16 + j][c])) where keep(i, c): dt [rows][ldt]
 * (32 columns used), a_cat [32][d]. */
int lr_rmsnorm_bwd_bf16(const uint16_t* dy, const uint16_t* x, const uint16_t* w, const uint16_t* res, uint16_t* out,
                        int32_t rows, int32_t d, float eps, const int32_t* out_rows, const uint16_t* dt, int32_t ldt,
                        const uint16_t* a_cat, int32_t r, uint32_t drop_stream, float drop_p, void* hip_stream);
/* Softmax cross-entropy over logits [m][vocab], rewritten in place into (softmax - onehot) * gscale; a row whose target is
 * outside [0, vocab) becomes zeros. out[0] = sum of the rows' -log p(target) / m, out[1] = m, out[2] = rows without a token
 * id. scal: scratch of 2 floats, or 2 + m with deterministic != 0 (the losses summed in row order). m = 0 still writes
 * out = {0, 0, 0}. */
int lr_ce_bf16(uint16_t* logits, int32_t m, int32_t vocab, const int32_t* targets, float gscale, float* scal, float* out,
               int32_t deterministic, void* hip_stream);
/* out[row * num_heads + h] = sum_d o[row][h][d] * d_o[row][h][d], fp32; head_dim a multiple of 8. */
int lr_rowdot_bf16(const uint16_t* o, const uint16_t* d_o, int32_t n, int32_t num_heads, int32_t head_dim, float* out,
                   void* hip_stream);
/* The forward sweep behind the q|k|v projection, in place on qkv [n][qw] (q columns [0, qcols), k [qcols, qcols + kcols), v the
 * rest; packed, pair-interleaved heads): q and v get their adapters' delta bf16(bf16(sum_j t[row][j (+16)] b[j][c]) * scaling)
 * (t [n][32]: 16 q ranks, 16 v ranks; bq_t [16][qcols], bv_t [16][vcols]), k too when bk_t is given (its ranks from tk [n][ldtk],
 * column tkcol; bk_t [16][kcols]); then, when q_norm is given, every q / k head its RMSNorm over head_dim (a power of two from
 * 16 to 256; weights [head_dim] in packed order; the pre-norm q | k values go to xsave [n][qcols + kcols]); then the rotation
 * of q and k at rope_cs[tok_pos[row]] (lr_rope_table's fp32 part). tk / bk_t null: no k adapter. q_norm, k_norm and xsave all
 * null: no norm. */
int lr_lora_rope_fwd_bf16(uint16_t* qkv, int32_t n, int32_t qw, int32_t qcols, int32_t kcols, int32_t head_dim, const uint16_t* t,
                          const uint16_t* bq_t, const uint16_t* bv_t, int32_t r, float scaling, const int32_t* tok_pos,
                          const float* rope_cs, const uint16_t* tk, int32_t ldtk, int32_t tkcol, const uint16_t* bk_t,
                          const uint16_t* q_norm, const uint16_t* k_norm, float eps, uint16_t* xsave, void* hip_stream);
/* The transpose of that rotation, in place on the first rot_cols columns of dqkv [n][qw] (head_dim a multiple of 8 dividing
 * rot_cols). */
int lr_rope_bwd_bf16(uint16_t* dqkv, int32_t n, int32_t qw, int32_t rot_cols, int32_t head_dim, const int32_t* tok_pos,
                     const float* rope_cs, void* hip_stream);
/* lr_swiglu_fwd_bf16 with the gate / up adapters' delta: gu += bf16(bf16(t w) * s) (t [n][ldt] from column tcol: 16 gate ranks,
 * 16 up ranks; w [32][2f]: their B^T in gu's interleaved column order), the sum written back to gu, h = swiglu of the sum. */
int lr_swiglu_lora_fwd_bf16(uint16_t* gu, uint16_t* h, int32_t n, int32_t f, const uint16_t* t, int32_t ldt, int32_t tcol,
                            const uint16_t* w, int32_t r, float s, void* hip_stream);
/* The bf16 working copies of fp32 masters (peft's lora_A [r][in], lora_B [out][r]), zero-padded to 16 rows. q|v pair: a_cat
 * [32][d] (rows 0.. = A_q, 16.. = A_v), bq_t [16][qcols] = B_q^T in the packed (pair-interleaved) column order, bv_t [16][vcols]
 * = B_v^T. One module: a_w [16][in], b_t [16][ldb] = B^T with perm 0 plain, 1 the pair interleave within heads of head_dim, 2 / 3
 * the gate / up columns of the interleaved gate-up layout (ldb >= 2 out; the other half's columns are not written). */
int lr_lora_prep_bf16(const float* aq, const float* bq, const float* av, const float* bv, int32_t r, int32_t d, int32_t qcols,
                      int32_t vcols, int32_t head_dim, uint16_t* a_cat, uint16_t* bq_t, uint16_t* bv_t, void* hip_stream);
int lr_lora_prep_module_bf16(const float* a, const float* b, int32_t r, int32_t in, int32_t out, int32_t perm, int32_t head_dim,
                             uint16_t* a_w, uint16_t* b_t, int32_t ldb, void* hip_stream);
/* clip_grad_norm_(max_grad_norm; <= 0: none) and one AdamW step over n fp32 elements at step ctr[0] + 1; ctr[0] is then
 * incremented. scratch: 4 floats. g is read only. out_norm (optional) = the norm before clipping. deterministic != 0: the
 * norm summed in an order fixed by n (g 16-byte aligned). n = 0 is LR_OK, launches nothing and is no step: ctr[0], scratch
 * and out_norm keep what they held. */
int lr_lora_adamw_f32(float* p, float* g, float* m, float* v, size_t n, float* scratch, int32_t* ctr, float lr,
                      float max_grad_norm, float beta1, float beta2, float eps, float weight_decay, float* out_norm,
                      int32_t deterministic, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LLAMAREC_MI355X_H */
