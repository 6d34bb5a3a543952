// api_llama_train.hip -- C ABI of the ranker's LoRA training step (declared in include/llamarec_mi355x.h,
// SURVEY.md 8(f) #4): forward with the adapters live (not merged), shifted cross-entropy on the labelled rows,
// backward through the frozen bf16 base to the LoRA matrices, clipping + AdamW.
//
// Replaces trainer/llm.py:103-136 (HF Trainer.train over the patched LlamaForCausalLM, model/llm.py:89-127, with
// peft LoRA on q_proj / v_proj, train_ranker.py:71-79). Data-gradient GEMMs reuse the forward's NT kernel on
// TRANSPOSED copies of the frozen weights (caller-owned, made once with lr_transpose_bf16): 13.5 GB more for
// Llama-2-7b, nothing against 288 GB, and the backward then runs at the forward's GEMM rate. Every activation the
// backward needs is kept (~100 KB per token and layer): no recomputation (the reference checkpoints, config.py:269,
// because its cards are 24-80 GB).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "llama_train.h"

typedef unsigned short u16;

struct lr_llama_lora {
  lr_llama* base;
  LrLoraTrainConfig cfg;
  LrLlamaLayerWeightsT* layers_t;  // host array
  const u16* lm_head_t;
  float *params, *grads, *m, *v;   // flat fp32 device buffers, n_params each
  size_t n_params, per_layer;
  u16* work;                       // bf16 working copies, work_per_layer elements per layer
  size_t work_per_layer;
  float* scratch;                  // [8]: 0 loss sum, 1 bad targets, 2 sumsq, 3 lr, 4 limit
  int* ctr;                        // [4]: 0 optimizer steps
  uint32_t pass;                   // host-side pass counter (dropout streams)
  int qcols, kcols, vcols;
  // adapted modules (LrLoraTargets bits: 0 q, 1 v, 2 k, 3 o, 4 gate, 5 up, 6 down). q|v is the layout and the code path
  // this step always had; every other module goes through the generic rank-r passes (LoraMods below)
  uint32_t mods;
  // The adapter-only kernels (rank-r products, dA / dB reductions: ~5 % of a step, a few hundred workgroups each) run
  // on a low-priority side stream next to the big GEMM they are independent of, and fill the CUs its last, partly
  // empty round of tiles leaves idle (7 k tokens: 448 tiles on 256 CUs). LR_LORA_OVERLAP=0 keeps everything in order.
  hipStream_t side;
  hipEvent_t ev_fork, ev_join;
  // lr_llama_lora_set_deterministic: a field of the handle, read on the host when a call is issued and handed to the launchers
  // as arguments; the mode's extra memory (LoraWs::det_loss, det_part) is carved from the caller's workspace
  int deterministic;
};

static int fork_side(lr_llama_lora* h, hipStream_t main, hipStream_t* work) {
  *work = main;
  if (!h->side) return LR_OK;
  LR_CHECK_HIP(hipEventRecord(h->ev_fork, main));
  LR_CHECK_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
  *work = h->side;
  return LR_OK;
}
static int join_side(lr_llama_lora* h, hipStream_t main) {
  if (!h->side) return LR_OK;
  LR_CHECK_HIP(hipEventRecord(h->ev_join, h->side));
  LR_CHECK_HIP(hipStreamWaitEvent(main, h->ev_join, 0));
  return LR_OK;
}

#define LT_MOD_QV 3u
#define LT_MOD_ALL 0x7fu
enum { MQ = 0, MV, MK, MO, MGATE, MUP, MDOWN, LT_NMOD };
// Where every selected module lives: fp32 masters per layer in the order q, v, k, o, gate, up, down with absent modules
// skipped (A [r][in] then B [out][r]); bf16 working copies per layer = the q/v block of always (a_cat, bq_t, bv_t) followed
// by the extra modules' (a_w [LT_RP][in], b_t [LT_RP][out]; gate and up share a [2*LT_RP][d] / [2*LT_RP][2f] pair so that one
// 32-column product serves both); t columns of the extra modules in the saved [n][tw] tile (gate and up adjacent).
struct LoraMods {
  uint32_t mask;
  int in[LT_NMOD], out[LT_NMOD];
  size_t pa[LT_NMOD], pb[LT_NMOD];  // fp32 offsets within a layer's parameters
  size_t per_layer;
  size_t wk_a, wk_b, wo_a, wo_b, wgu_a, wgu_b, wdn_a, wdn_b, work_per_layer;  // bf16 element offsets
  int tk, to, tgu, tdn, tw;         // t column offsets of the extra modules, tw = their total width (0: none)
  bool has(int m) const { return (mask >> m) & 1u; }
  bool gu() const { return has(MGATE) || has(MUP); }
};
static LoraMods lora_mods(const LrLlamaConfig& c, int r, uint32_t mask) {
  LoraMods m;
  memset(&m, 0, sizeof(m));
  m.mask = mask;
  const int d = c.hidden_size, f = c.intermediate_size, qc = c.num_heads * c.head_dim, kv = c.num_kv_heads * c.head_dim;
  const int in[LT_NMOD] = {d, d, d, qc, d, d, f}, out[LT_NMOD] = {qc, kv, kv, d, f, f, d};
  size_t o = 0;
  for (int i = 0; i < LT_NMOD; ++i) {
    m.in[i] = in[i];
    m.out[i] = out[i];
    if (!m.has(i)) continue;
    m.pa[i] = o;
    o += (size_t)r * in[i];
    m.pb[i] = o;
    o += (size_t)r * out[i];
  }
  m.per_layer = o;
  size_t w = 2 * (size_t)LT_RP * d + (size_t)LT_RP * (qc + kv);
  int t = 0;
  auto take = [&](size_t n) {
    size_t at = w;
    w += n;
    return at;
  };
  m.tk = m.to = m.tgu = m.tdn = -1;
  if (m.has(MK)) m.wk_a = take((size_t)LT_RP * d), m.wk_b = take((size_t)LT_RP * kv), m.tk = t, t += LT_RP;
  if (m.has(MO)) m.wo_a = take((size_t)LT_RP * qc), m.wo_b = take((size_t)LT_RP * d), m.to = t, t += LT_RP;
  if (m.gu()) m.wgu_a = take(2 * (size_t)LT_RP * d), m.wgu_b = take(2 * (size_t)LT_RP * 2 * f), m.tgu = t, t += 2 * LT_RP;
  if (m.has(MDOWN)) m.wdn_a = take((size_t)LT_RP * f), m.wdn_b = take((size_t)LT_RP * d), m.tdn = t, t += LT_RP;
  m.work_per_layer = w;
  m.tw = t;
  return m;
}

struct LoraStateLayout {
  size_t params, grads, m, v, work, scratch, ctr, total;
};
static LoraStateLayout state_layout(const LrLlamaConfig& c, int r, uint32_t mask) {
  LoraStateLayout s;
  const LoraMods md = lora_mods(c, r, mask);
  const size_t n = (size_t)c.num_layers * md.per_layer;
  const size_t wl = md.work_per_layer;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += lr_align_up(bytes, 256);
    return at;
  };
  s.params = take(n * 4);
  s.grads = take(n * 4);
  s.m = take(n * 4);
  s.v = take(n * 4);
  s.work = take((size_t)c.num_layers * wl * 2);
  s.scratch = take(8 * 4);
  s.ctr = take(4 * 4);
  s.total = o;
  return s;
}

static int check_cfg(const lr_llama_t* base, const LrLoraTrainConfig* cfg, const char* who) {
  if (!base || !cfg) LR_FAIL(LR_EINVAL, "%s: null argument", who);
  if (cfg->r < 1 || cfg->r > LT_RP) LR_FAIL(LR_EUNSUPPORTED, "%s: LoRA rank %d outside [1, %d]", who, cfg->r, LT_RP);
  if (cfg->dropout < 0.f || cfg->dropout >= 1.f) LR_FAIL(LR_EINVAL, "%s: dropout outside [0, 1)", who);
  const LrLlamaConfig& c = base->cfg;
  if (c.hidden_size % 64 != 0 || (c.num_heads * c.head_dim) % 64 != 0 || (c.num_kv_heads * c.head_dim) % 64 != 0)
    LR_FAIL(LR_EUNSUPPORTED, "%s: hidden size and q / v widths must be multiples of 64", who);
  if (c.head_dim % 8 != 0) LR_FAIL(LR_EUNSUPPORTED, "%s: head_dim %d (must be a multiple of 8)", who, c.head_dim);
  return LR_OK;
}
// NULL = q_proj | v_proj
static int check_targets(const lr_llama_t* base, const LrLoraTargets* t, const char* who, uint32_t* mask) {
  *mask = LT_MOD_QV;
  if (!t) return LR_OK;
  for (int i = 0; i < 7; ++i)
    if (t->reserved[i]) LR_FAIL(LR_EINVAL, "%s: LrLoraTargets.reserved[%d] is not zero", who, i);
  if (t->modules == 0 || (t->modules & ~LT_MOD_ALL))
    LR_FAIL(LR_EINVAL, "%s: LrLoraTargets.modules = 0x%x (bits 0..6, at least one)", who, t->modules);
  if ((t->modules & 0x70u) && base->cfg.intermediate_size % 64 != 0)
    LR_FAIL(LR_EUNSUPPORTED, "%s: adapters on gate / up / down need an intermediate size that is a multiple of 64 (%d)", who,
            base->cfg.intermediate_size);
  *mask = t->modules;
  return LR_OK;
}

extern "C" size_t lr_llama_lora_state_bytes_ex(const lr_llama_t* base, const LrLoraTrainConfig* cfg,
                                               const LrLoraTargets* targets) {
  uint32_t mask;
  if (check_cfg(base, cfg, "lr_llama_lora_state_bytes") || check_targets(base, targets, "lr_llama_lora_state_bytes", &mask))
    return 0;
  return state_layout(base->cfg, cfg->r, mask).total;
}
extern "C" size_t lr_llama_lora_state_bytes(const lr_llama_t* base, const LrLoraTrainConfig* cfg) {
  return lr_llama_lora_state_bytes_ex(base, cfg, nullptr);
}

extern "C" int lr_llama_lora_create(lr_llama_t* base, const LrLlamaWeightsTDesc* wt, const LrLoraTrainConfig* cfg,
                                    void* state, size_t state_bytes, void* hip_stream, lr_llama_lora_t** out) {
  return lr_llama_lora_create_ex(base, wt, cfg, nullptr, state, state_bytes, hip_stream, out);
}
extern "C" int lr_llama_lora_create_ex(lr_llama_t* base, const LrLlamaWeightsTDesc* wt, const LrLoraTrainConfig* cfg,
                                       const LrLoraTargets* targets, void* state, size_t state_bytes, void* hip_stream,
                                       lr_llama_lora_t** out) {
  int rc = check_cfg(base, cfg, "lr_llama_lora_create");
  if (rc) return rc;
  uint32_t mask;
  rc = check_targets(base, targets, "lr_llama_lora_create", &mask);
  if (rc) return rc;
  if (base->arch.norm_style != 0 || base->arch.mlp_act != 0 || base->arch.embed_scale != 1.0f)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_lora_create: fine-tuning needs a Llama base (no GeGLU / Gemma-norm backward)");
  if (base->gemma2)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_lora_create: fine-tuning needs a Llama base (no soft-cap / sandwich-norm backward)");
  if (base->gemma3)
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_lora_create: fine-tuning needs a Llama base (no sliding-window / sandwich-norm backward)");
  if (base->bqkv)   // the live-adapter forward adds its delta and rotates in lr_launch_lora_rope_fwd, which knows no bias
    LR_FAIL(LR_EUNSUPPORTED, "lr_llama_lora_create: fine-tuning needs a base without q/k/v biases (lr_llama_set_qkv_bias)");
  if (!wt || !wt->layers || !wt->lm_head_t || !state || !out) LR_FAIL(LR_EINVAL, "lr_llama_lora_create: null argument");
  const LrLlamaConfig& c = base->cfg;
  for (int l = 0; l < c.num_layers; ++l) {
    const LrLlamaLayerWeightsT& t = wt->layers[l];
    if (!t.wqkv_t || !t.wo_t || !t.wgu_t || !t.wdown_t)
      LR_FAIL(LR_EINVAL, "lr_llama_lora_create: layer %d has a null transposed weight", l);
  }
  const LoraStateLayout s = state_layout(c, cfg->r, mask);
  const LoraMods md = lora_mods(c, cfg->r, mask);
  if (state_bytes < s.total)
    LR_FAIL(LR_EWORKSPACE, "lr_llama_lora_create: state needs %zu bytes, have %zu", s.total, state_bytes);
  lr_llama_lora* h = (lr_llama_lora*)calloc(1, sizeof(lr_llama_lora));
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_lora_create: out of host memory");
  h->base = base;
  h->cfg = *cfg;
  h->layers_t = (LrLlamaLayerWeightsT*)malloc(sizeof(LrLlamaLayerWeightsT) * c.num_layers);
  memcpy(h->layers_t, wt->layers, sizeof(LrLlamaLayerWeightsT) * c.num_layers);
  h->lm_head_t = wt->lm_head_t;
  char* b = (char*)state;
  h->params = (float*)(b + s.params);
  h->grads = (float*)(b + s.grads);
  h->m = (float*)(b + s.m);
  h->v = (float*)(b + s.v);
  h->work = (u16*)(b + s.work);
  h->scratch = (float*)(b + s.scratch);
  h->ctr = (int*)(b + s.ctr);
  h->qcols = c.num_heads * c.head_dim;
  h->kcols = h->vcols = c.num_kv_heads * c.head_dim;
  h->mods = mask;
  h->per_layer = md.per_layer;
  h->n_params = (size_t)c.num_layers * h->per_layer;
  h->work_per_layer = md.work_per_layer;
  const char* ov = getenv("LR_LORA_OVERLAP");
  if (!ov || ov[0] != '0') {
    // NORMAL priority (round 5). The side stream used to be created with the device's lowest priority, so that the rank-r products
    // never took a CU from the GEMM they run beside. But a lowest-priority stream -- alive or destroyed -- makes this HIP runtime
    // map some LATER normal-priority streams of the process onto its hardware queue: every third or fourth torch stream created
    // afterwards ran the same captured graph 2-3 x slower (tools/diag/stream_index_probe.py: 0.50 -> 0.94-1.56 ms; a normal-priority
    // stream has no such effect). LR_LORA_SIDE_PRIORITY=low restores the old behaviour for A/B runs.
    int lo = 0, hi = 0, prio = 0;
    const char* sp = getenv("LR_LORA_SIDE_PRIORITY");
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
        hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, (sp && sp[0] == 'l') ? lo : prio) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
      free(h->layers_t);
      free(h);
      LR_FAIL(LR_EHIP, "lr_llama_lora_create: side stream / events");
    }
  }
  // parameters are the caller's to fill (lr_llama_lora_buffers); gradients, moments and counters start at zero
  hipStream_t st = (hipStream_t)hip_stream;
  if (hipMemsetAsync(b + s.grads, 0, s.total - s.grads, st) != hipSuccess) {
    free(h->layers_t);
    free(h);
    LR_FAIL(LR_EHIP, "lr_llama_lora_create: hipMemsetAsync failed");
  }
  *out = h;
  return LR_OK;
}

extern "C" void lr_llama_lora_destroy(lr_llama_lora_t* h) {
  if (!h) return;
  if (h->side) {
    (void)hipStreamSynchronize(h->side);
    (void)hipEventDestroy(h->ev_fork);
    (void)hipEventDestroy(h->ev_join);
    (void)hipStreamDestroy(h->side);
  }
  free(h->layers_t);
  free(h);
}

extern "C" int lr_llama_lora_buffers(lr_llama_lora_t* h, float** params, float** grads, float** m, float** v,
                                     size_t* n) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_lora_buffers: null handle");
  if (params) *params = h->params;
  if (grads) *grads = h->grads;
  if (m) *m = h->m;
  if (v) *v = h->v;
  if (n) *n = h->n_params;
  return LR_OK;
}

// which: 0 q_proj, 1 v_proj, 2 k_proj, 3 o_proj, 4 gate_proj, 5 up_proj, 6 down_proj; ab: 0 lora_A [r][in], 1 lora_B [out][r]
// (peft's layouts)
extern "C" int lr_llama_lora_param_range(const lr_llama_lora_t* h, int32_t layer, int32_t which, int32_t ab,
                                         size_t* offset, size_t* count) {
  if (!h || !offset || !count) LR_FAIL(LR_EINVAL, "lr_llama_lora_param_range: null argument");
  const LrLlamaConfig& c = h->base->cfg;
  if (layer < 0 || layer >= c.num_layers || which < 0 || which >= LT_NMOD || ab < 0 || ab > 1)
    LR_FAIL(LR_EINVAL, "lr_llama_lora_param_range: layer=%d which=%d ab=%d", layer, which, ab);
  const LoraMods md = lora_mods(c, h->cfg.r, h->mods);
  if (!md.has(which)) LR_FAIL(LR_EINVAL, "lr_llama_lora_param_range: module %d is not adapted by this handle", which);
  *offset = (size_t)layer * h->per_layer + (ab ? md.pb[which] : md.pa[which]);
  *count = (size_t)h->cfg.r * (ab ? md.out[which] : md.in[which]);
  return LR_OK;
}

// ---- workspace -----------------------------------------------------------------------------------------------
struct LoraLayerSave {
  u16 *x, *xn, *qkv, *att, *xmid, *gu, *t;
  float* lse;
  u16* t2;  // [n][tw]: drop(input) A^T of the extra modules
  u16* xqk; // [n][(nh + nkv) hd]: the pre-norm q | k values, delta included (a base with q/k norms only, else null)
};
struct LoraWs {
  int32_t *tok_pos, *last_rows;
  float* rope;
  u16 *x_final, *xn2, *hmid;              // forward transients (xn2/hmid alias backward transients)
  u16 *dx, *dh, *dxn, *datt, *dqkv, *dt;  // backward
  float *dsum, *dkv32;
  u16 *xg, *hn, *logits, *dhn;            // loss head, m rows
  u16 *dt2, *xn2_b, *hmid_b;              // extra modules' backward: d t [n][tw]; recomputed inputs of gate/up and of down
  // deterministic mode only (null otherwise). det_loss [2 + m]: rows without a token id, per-row losses. det_part: the token
  // reductions' per-chunk partial tiles, sized for the largest of them. ONE region serves them all: every token reduction of a
  // call is issued on one stream (the side stream, or the caller's without one), which runs partials, fold, next partials in
  // order; the main stream never touches the region.
  float *det_loss, *det_part;
  size_t o_t2, o_xqk;
  bool qk_norm;
  size_t save0, save_stride;              // per-layer saved activations: base + l * save_stride
  size_t o_x, o_xn, o_qkv, o_att, o_xmid, o_gu, o_t, o_lse;
  char* base;
  size_t total;
};
static LoraWs carve(const LrLlamaConfig& c, const LoraMods& md, int n_tok, int B, int m, int slots, bool training,
                    char* base, int r = 0, bool deterministic = false, bool qk_norm = false) {
  LoraWs w;
  memset(&w, 0, sizeof(w));
  w.base = base;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += lr_align_up(bytes, 256);
    return at;
  };
  const size_t n = (size_t)n_tok, d = c.hidden_size, f = c.intermediate_size;
  const size_t qcols = (size_t)c.num_heads * c.head_dim, kv = (size_t)c.num_kv_heads * c.head_dim;
  const size_t qw = qcols + 2 * kv;
  w.tok_pos = (int32_t*)(base + take(n * 4));
  w.last_rows = (int32_t*)(base + take((size_t)(B > 0 ? B : 1) * 4));
  // built per pass for its longest prompt, which has at most n_tok rows (max_positions is 131 072 in a Llama-3.1 / 3.2 config)
  w.rope = (float*)(base + take((c.max_positions < n_tok ? (size_t)c.max_positions : n) * (c.head_dim / 2) * 2 * sizeof(float)));
  w.x_final = (u16*)(base + take(n * d * 2));
  // one slot of saved activations
  size_t so = 0;
  auto stake = [&](size_t bytes) {
    size_t at = so;
    so += lr_align_up(bytes, 256);
    return at;
  };
  w.o_x = stake(n * d * 2);
  w.o_xn = stake(n * d * 2);
  w.o_qkv = stake(n * qw * 2);
  w.o_att = stake(n * qcols * 2);
  w.o_xmid = stake(n * d * 2);
  w.o_gu = stake(n * 2 * f * 2);
  w.o_t = stake(n * 2 * LT_RP * 2);
  w.o_lse = stake(n * c.num_heads * 4);
  w.o_t2 = stake(n * md.tw * 2);
  // behind everything else and empty without q/k norms: such a handle keeps its layout and sizes to the byte
  w.qk_norm = qk_norm;
  w.o_xqk = stake(qk_norm ? n * (qcols + kv) * 2 : 0);
  w.save_stride = so;
  w.save0 = take(so * (size_t)slots);
  // transients: forward's (xn2, hmid) share memory with backward's (dxn, dh)
  w.xn2 = w.dxn = (u16*)(base + take(n * d * 2));
  w.hmid = w.dh = (u16*)(base + take(n * f * 2));
  if (training) {
    w.dx = (u16*)(base + take(n * d * 2));
    w.datt = (u16*)(base + take(n * qcols * 2));
    w.dqkv = (u16*)(base + take(n * qw * 2));
    w.dt = (u16*)(base + take(n * 2 * LT_RP * 2));
    w.dsum = (float*)(base + take(n * c.num_heads * 4));
    w.dkv32 = c.head_dim == 128 ? nullptr : (float*)(base + take(n * 2 * kv * 4));
    const size_t mm = (size_t)(m > 0 ? m : 1);
    w.xg = (u16*)(base + take(mm * d * 2));
    w.hn = (u16*)(base + take(mm * d * 2));
    w.logits = (u16*)(base + take(mm * c.vocab_size * 2));
    w.dhn = (u16*)(base + take(mm * d * 2));
    // The inputs of gate/up (xn2) and down (hmid) live in shared forward transients: the backward recomputes them (one rmsnorm /
    // swiglu pass per layer on the side stream) instead of saving n * (d + f) more bytes per layer
    if (md.tw) w.dt2 = (u16*)(base + take(n * md.tw * 2));
    if (md.gu()) w.xn2_b = (u16*)(base + take(n * d * 2));
    if (md.has(MDOWN)) w.hmid_b = (u16*)(base + take(n * f * 2));
    if (deterministic) {
      w.det_loss = (float*)(base + take((2 + mm) * 4));
      // the shapes loss_grad hands to lr_launch_lora_tn / _db / _da: (tiles, columns, layout)
      const int dd = (int)d, ff = (int)f;
      size_t part = 0;
      auto shape = [&](bool on, int nj, int cols, int layout) {
        const size_t need = on ? lr_lora_tn_partial_floats(nj, n_tok, cols, r, layout) : 0;
        if (need > part) part = need;
      };
      shape(md.has(MQ), 1, (int)qcols, 2), shape(md.has(MV) || md.has(MK), 1, (int)kv, 1);
      shape(md.has(MQ) || md.has(MV), 2, dd, 0), shape(md.has(MK) || md.has(MDOWN) || md.has(MO), 1, dd, 0);
      shape(md.has(MO), 1, (int)qcols, 0);
      shape(md.gu(), 2, 2 * ff, 3), shape(md.gu(), 2, dd, 0), shape(md.has(MDOWN), 1, ff, 0);
      w.det_part = (float*)(base + take(part * 4));
    }
  }
  w.total = o;
  return w;
}
static LoraLayerSave slot(const LoraWs& w, int l) {
  char* b = w.base + w.save0 + (size_t)l * w.save_stride;
  LoraLayerSave s;
  s.x = (u16*)(b + w.o_x);
  s.xn = (u16*)(b + w.o_xn);
  s.qkv = (u16*)(b + w.o_qkv);
  s.att = (u16*)(b + w.o_att);
  s.xmid = (u16*)(b + w.o_xmid);
  s.gu = (u16*)(b + w.o_gu);
  s.t = (u16*)(b + w.o_t);
  s.lse = (float*)(b + w.o_lse);
  s.t2 = (u16*)(b + w.o_t2);
  s.xqk = w.qk_norm ? (u16*)(b + w.o_xqk) : nullptr;
  return s;
}

extern "C" size_t lr_llama_lora_workspace_bytes(const lr_llama_lora_t* h, int32_t max_tokens, int32_t max_seqs,
                                                int32_t max_loss_rows) {
  if (!h || max_tokens < 1) return 0;
  if (max_seqs < 1) max_seqs = 1;
  const LrLlamaConfig& c = h->base->cfg;
  return carve(c, lora_mods(c, h->cfg.r, h->mods), max_tokens, max_seqs, max_loss_rows, c.num_layers, true, nullptr, h->cfg.r,
               h->deterministic != 0, h->base->q_norm != nullptr).total;
}
extern "C" int lr_llama_lora_set_deterministic(lr_llama_lora_t* h, int32_t enable) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_lora_set_deterministic: null handle");
  h->deterministic = enable != 0;
  return LR_OK;
}
// The two counters of a handle that sit in no buffer of lr_llama_lora_buffers: ctr[0] on the device (lt_adamw_kernel's bias
// correction) and the host's pass counter (the dropout streams). Everything else a trajectory depends on is params / m / v;
// grads, the bf16 working copies and the scratch scalars are rebuilt by every pass.
static int check_progress(const lr_llama_lora* h, const LrLoraProgress* p, const char* who) {
  if (!h || !p) LR_FAIL(LR_EINVAL, "%s: null argument", who);
  return LR_OK;
}
extern "C" int lr_llama_lora_get_progress(lr_llama_lora_t* h, LrLoraProgress* out, void* hip_stream) {
  LR_RUN(check_progress(h, out, "lr_llama_lora_get_progress"));
  hipStream_t st = (hipStream_t)hip_stream;
  int steps = 0;
  LR_CHECK_HIP(hipMemcpyAsync(&steps, h->ctr, sizeof(int), hipMemcpyDeviceToHost, st));
  LR_CHECK_HIP(hipStreamSynchronize(st));
  memset(out, 0, sizeof(*out));
  out->optimizer_steps = steps;
  out->passes = h->pass;
  return LR_OK;
}
extern "C" int lr_llama_lora_set_progress(lr_llama_lora_t* h, const LrLoraProgress* in, void* hip_stream) {
  LR_RUN(check_progress(h, in, "lr_llama_lora_set_progress"));
  for (int i = 0; i < 2; ++i)
    if (in->reserved[i]) LR_FAIL(LR_EINVAL, "lr_llama_lora_set_progress: LrLoraProgress.reserved[%d] is not zero", i);
  if (in->optimizer_steps < 0 || in->passes < 0)
    LR_FAIL(LR_EINVAL, "lr_llama_lora_set_progress: negative count (optimizer_steps=%lld, passes=%lld)",
            (long long)in->optimizer_steps, (long long)in->passes);
  if (in->optimizer_steps > (int64_t)INT32_MAX)   // ctr[0] is an int on the device
    LR_FAIL(LR_EINVAL, "lr_llama_lora_set_progress: optimizer_steps=%lld exceeds the handle's 31-bit step counter",
            (long long)in->optimizer_steps);
  if (in->passes > (int64_t)UINT32_MAX)           // the pass counter is a uint32_t
    LR_FAIL(LR_EINVAL, "lr_llama_lora_set_progress: passes=%lld exceeds the handle's 32-bit pass counter",
            (long long)in->passes);
  // the value travels in the command itself: no host buffer has to outlive the call
  LR_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)h->ctr, (int)in->optimizer_steps, 1, (hipStream_t)hip_stream));
  h->pass = (uint32_t)in->passes;
  return LR_OK;
}
extern "C" size_t lr_llama_lora_eval_workspace_bytes(const lr_llama_lora_t* h, int32_t max_tokens, int32_t max_seqs) {
  if (!h || max_tokens < 1) return 0;
  if (max_seqs < 1) max_seqs = 1;
  const LrLlamaConfig& c = h->base->cfg;
  return carve(c, lora_mods(c, h->cfg.r, h->mods), max_tokens, max_seqs, 0, 1, false, nullptr, 0, false,
               h->base->q_norm != nullptr).total;
}

static u16* work_of(const lr_llama_lora* h, int l) { return h->work + (size_t)l * h->work_per_layer; }

// bf16 working copies of every layer's adapters from the fp32 masters
static int prep_adapters(lr_llama_lora* h, hipStream_t st) {
  const LrLlamaConfig& c = h->base->cfg;
  const size_t r = h->cfg.r, d = c.hidden_size;
  const LoraMods md = lora_mods(c, h->cfg.r, h->mods);
  for (int l = 0; l < c.num_layers; ++l) {
    const float* p = h->params + (size_t)l * h->per_layer;
    u16* w = work_of(h, l);
    if (h->mods == LT_MOD_QV) {
      LR_RUN(lr_launch_prep_lora(p, p + r * d, p + r * d + r * h->qcols, p + 2 * r * d + r * h->qcols, (int)r, (int)d,
                                 h->qcols, h->vcols, c.head_dim, w, w + 2 * LT_RP * d, w + 2 * LT_RP * d + LT_RP * h->qcols,
                                 st));
      continue;
    }
    // the copies of a module that is not adapted are never written: they stay zero from the state's initial memset
    u16 *bq_t = w + 2 * LT_RP * d, *bv_t = bq_t + LT_RP * (size_t)h->qcols;
    const int f2 = 2 * c.intermediate_size;
    struct { int m, perm; u16 *a, *b; int ldb; } job[LT_NMOD] = {
        {MQ, 1, w, bq_t, h->qcols},
        {MV, 0, w + LT_RP * d, bv_t, h->vcols},
        {MK, 1, w + md.wk_a, w + md.wk_b, h->kcols},
        {MO, 0, w + md.wo_a, w + md.wo_b, (int)d},
        {MGATE, 2, w + md.wgu_a, w + md.wgu_b, f2},
        {MUP, 3, w + md.wgu_a + LT_RP * d, w + md.wgu_b + (size_t)LT_RP * f2, f2},
        {MDOWN, 0, w + md.wdn_a, w + md.wdn_b, (int)d}};
    for (const auto& j : job)
      if (md.has(j.m))
        LR_RUN(lr_launch_prep_module(p + md.pa[j.m], p + md.pb[j.m], (int)r, md.in[j.m], md.out[j.m], j.perm, c.head_dim, j.a,
                                     j.b, j.ldb, st));
  }
  return LR_OK;
}

static int validate_batch(const lr_llama_lora* h, const int32_t* cu_host, int B, int* n_out, int* maxT_out) {
  const LrLlamaConfig& c = h->base->cfg;
  if (int rc = lr_check_segments(cu_host, B, "llama lora", nullptr, maxT_out)) return rc;
  if (*maxT_out > c.max_positions)
    LR_FAIL(LR_EINVAL, "llama lora: prompt of %d tokens exceeds max_positions %d", *maxT_out, c.max_positions);
  *n_out = cu_host[B];
  return LR_OK;
}

// forward with live adapters; layer l's activations go to slot (save ? l : 0); the final residual lands in ws.x_final
static int forward(lr_llama_lora* h, const int32_t* ids, const int32_t* cu, const int32_t* cu_host, int B, int n,
                   int maxT, const LoraWs& ws, bool save, float drop_p, hipStream_t st) {
  const LrLlamaConfig& c = h->base->cfg;
  const int d = c.hidden_size, f = c.intermediate_size, nh = c.num_heads, nkv = c.num_kv_heads, hd = c.head_dim;
  const int qw = (nh + 2 * nkv) * hd;
  const float scaling = h->cfg.alpha / (float)h->cfg.r;
  const int gv = (h->base->gemm_variant == 5 || h->base->gemm_variant == 7) ? 0 : h->base->gemm_variant;
  const LoraMods md = lora_mods(c, h->cfg.r, h->mods);
  const int r = h->cfg.r, tw = md.tw, L = c.num_layers;
  LrAttnKernel attn_kernel;  // the backward needs the statistics: lse wanted
  LR_RUN(lr_resolve_attention({.variant = h->base->attn_variant, .hd = hd, .want_lse = true, .lora = true}, &attn_kernel));
  LR_RUN(lr_launch_token_meta(cu, B, 0, nullptr, ws.tok_pos, nullptr, ws.last_rows, st));
  LR_RUN(lr_launch_rope_table(ws.rope, maxT, hd, c.rope_theta, st, nullptr, &h->base->rope_scaling));   // the base's scaling
  LR_RUN(lr_launch_embed(ids, nullptr, h->base->embed, c.vocab_size, d, slot(ws, 0).x, n, st));
  for (int l = 0; l < c.num_layers; ++l) {
    const LrLlamaLayerWeights& w = h->base->layers[l];
    const LoraLayerSave s = slot(ws, save ? l : 0);
    u16* x_next = l + 1 < c.num_layers ? (save ? slot(ws, l + 1).x : s.x) : ws.x_final;
    const u16* wk = work_of(h, l);
    const u16 *a_cat = wk, *bq_t = wk + 2 * LT_RP * (size_t)d, *bv_t = bq_t + LT_RP * (size_t)h->qcols;
    const uint32_t stream = lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)l);
    LR_RUN(lr_launch_rmsnorm(s.x, w.input_norm, s.xn, n, d, c.rms_eps, nullptr, st));
    hipStream_t sd;
    LR_RUN(fork_side(h, st, &sd));  // t = drop(xn) A^T next to the QKV GEMM: both only read xn
    LR_RUN(lr_launch_skinny(s.xn, d, n, d, a_cat, 2, s.t, 2 * LT_RP, 0, 1.0f, stream, drop_p, sd));
    if (md.has(MK)) LR_RUN(lr_launch_skinny(s.xn, d, n, d, wk + md.wk_a, 1, s.t2, tw, md.tk, 1.0f, stream, drop_p, sd));
    LR_RUN(lr_launch_gemm({.A = s.xn, .B = w.wqkv, .C = s.qkv, .M = n, .N = qw, .K = d, .variant = gv}, st));
    LR_RUN(join_side(h, st));
    // k's delta rides in the same sweep, before the rotation like q's
    LR_RUN(lr_launch_lora_rope_fwd(s.qkv, n, qw, h->qcols, h->kcols, hd, s.t, bq_t, bv_t, h->cfg.r, scaling, ws.tok_pos,
                                   ws.rope, st, s.t2, tw, md.tk, md.has(MK) ? wk + md.wk_b : nullptr,
                                   h->base->q_norm ? LrQkNormFwd{h->base->q_norm[l], h->base->k_norm[l], c.rms_eps, s.xqk}
                                                   : LrQkNormFwd{}));
    LR_RUN(lr_launch_attention({.qkv = s.qkv, .out = s.att, .lse = s.lse, .cu = cu, .cu_host = cu_host, .S = B, .n_tok = n,
                                .nh = nh, .nkv = nkv, .hd = hd}, attn_kernel, st));
    // the extra modules: t = drop(input) A^T on the side stream next to the GEMM that reads the same input, the delta
    // s * t B^T added behind the GEMM (o and down: behind its residual epilogue; gate / up: before swiglu reads gu, so
    // that the saved gu holds the pre-activation values the backward differentiates at)
    if (md.has(MO)) {
      LR_RUN(fork_side(h, st, &sd));
      LR_RUN(lr_launch_skinny(s.att, h->qcols, n, h->qcols, wk + md.wo_a, 1, s.t2, tw, md.to, 1.0f,
                              lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)(l + L)), drop_p, sd));
    }
    LR_RUN(lr_launch_gemm({.A = s.att, .B = w.wo, .C = s.xmid, .R = s.x, .M = n, .N = d, .K = nh * hd, .epi = LR_EPI_RESIDUAL,
                           .variant = gv}, st));
    if (md.has(MO)) {
      LR_RUN(join_side(h, st));
      LR_RUN(lr_launch_lora_expand(s.xmid, d, n, d, s.t2, tw, md.to, wk + md.wo_b, r, scaling, 0, 0.f, st));
    }
    LR_RUN(lr_launch_rmsnorm(s.xmid, w.post_norm, ws.xn2, n, d, c.rms_eps, nullptr, st));
    if (md.gu()) {
      LR_RUN(fork_side(h, st, &sd));
      LR_RUN(lr_launch_skinny(ws.xn2, d, n, d, wk + md.wgu_a, 2, s.t2, tw, md.tgu, 1.0f,
                              lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)(l + 2 * L)), drop_p, sd));
    }
    LR_RUN(lr_launch_gemm({.A = ws.xn2, .B = w.wgu, .C = s.gu, .M = n, .N = 2 * f, .K = d, .variant = gv}, st));
    if (md.gu()) {  // the delta rides in the pass that reads gu
      LR_RUN(join_side(h, st));
      LR_RUN(lr_launch_swiglu_lora_fwd(s.gu, ws.hmid, n, f, s.t2, tw, md.tgu, wk + md.wgu_b, r, scaling, st));
    } else {
      LR_RUN(lr_launch_swiglu_fwd(s.gu, ws.hmid, n, f, st));
    }
    if (md.has(MDOWN)) {
      LR_RUN(fork_side(h, st, &sd));
      LR_RUN(lr_launch_skinny(ws.hmid, f, n, f, wk + md.wdn_a, 1, s.t2, tw, md.tdn, 1.0f,
                              lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)(l + 3 * L)), drop_p, sd));
    }
    LR_RUN(lr_launch_gemm({.A = ws.hmid, .B = w.wdown, .C = x_next, .R = s.xmid, .M = n, .N = d, .K = f, .epi = LR_EPI_RESIDUAL,
                           .variant = gv}, st));
    if (md.has(MDOWN)) {
      LR_RUN(join_side(h, st));
      LR_RUN(lr_launch_lora_expand(x_next, d, n, d, s.t2, tw, md.tdn, wk + md.wdn_b, r, scaling, 0, 0.f, st));
    }
  }
  return LR_OK;
}

extern "C" int lr_llama_lora_loss_grad(lr_llama_lora_t* h, const int32_t* packed_ids, const int32_t* cu_seqlens,
                                       const int32_t* cu_seqlens_host, int32_t B, const int32_t* loss_rows,
                                       const int32_t* loss_targets, int32_t m, float grad_scale, int32_t accumulate,
                                       float* out, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!h || !packed_ids || !cu_seqlens || !cu_seqlens_host || !loss_rows || !loss_targets || !out || !workspace)
    LR_FAIL(LR_EINVAL, "lr_llama_lora_loss_grad: null argument");
  if (m < 1) LR_FAIL(LR_EINVAL, "lr_llama_lora_loss_grad: no labelled rows (m=%d)", m);
  hipStream_t st = (hipStream_t)hip_stream;
  const LrLlamaConfig& c = h->base->cfg;
  int n, maxT;
  LR_RUN(validate_batch(h, cu_seqlens_host, B, &n, &maxT));
  if (m > n) LR_FAIL(LR_EINVAL, "lr_llama_lora_loss_grad: %d labelled rows for %d tokens", m, n);
  const LoraMods md = lora_mods(c, h->cfg.r, h->mods);
  const bool det = h->deterministic != 0;
  const LoraWs ws = carve(c, md, n, B, m, c.num_layers, true, (char*)workspace, h->cfg.r, det, h->base->q_norm != nullptr);
  if (ws.total > workspace_bytes)
    LR_FAIL(LR_EWORKSPACE, "lr_llama_lora_loss_grad: workspace needs %zu bytes for %d tokens, have %zu", ws.total, n,
            workspace_bytes);
  const int d = c.hidden_size, f = c.intermediate_size, nh = c.num_heads, nkv = c.num_kv_heads, hd = c.head_dim;
  const int qw = (nh + 2 * nkv) * hd, r = h->cfg.r;
  const float scaling = h->cfg.alpha / (float)r, drop_p = h->cfg.dropout;
  const float drop_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  const int gv = (h->base->gemm_variant == 5 || h->base->gemm_variant == 7) ? 0 : h->base->gemm_variant;
  const int tw = md.tw, L = c.num_layers;
  // the backward follows the forward's kernel (lr_resolve_attention's lora route): the head_dim-64 MFMA pair is variant 6,
  // the head_dim-96 one variant 8, the head_dim-256 one variant 9
  LrAttnKernel fwd_kernel;
  LR_RUN(lr_resolve_attention({.variant = h->base->attn_variant, .hd = hd, .want_lse = true, .lora = true}, &fwd_kernel));
  const int attn_bwd_variant = fwd_kernel == LR_ATTN_HD64    ? 6
                               : fwd_kernel == LR_ATTN_HD96  ? 8
                               : fwd_kernel == LR_ATTN_HD256 ? 9
                                                             : h->base->attn_variant;
  h->pass += 1;
  if (!accumulate) LR_CHECK_HIP(hipMemsetAsync(h->grads, 0, h->n_params * sizeof(float), st));
  float* const scal = det ? ws.det_loss : h->scratch;  // loss sum / per-row losses, rows without a token id
  float* const dp = ws.det_part;                       // null in the default mode: the launchers then add atomically
  LR_CHECK_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(float), st));
  LR_RUN(prep_adapters(h, st));
  LR_RUN(forward(h, packed_ids, cu_seqlens, cu_seqlens_host, B, n, maxT, ws, true, drop_p, st));

  // ---- loss head on the labelled rows only (model/llm.py:113-126)
  LR_RUN(lr_launch_gather_rows(ws.x_final, loss_rows, m, d, ws.xg, st));
  LR_RUN(lr_launch_rmsnorm(ws.xg, h->base->final_norm, ws.hn, m, d, c.rms_eps, nullptr, st));
  LR_RUN(lr_launch_gemm({.A = ws.hn, .B = h->base->lm_head, .C = ws.logits, .M = m, .N = c.vocab_size, .K = d, .variant = gv}, st));
  LR_RUN(lr_launch_ce_bf16(ws.logits, m, c.vocab_size, loss_targets, grad_scale / (float)m, scal, st, det));
  LR_RUN(lr_launch_finish_loss(scal, m, out, st, det));
  LR_RUN(lr_launch_gemm({.A = ws.logits, .B = h->lm_head_t, .C = ws.dhn, .M = m, .N = d, .K = c.vocab_size, .variant = gv}, st));
  LR_CHECK_HIP(hipMemsetAsync(ws.dx, 0, (size_t)n * d * 2, st));
  LR_RUN(lr_launch_rmsnorm_bwd(ws.dhn, ws.xg, h->base->final_norm, nullptr, ws.dx, m, d, c.rms_eps, loss_rows, nullptr,
                               nullptr, 0, 0, 0.f, st));

  // ---- backward through the layers; ws.dx = gradient of the residual stream
  for (int l = c.num_layers - 1; l >= 0; --l) {
    const LrLlamaLayerWeights& w = h->base->layers[l];
    const LrLlamaLayerWeightsT& wt = h->layers_t[l];
    const LoraLayerSave s = slot(ws, l);
    const u16* wk = work_of(h, l);
    const u16 *a_cat = wk, *bq_t = wk + 2 * LT_RP * (size_t)d, *bv_t = bq_t + LT_RP * (size_t)h->qcols;
    float* g = h->grads + (size_t)l * h->per_layer;
    auto grad_of = [&](int mod, int ab) { return md.has(mod) ? g + (ab ? md.pb[mod] : md.pa[mod]) : (float*)nullptr; };
    float *daq = grad_of(MQ, 0), *dbq = grad_of(MQ, 1), *dav = grad_of(MV, 0), *dbv = grad_of(MV, 1);
    const uint32_t stream = lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)l);
    hipStream_t sd;
    // One extra module with input X [n][in], output gradient dY [n][.]: on the side stream, next to the data-gradient GEMM that
    // reads the same dY,  d B += s t^T dY,  d t = s dY B,  d A += drop(X)^T d t;  behind the GEMM,  d X += mask .* (d t A).
    // MLP: x_out = xmid + down(silu(gate) * up)
    if (md.has(MDOWN)) {
      const uint32_t s3 = lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)(l + 3 * L));
      LR_RUN(fork_side(h, st, &sd));
      LR_RUN(lr_launch_lora_tn(1, s.t2, tw, md.tdn, ws.dx, d, n, d, scaling, grad_of(MDOWN, 1), nullptr, r, 1, 0, 0, 0.f, sd, dp));
      LR_RUN(lr_launch_skinny(ws.dx, d, n, d, wk + md.wdn_b, 1, ws.dt2, tw, md.tdn, scaling, 0, 0.f, sd));
      LR_RUN(lr_launch_swiglu_fwd(s.gu, ws.hmid_b, n, f, sd));  // down's input, recomputed before swiglu_bwd overwrites gu
      LR_RUN(lr_launch_lora_tn(1, ws.dt2, tw, md.tdn, ws.hmid_b, f, n, f, 1.0f, grad_of(MDOWN, 0), nullptr, r, 0, 0, s3, drop_p,
                               sd, dp));
      LR_RUN(lr_launch_gemm({.A = ws.dx, .B = wt.wdown_t, .C = ws.dh, .M = n, .N = f, .K = d, .variant = gv}, st));
      LR_RUN(join_side(h, st));
      LR_RUN(lr_launch_lora_expand(ws.dh, f, n, f, ws.dt2, tw, md.tdn, wk + md.wdn_a, r, drop_scale, s3, drop_p, st));
    } else {
      LR_RUN(lr_launch_gemm({.A = ws.dx, .B = wt.wdown_t, .C = ws.dh, .M = n, .N = f, .K = d, .variant = gv}, st));
    }
    LR_RUN(lr_launch_swiglu_bwd(s.gu, ws.dh, n, f, st));
    if (md.gu()) {  // s.gu now holds d gu in the interleaved layout; b_gu's zero half-columns make it a plain weight
      const uint32_t s2 = lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)(l + 2 * L));
      LR_RUN(fork_side(h, st, &sd));
      LR_RUN(lr_launch_lora_tn(2, s.t2, tw, md.tgu, s.gu, 2 * f, n, 2 * f, scaling, grad_of(MGATE, 1), grad_of(MUP, 1), r, 3, 0, 0,
                               0.f, sd, dp));
      LR_RUN(lr_launch_skinny(s.gu, 2 * f, n, 2 * f, wk + md.wgu_b, 2, ws.dt2, tw, md.tgu, scaling, 0, 0.f, sd));
      LR_RUN(lr_launch_rmsnorm(s.xmid, w.post_norm, ws.xn2_b, n, d, c.rms_eps, nullptr, sd));  // gate / up's input, recomputed
      LR_RUN(lr_launch_lora_tn(2, ws.dt2, tw, md.tgu, ws.xn2_b, d, n, d, 1.0f, grad_of(MGATE, 0), grad_of(MUP, 0), r, 0, 0, s2,
                               drop_p, sd, dp));
      LR_RUN(lr_launch_gemm({.A = s.gu, .B = wt.wgu_t, .C = ws.dxn, .M = n, .N = d, .K = 2 * f, .variant = gv}, st));
      LR_RUN(join_side(h, st));
      // d xn2 += mask .* (d t_gate A_gate + d t_up A_up) rides in the norm's LoRA arm, as q / v's does in the input norm's
      LR_RUN(lr_launch_rmsnorm_bwd(ws.dxn, s.xmid, w.post_norm, ws.dx, ws.dx, n, d, c.rms_eps, nullptr, ws.dt2 + md.tgu,
                                   wk + md.wgu_a, r, s2, drop_p, st, tw));
    } else {
      LR_RUN(lr_launch_gemm({.A = s.gu, .B = wt.wgu_t, .C = ws.dxn, .M = n, .N = d, .K = 2 * f, .variant = gv}, st));
      LR_RUN(lr_launch_rmsnorm_bwd(ws.dxn, s.xmid, w.post_norm, ws.dx, ws.dx, n, d, c.rms_eps, nullptr, nullptr, nullptr, 0,
                                   0, 0.f, st));
    }
    // attention block: xmid = x + o_proj(attention(q, k, v))
    if (md.has(MO)) {
      const uint32_t s1 = lr_lora_drop_stream(h->cfg.seed, h->pass, (uint32_t)(l + L));
      LR_RUN(fork_side(h, st, &sd));
      LR_RUN(lr_launch_lora_tn(1, s.t2, tw, md.to, ws.dx, d, n, d, scaling, grad_of(MO, 1), nullptr, r, 1, 0, 0, 0.f, sd, dp));
      LR_RUN(lr_launch_skinny(ws.dx, d, n, d, wk + md.wo_b, 1, ws.dt2, tw, md.to, scaling, 0, 0.f, sd));
      LR_RUN(lr_launch_lora_tn(1, ws.dt2, tw, md.to, s.att, h->qcols, n, h->qcols, 1.0f, grad_of(MO, 0), nullptr, r, 0, 0, s1,
                               drop_p, sd, dp));
      LR_RUN(lr_launch_gemm({.A = ws.dx, .B = wt.wo_t, .C = ws.datt, .M = n, .N = nh * hd, .K = d, .variant = gv}, st));
      LR_RUN(join_side(h, st));
      LR_RUN(lr_launch_lora_expand(ws.datt, h->qcols, n, h->qcols, ws.dt2, tw, md.to, wk + md.wo_a, r, drop_scale, s1,
                                   drop_p, st));
    } else {
      LR_RUN(lr_launch_gemm({.A = ws.dx, .B = wt.wo_t, .C = ws.datt, .M = n, .N = nh * hd, .K = d, .variant = gv}, st));
    }
    // ... down to the gradient of the UNROTATED q, k, v (the inverse rotation rides in the attention passes)
    LR_RUN(lr_launch_attention_bwd(s.qkv, s.att, ws.datt, s.lse, ws.dqkv, ws.dsum, ws.dkv32, cu_seqlens, cu_seqlens_host, B,
                                   n, nh, nkv, hd, attn_bwd_variant, st, ws.tok_pos, ws.rope, det));
    // Qwen3: ... and through the per-head norms to the gradient of the projections' outputs, before anything reads dqkv
    if (h->base->q_norm)
      LR_RUN(lr_launch_qk_norm_bwd(ws.dqkv, n, qw, s.xqk, h->qcols + h->kcols, nh, nkv, hd, h->base->q_norm[l],
                                   h->base->k_norm[l], c.rms_eps, st));
    // adapters (side stream, next to the qkv data-gradient GEMM; both only read dqkv):
    // d B, d t = scaling * (d q B_q | d v B_v), d A
    LR_RUN(fork_side(h, st, &sd));
    if (dbq && dbv) {
      LR_RUN(lr_launch_lora_db(ws.dqkv, n, qw, h->qcols, h->kcols, hd, s.t, r, scaling, dbq, dbv, sd, dp));
    } else {
      if (dbq) LR_RUN(lr_launch_lora_tn(1, s.t, 2 * LT_RP, 0, ws.dqkv, qw, n, h->qcols, scaling, dbq, nullptr, r, 2, hd, 0, 0.f, sd, dp));
      if (dbv)
        LR_RUN(lr_launch_lora_tn(1, s.t, 2 * LT_RP, LT_RP, ws.dqkv + h->qcols + h->kcols, qw, n, h->vcols, scaling, dbv, nullptr,
                                 r, 1, hd, 0, 0.f, sd, dp));
    }
    // (the working copies of a q / v that is not adapted are zero: its d t columns come out zero for the norm's LoRA arm)
    LR_RUN(lr_launch_skinny(ws.dqkv, qw, n, h->qcols, bq_t, 1, ws.dt, 2 * LT_RP, 0, scaling, 0, 0.f, sd));
    LR_RUN(lr_launch_skinny(ws.dqkv + h->qcols + h->kcols, qw, n, h->vcols, bv_t, 1, ws.dt, 2 * LT_RP, LT_RP, scaling, 0,
                            0.f, sd));
    if (daq && dav) LR_RUN(lr_launch_lora_da(s.xn, n, d, ws.dt, r, stream, drop_p, daq, dav, sd, dp));
    else if (daq || dav)
      LR_RUN(lr_launch_lora_tn(1, ws.dt, 2 * LT_RP, daq ? 0 : LT_RP, s.xn, d, n, d, 1.0f, daq ? daq : dav, nullptr, r, 0, 0,
                               stream, drop_p, sd, dp));
    if (md.has(MK)) {
      LR_RUN(lr_launch_lora_tn(1, s.t2, tw, md.tk, ws.dqkv + h->qcols, qw, n, h->kcols, scaling, grad_of(MK, 1), nullptr, r, 2, hd,
                               0, 0.f, sd, dp));
      LR_RUN(lr_launch_skinny(ws.dqkv + h->qcols, qw, n, h->kcols, wk + md.wk_b, 1, ws.dt2, tw, md.tk, scaling, 0, 0.f, sd));
      LR_RUN(lr_launch_lora_tn(1, ws.dt2, tw, md.tk, s.xn, d, n, d, 1.0f, grad_of(MK, 0), nullptr, r, 0, 0, stream, drop_p, sd, dp));
    }
    if (l > 0)  // below layer 0 only the frozen embedding is left: its input gradient has no reader
      LR_RUN(lr_launch_gemm({.A = ws.dqkv, .B = wt.wqkv_t, .C = ws.dxn, .M = n, .N = d, .K = qw, .variant = gv}, st));
    LR_RUN(join_side(h, st));
    if (l > 0 && md.has(MK))  // k shares q / v's input and its mask
      LR_RUN(lr_launch_lora_expand(ws.dxn, d, n, d, ws.dt2, tw, md.tk, wk + md.wk_a, r, drop_scale, stream, drop_p, st));
    if (l > 0)
      LR_RUN(lr_launch_rmsnorm_bwd(ws.dxn, s.x, w.input_norm, ws.dx, ws.dx, n, d, c.rms_eps, nullptr, ws.dt, a_cat, r,
                                   stream, drop_p, st));
  }
  return LR_OK;
}

extern "C" int lr_llama_lora_apply(lr_llama_lora_t* h, float lr, float max_grad_norm, float* out_norm,
                                   void* hip_stream) {
  if (!h) LR_FAIL(LR_EINVAL, "lr_llama_lora_apply: null handle");
  return lr_launch_lora_adamw(h->params, h->grads, h->m, h->v, h->n_params, h->scratch + 2, h->ctr, lr, max_grad_norm,
                              h->cfg.beta1, h->cfg.beta2, h->cfg.eps, h->cfg.weight_decay, out_norm,
                              (hipStream_t)hip_stream, h->deterministic != 0);
}

// scoring with the adapters as they are now (validation during training, trainer/llm.py:123-126): the forward
// above without dropout, then the inference head (final norm + verbalizer rows of lm_head at each prompt's end)
extern "C" int lr_llama_lora_prefill_verbalize(lr_llama_lora_t* h, const int32_t* packed_ids,
                                               const int32_t* cu_seqlens, const int32_t* cu_seqlens_host, int32_t B,
                                               const int32_t* label_token_ids, int32_t C, float* out_scores,
                                               void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!h || !packed_ids || !cu_seqlens || !cu_seqlens_host || !label_token_ids || !out_scores || !workspace || C < 1)
    LR_FAIL(LR_EINVAL, "lr_llama_lora_prefill_verbalize: bad argument");
  hipStream_t st = (hipStream_t)hip_stream;
  const LrLlamaConfig& c = h->base->cfg;
  int n, maxT;
  LR_RUN(validate_batch(h, cu_seqlens_host, B, &n, &maxT));
  const LoraWs ws = carve(c, lora_mods(c, h->cfg.r, h->mods), n, B, 0, 1, false, (char*)workspace, 0, false,
                          h->base->q_norm != nullptr);
  if (ws.total > workspace_bytes)
    LR_FAIL(LR_EWORKSPACE, "lr_llama_lora_prefill_verbalize: workspace needs %zu bytes for %d tokens, have %zu",
            ws.total, n, workspace_bytes);
  LR_RUN(prep_adapters(h, st));
  LR_RUN(forward(h, packed_ids, cu_seqlens, cu_seqlens_host, B, n, maxT, ws, false, 0.f, st));
  return lr_launch_head(ws.x_final, ws.last_rows, h->base->final_norm, h->base->lm_head, label_token_ids, B, C,
                        c.hidden_size, c.rms_eps, out_scores, c.vocab_size, st);
}

extern "C" int lr_qk_norm_bwd_bf16(uint16_t* dqk, int32_t rows, int32_t ld, int32_t col0, const uint16_t* x, int32_t ldx,
                                   int32_t nq, int32_t nk, int32_t head_dim, const uint16_t* q_norm, const uint16_t* k_norm,
                                   float eps, void* hip_stream) {
  if (!lr_qk_norm_head_dim_ok(head_dim))
    LR_FAIL(LR_EUNSUPPORTED, "lr_qk_norm_bwd_bf16: head_dim %d (a power of two from 16 to 256)", head_dim);
  if (!dqk || !x || rows < 1 || ld < 8 || ldx < 8 || col0 < 0 || col0 % 8 != 0 || nq < 0 || nk < 0 || nq + nk < 1 ||
      (long long)col0 + (long long)(nq + nk) * head_dim > ld || !(eps >= 0.f) || !(eps < __builtin_inff()))
    LR_FAIL(LR_EINVAL, "lr_qk_norm_bwd_bf16: bad argument (rows %d, ld %d, col0 %d a multiple of 8, %d + %d heads of %d)", rows,
            ld, col0, nq, nk, head_dim);
  return lr_launch_qk_norm_bwd(dqk + col0, rows, ld, x, ldx, nq, nk, head_dim, q_norm, k_norm, eps, (hipStream_t)hip_stream);
}

extern "C" int lr_transpose_bf16(const uint16_t* src, int32_t rows, int32_t cols, uint16_t* dst, void* hip_stream) {
  if (!src || !dst) LR_FAIL(LR_EINVAL, "lr_transpose_bf16: null pointer");
  return lr_launch_transpose_bf16(src, rows, cols, dst, (hipStream_t)hip_stream);
}

extern "C" int lr_attention_varlen_lse(const uint16_t* qkv, uint16_t* out, float* lse, const int32_t* cu_seqlens,
                                       const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads,
                                       int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* hip_stream) {
  if (!qkv || !out || !lse || !cu_seqlens || !cu_seqlens_host || B < 1)
    LR_FAIL(LR_EINVAL, "lr_attention_varlen_lse: bad argument");
  if (int rc = lr_check_segments(cu_seqlens_host, B, "lr_attention_varlen_lse")) return rc;
  LrAttnKernel kernel;
  if (int rc = lr_resolve_attention({.variant = variant, .hd = head_dim, .want_lse = true}, &kernel)) return rc;
  return lr_launch_attention({.qkv = qkv, .out = out, .lse = lse, .cu = cu_seqlens, .cu_host = cu_seqlens_host, .S = B,
                              .n_tok = cu_seqlens_host[B], .nh = num_heads, .nkv = num_kv_heads, .hd = head_dim},
                             kernel, (hipStream_t)hip_stream);
}

extern "C" size_t lr_attention_bwd_scratch_bytes(int32_t total, int32_t num_heads, int32_t num_kv_heads,
                                                 int32_t head_dim) {
  if (total < 1) return 0;
  return lr_align_up((size_t)total * num_heads * 4, 256) + (size_t)total * 2 * num_kv_heads * head_dim * 4;
}

extern "C" int lr_attention_varlen_bwd_ex(const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out,
                                          const float* lse, uint16_t* dqkv, const int32_t* cu_seqlens,
                                          const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads,
                                          int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* scratch,
                                          size_t scratch_bytes, const int32_t* tok_pos, const float* rope_cs,
                                          int32_t rope_positions, int32_t deterministic, void* hip_stream) {
  if (!qkv || !out || !d_out || !lse || !dqkv || !cu_seqlens || !cu_seqlens_host || !scratch || B < 1)
    LR_FAIL(LR_EINVAL, "lr_attention_varlen_bwd: bad argument");
  if (int rc = lr_check_segments(cu_seqlens_host, B, "lr_attention_varlen_bwd")) return rc;
  if (rope_cs) {
    if (!tok_pos) LR_FAIL(LR_EINVAL, "lr_attention_varlen_bwd: rotary table without token positions");
    for (int b = 0; b < B; ++b)  // the MFMA epilogues index the table by the position inside the prompt
      if (cu_seqlens_host[b + 1] - cu_seqlens_host[b] > rope_positions)
        LR_FAIL(LR_EINVAL, "lr_attention_varlen_bwd: segment %d has %d tokens, the rotary table %d positions", b,
                cu_seqlens_host[b + 1] - cu_seqlens_host[b], rope_positions);
  }
  const int n = cu_seqlens_host[B];
  if (scratch_bytes < lr_attention_bwd_scratch_bytes(n, num_heads, num_kv_heads, head_dim))
    LR_FAIL(LR_EWORKSPACE, "lr_attention_varlen_bwd: scratch too small");
  float* dsum = (float*)scratch;
  float* dkv32 = (float*)((char*)scratch + lr_align_up((size_t)n * num_heads * 4, 256));
  return lr_launch_attention_bwd(qkv, out, d_out, lse, dqkv, dsum, dkv32, cu_seqlens, cu_seqlens_host, B, n, num_heads,
                                 num_kv_heads, head_dim, variant, (hipStream_t)hip_stream, tok_pos, rope_cs,
                                 deterministic != 0);
}

extern "C" int lr_attention_varlen_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* d_out,
                                       const float* lse, uint16_t* dqkv, const int32_t* cu_seqlens,
                                       const int32_t* cu_seqlens_host, int32_t B, int32_t num_heads,
                                       int32_t num_kv_heads, int32_t head_dim, int32_t variant, void* scratch,
                                       size_t scratch_bytes, void* hip_stream) {
  return lr_attention_varlen_bwd_ex(qkv, out, d_out, lse, dqkv, cu_seqlens, cu_seqlens_host, B, num_heads, num_kv_heads,
                                    head_dim, variant, scratch, scratch_bytes, nullptr, nullptr, 0, 0, hip_stream);
}

// ---- the LoRA step's small kernels alone (exposed for parity tests) ----------------------------------------------------------
// Thin wrappers of llama_train.h's launchers: every assumption a kernel makes about its arguments that the host can see is checked
// here before anything is launched; no arithmetic is added. The training step calls the launchers, never these.
static inline bool lt_al16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                           const void* e = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e)) & 15) == 0;
}
static inline bool lt_drop_ok(float p) { return p >= 0.f && p < 1.f; }

extern "C" int lr_lora_skinny_bf16(const uint16_t* x, int32_t ldx, int32_t n, int32_t k, const uint16_t* w, int32_t nt,
                                   uint16_t* out, int32_t ldo, int32_t ocol, float scale, uint32_t drop_stream, float drop_p,
                                   void* hip_stream) {
  if (!x || !w || !out) LR_FAIL(LR_EINVAL, "lr_lora_skinny_bf16: null pointer");
  if (n < 0 || k < 1 || ldx < k || (nt != 1 && nt != 2) || ocol < 0 || (long long)ocol + 16 * nt > ldo || !lt_drop_ok(drop_p))
    LR_FAIL(LR_EINVAL, "lr_lora_skinny_bf16: bad argument (n %d, K %d <= ldx %d, %d tiles from column %d of %d, dropout %g)", n, k,
            ldx, nt, ocol, ldo, (double)drop_p);
  if (k % 64 != 0 || ldx % 8 != 0 || !lt_al16(x, w))
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_skinny_bf16: K %d must be a multiple of 64, ldx %d of 8, x and w 16-byte aligned", k, ldx);
  return lr_launch_skinny(x, ldx, n, k, w, nt, out, ldo, ocol, scale, drop_stream, drop_p, (hipStream_t)hip_stream);
}

// the C name of llama_train.h's lr_lora_tn_partial_floats (one quantity: the floats of det_part), with the arguments checked
extern "C" size_t lr_lora_tn_det_floats(int32_t nj, int32_t n, int32_t cols, int32_t r, int32_t layout) {
  if ((nj != 1 && nj != 2) || n < 1 || cols < 1 || r < 1 || r > LT_RP || layout < 0 || layout > 3) return 0;
  return lr_lora_tn_partial_floats(nj, n, cols, r, layout);
}

extern "C" int lr_lora_tn_f32(int32_t nj, const uint16_t* t, int32_t ldt, int32_t tcol, const uint16_t* x, int32_t ldx, int32_t n,
                              int32_t cols, float scale, float* out0, float* out1, int32_t r, int32_t layout, int32_t head_dim,
                              uint32_t drop_stream, float drop_p, float* det_part, size_t det_part_floats, void* hip_stream) {
  if (!t || !x) LR_FAIL(LR_EINVAL, "lr_lora_tn_f32: null pointer");
  if ((nj != 1 && nj != 2) || n < 0 || r < 1 || r > LT_RP || layout < 0 || layout > 3 || tcol < 0 ||
      (long long)tcol + 16 * nj > ldt || cols < 1 || cols > ldx || !lt_drop_ok(drop_p))
    LR_FAIL(LR_EINVAL, "lr_lora_tn_f32: bad argument (%d tiles from column %d of %d, n %d, cols %d <= ldx %d, r %d, layout %d, "
            "dropout %g)", nj, tcol, ldt, n, cols, ldx, r, layout, (double)drop_p);
  // which outputs a layout writes: layout 3 splits the two tiles over out0 (gate) and out1 (up), either may be null;
  // the others write tile a to out_a
  if (layout == 3 ? (nj != 2 || (!out0 && !out1)) : (!out0 || (nj == 2 && !out1)))
    LR_FAIL(LR_EINVAL, "lr_lora_tn_f32: layout %d with %d tiles: null output", layout, nj);
  if (cols % 64 != 0) LR_FAIL(LR_EUNSUPPORTED, "lr_lora_tn_f32: %d columns (must be a multiple of 64)", cols);
  if (layout == 2 && (head_dim < 2 || head_dim % 2 != 0 || cols % head_dim != 0))
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_tn_f32: layout 2 needs an even head_dim %d dividing %d columns", head_dim, cols);
  if (((uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)det_part) & 3) LR_FAIL(LR_EINVAL, "lr_lora_tn_f32: misaligned fp32 pointer");
  if (det_part && det_part_floats < lr_lora_tn_partial_floats(nj, n, cols, r, layout))
    LR_FAIL(LR_EWORKSPACE, "lr_lora_tn_f32: %zu floats of partial tiles, %zu needed", det_part_floats,
            lr_lora_tn_partial_floats(nj, n, cols, r, layout));
  return lr_launch_lora_tn(nj, t, ldt, tcol, x, ldx, n, cols, scale, out0, out1, r, layout, head_dim, drop_stream, drop_p,
                           (hipStream_t)hip_stream, det_part);
}

extern "C" int lr_lora_expand_bf16(uint16_t* y, int32_t ldy, int32_t n, int32_t cols, const uint16_t* t, int32_t ldt, int32_t tcol,
                                   const uint16_t* w, int32_t r, float s, uint32_t drop_stream, float drop_p, void* hip_stream) {
  if (!y || !t || !w) LR_FAIL(LR_EINVAL, "lr_lora_expand_bf16: null pointer");
  if (n < 0 || cols < 1 || cols > ldy || r < 1 || r > LT_RP || tcol < 0 || (long long)tcol + LT_RP > ldt || !lt_drop_ok(drop_p))
    LR_FAIL(LR_EINVAL, "lr_lora_expand_bf16: bad argument (n %d, cols %d <= ldy %d, r %d, column %d of %d, dropout %g)", n, cols,
            ldy, r, tcol, ldt, (double)drop_p);
  if (cols % 8 != 0 || ldy % 8 != 0 || !lt_al16(y, w))
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_expand_bf16: cols %d and ldy %d must be multiples of 8, y and w 16-byte aligned", cols, ldy);
  return lr_launch_lora_expand(y, ldy, n, cols, t, ldt, tcol, w, r, s, drop_stream, drop_p, (hipStream_t)hip_stream);
}

extern "C" int lr_swiglu_fwd_bf16(const uint16_t* gu, uint16_t* h, int32_t n, int32_t f, void* hip_stream) {
  if (!gu || !h || n < 0 || f < 1) LR_FAIL(LR_EINVAL, "lr_swiglu_fwd_bf16: bad argument (n %d, f %d)", n, f);
  if (f % 16 != 0 || !lt_al16(gu, h)) LR_FAIL(LR_EUNSUPPORTED, "lr_swiglu_fwd_bf16: intermediate size %d (a multiple of 16)", f);
  return lr_launch_swiglu_fwd(gu, h, n, f, (hipStream_t)hip_stream);
}

extern "C" int lr_swiglu_bwd_bf16(uint16_t* gu, const uint16_t* dh, int32_t n, int32_t f, void* hip_stream) {
  if (!gu || !dh || n < 0 || f < 1) LR_FAIL(LR_EINVAL, "lr_swiglu_bwd_bf16: bad argument (n %d, f %d)", n, f);
  if (f % 16 != 0 || !lt_al16(gu, dh)) LR_FAIL(LR_EUNSUPPORTED, "lr_swiglu_bwd_bf16: intermediate size %d (a multiple of 16)", f);
  return lr_launch_swiglu_bwd(gu, dh, n, f, (hipStream_t)hip_stream);
}

extern "C" int lr_rmsnorm_bwd_bf16(const uint16_t* dy, const uint16_t* x, const uint16_t* w, const uint16_t* res, uint16_t* out,
                                   int32_t rows, int32_t d, float eps, const int32_t* out_rows, const uint16_t* dt, int32_t ldt,
                                   const uint16_t* a_cat, int32_t r, uint32_t drop_stream, float drop_p, void* hip_stream) {
  if (!dy || !x || !w || !out) LR_FAIL(LR_EINVAL, "lr_rmsnorm_bwd_bf16: null pointer");
  if (rows < 0 || d < 1 || !(eps >= 0.f) || !(eps < __builtin_inff()) || !lt_drop_ok(drop_p))
    LR_FAIL(LR_EINVAL, "lr_rmsnorm_bwd_bf16: bad argument (rows %d, d %d, eps %g, dropout %g)", rows, d, (double)eps,
            (double)drop_p);
  if (dt && (!a_cat || r < 1 || r > LT_RP || ldt < 2 * LT_RP))
    LR_FAIL(LR_EINVAL, "lr_rmsnorm_bwd_bf16: the LoRA arm needs a_cat, 1 <= r %d <= 16 and ldt %d >= 32", r, ldt);
  if (d % 8 != 0 || d > 256 * 8 * 4)
    LR_FAIL(LR_EUNSUPPORTED, "lr_rmsnorm_bwd_bf16: hidden_size %d (multiple of 8, <= 8192)", d);
  if (!lt_al16(dy, x, w, res, out) || !lt_al16(a_cat))
    LR_FAIL(LR_EUNSUPPORTED, "lr_rmsnorm_bwd_bf16: pointers must be 16-byte aligned");
  return lr_launch_rmsnorm_bwd(dy, x, w, res, out, rows, d, eps, out_rows, dt, a_cat, r, drop_stream, drop_p,
                               (hipStream_t)hip_stream, ldt);
}

extern "C" int lr_ce_bf16(uint16_t* logits, int32_t m, int32_t vocab, const int32_t* targets, float gscale, float* scal,
                          float* out, int32_t deterministic, void* hip_stream) {
  if (!logits || !targets || !scal || !out || m < 0 || vocab < 1)
    LR_FAIL(LR_EINVAL, "lr_ce_bf16: bad argument (m %d, vocab %d)", m, vocab);
  hipStream_t st = (hipStream_t)hip_stream;
  LR_CHECK_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(float), st));
  LR_RUN(lr_launch_ce_bf16(logits, m, vocab, targets, gscale, scal, st, deterministic != 0));
  return lr_launch_finish_loss(scal, m, out, st, deterministic != 0);
}

extern "C" int lr_rowdot_bf16(const uint16_t* o, const uint16_t* d_o, int32_t n, int32_t num_heads, int32_t head_dim, float* out,
                              void* hip_stream) {
  if (!o || !d_o || !out || n < 0 || num_heads < 1 || head_dim < 1 || (long long)n * num_heads > 0x7fffffff - 16)
    LR_FAIL(LR_EINVAL, "lr_rowdot_bf16: bad argument (n %d, %d heads of %d)", n, num_heads, head_dim);
  if (head_dim % 8 != 0 || !lt_al16(o, d_o)) LR_FAIL(LR_EUNSUPPORTED, "lr_rowdot_bf16: head_dim %d (a multiple of 8)", head_dim);
  return lr_launch_rowdot(o, d_o, n, num_heads, head_dim, out, (hipStream_t)hip_stream);
}

extern "C" int lr_lora_adamw_f32(float* p, float* g, float* m, float* v, size_t n, float* scratch, int32_t* ctr, float lr,
                                 float max_grad_norm, float beta1, float beta2, float eps, float weight_decay, float* out_norm,
                                 int32_t deterministic, void* hip_stream) {
  if (!p || !g || !m || !v || !scratch || !ctr) LR_FAIL(LR_EINVAL, "lr_lora_adamw_f32: null pointer");
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f))
    LR_FAIL(LR_EINVAL, "lr_lora_adamw_f32: bad argument (betas %g %g, eps %g)", (double)beta1, (double)beta2, (double)eps);
  if (n == 0) return LR_OK;   // no parameters, no step: ctr stays (the header says so)
  if (deterministic && !lt_al16(g)) LR_FAIL(LR_EUNSUPPORTED, "lr_lora_adamw_f32: deterministic norm needs a 16-byte aligned g");
  return lr_launch_lora_adamw(p, g, m, v, n, scratch, ctr, lr, max_grad_norm, beta1, beta2, eps, weight_decay, out_norm,
                              (hipStream_t)hip_stream, deterministic != 0);
}

extern "C" int lr_lora_rope_fwd_bf16(uint16_t* qkv, int32_t n, int32_t qw, int32_t qcols, int32_t kcols, int32_t head_dim,
                                     const uint16_t* t, const uint16_t* bq_t, const uint16_t* bv_t, int32_t r, float scaling,
                                     const int32_t* tok_pos, const float* rope_cs, const uint16_t* tk, int32_t ldtk, int32_t tkcol,
                                     const uint16_t* bk_t, const uint16_t* q_norm, const uint16_t* k_norm, float eps,
                                     uint16_t* xsave, void* hip_stream) {
  if (!qkv || !t || !bq_t || !bv_t || !tok_pos || !rope_cs) LR_FAIL(LR_EINVAL, "lr_lora_rope_fwd_bf16: null pointer");
  if (n < 0 || r < 1 || r > LT_RP || head_dim < 2 || qcols < 0 || kcols < 0 || (long long)qcols + kcols > qw)
    LR_FAIL(LR_EINVAL, "lr_lora_rope_fwd_bf16: bad argument (n %d, r %d, head_dim %d, q %d + k %d columns of %d)", n, r, head_dim,
            qcols, kcols, qw);
  if (bk_t && (!tk || tkcol < 0 || (long long)tkcol + LT_RP > ldtk))
    LR_FAIL(LR_EINVAL, "lr_lora_rope_fwd_bf16: the k adapter needs tk and column %d + 16 <= ldtk %d", tkcol, ldtk);
  if (!q_norm && (k_norm || xsave)) LR_FAIL(LR_EINVAL, "lr_lora_rope_fwd_bf16: k norm or save buffer without a q norm");
  if (q_norm && (!(eps >= 0.f) || !(eps < __builtin_inff()))) LR_FAIL(LR_EINVAL, "lr_lora_rope_fwd_bf16: eps %g", (double)eps);
  if (head_dim % 8 != 0 || qw % 8 != 0 || qcols % head_dim != 0 || kcols % head_dim != 0)
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_rope_fwd_bf16: head_dim %d must be a multiple of 8 and divide the q %d and k %d columns, "
            "row stride %d a multiple of 8", head_dim, qcols, kcols, qw);
  if (!lt_al16(qkv, bq_t, bv_t, bk_t, rope_cs) || !lt_al16(q_norm, k_norm, xsave))
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_rope_fwd_bf16: pointers must be 16-byte aligned");
  LrQkNormFwd qkn;
  qkn.q_norm = q_norm;
  qkn.k_norm = k_norm;
  qkn.eps = eps;
  qkn.xsave = xsave;
  return lr_launch_lora_rope_fwd(qkv, n, qw, qcols, kcols, head_dim, t, bq_t, bv_t, r, scaling, tok_pos, rope_cs,
                                 (hipStream_t)hip_stream, tk, ldtk, tkcol, bk_t, qkn);
}

extern "C" int lr_rope_bwd_bf16(uint16_t* dqkv, int32_t n, int32_t qw, int32_t rot_cols, int32_t head_dim, const int32_t* tok_pos,
                                const float* rope_cs, void* hip_stream) {
  if (!dqkv || !tok_pos || !rope_cs) LR_FAIL(LR_EINVAL, "lr_rope_bwd_bf16: null pointer");
  if (n < 0 || rot_cols < 0 || rot_cols > qw || head_dim < 2)
    LR_FAIL(LR_EINVAL, "lr_rope_bwd_bf16: bad argument (n %d, %d rotated columns of %d, head_dim %d)", n, rot_cols, qw, head_dim);
  if (!lt_al16(dqkv)) LR_FAIL(LR_EUNSUPPORTED, "lr_rope_bwd_bf16: dqkv must be 16-byte aligned");
  return lr_launch_rope_bwd(dqkv, n, qw, rot_cols, head_dim, tok_pos, rope_cs, (hipStream_t)hip_stream);
}

extern "C" int lr_swiglu_lora_fwd_bf16(uint16_t* gu, uint16_t* h, int32_t n, int32_t f, const uint16_t* t, int32_t ldt, int32_t tcol,
                                       const uint16_t* w, int32_t r, float s, void* hip_stream) {
  if (!gu || !h || !t || !w) LR_FAIL(LR_EINVAL, "lr_swiglu_lora_fwd_bf16: null pointer");
  if (n < 0 || f < 1 || r < 1 || r > LT_RP || tcol < 0 || (long long)tcol + 2 * LT_RP > ldt)
    LR_FAIL(LR_EINVAL, "lr_swiglu_lora_fwd_bf16: bad argument (n %d, f %d, r %d, column %d + 32 <= ldt %d)", n, f, r, tcol, ldt);
  if (f % 16 != 0 || !lt_al16(gu, h, w))
    LR_FAIL(LR_EUNSUPPORTED, "lr_swiglu_lora_fwd_bf16: intermediate size %d (a multiple of 16), 16-byte aligned pointers", f);
  return lr_launch_swiglu_lora_fwd(gu, h, n, f, t, ldt, tcol, w, r, s, (hipStream_t)hip_stream);
}

extern "C" int lr_lora_prep_bf16(const float* aq, const float* bq, const float* av, const float* bv, int32_t r, int32_t d,
                                 int32_t qcols, int32_t vcols, int32_t head_dim, uint16_t* a_cat, uint16_t* bq_t, uint16_t* bv_t,
                                 void* hip_stream) {
  if (!aq || !bq || !av || !bv || !a_cat || !bq_t || !bv_t) LR_FAIL(LR_EINVAL, "lr_lora_prep_bf16: null pointer");
  if (r < 1 || r > LT_RP || d < 1 || qcols < 1 || vcols < 1 || head_dim < 2 || head_dim % 2 != 0 || qcols % head_dim != 0 ||
      2LL * LT_RP * d + (long long)LT_RP * ((long long)qcols + vcols) > 0x7fffffff)
    LR_FAIL(LR_EINVAL, "lr_lora_prep_bf16: bad argument (r %d, hidden %d, q %d and v %d columns, head_dim %d)", r, d, qcols, vcols,
            head_dim);
  return lr_launch_prep_lora(aq, bq, av, bv, r, d, qcols, vcols, head_dim, a_cat, bq_t, bv_t, (hipStream_t)hip_stream);
}

extern "C" int lr_lora_prep_module_bf16(const float* a, const float* b, int32_t r, int32_t in, int32_t out, int32_t perm,
                                        int32_t head_dim, uint16_t* a_w, uint16_t* b_t, int32_t ldb, void* hip_stream) {
  if (!a || !b || !a_w || !b_t) LR_FAIL(LR_EINVAL, "lr_lora_prep_module_bf16: null pointer");
  if (r < 1 || r > LT_RP || in < 1 || out < 1 || perm < 0 || perm > 3 || (long long)LT_RP * ((long long)in + out) > 0x7fffffff ||
      ldb < (perm >= 2 ? 2LL * out : (long long)out))
    LR_FAIL(LR_EINVAL, "lr_lora_prep_module_bf16: bad argument (r %d, in %d, out %d, perm %d, ldb %d)", r, in, out, perm, ldb);
  if (perm == 1 && (head_dim < 2 || head_dim % 2 != 0 || out % head_dim != 0))
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_prep_module_bf16: perm 1 needs an even head_dim %d dividing %d rows", head_dim, out);
  if (perm >= 2 && out % 16 != 0)
    LR_FAIL(LR_EUNSUPPORTED, "lr_lora_prep_module_bf16: perm %d needs out %d a multiple of 16", perm, out);
  return lr_launch_prep_module(a, b, r, in, out, perm, head_dim, a_w, b_t, ldb, (hipStream_t)hip_stream);
}
