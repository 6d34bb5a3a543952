// lru_topk_plan.h -- everything the HOST decides about one top-K call (lru_topk.hip, lru_topk_bf16.hip): which path serves
// the shape, the launch geometry of the exact pass and of the two bf16 passes, and where every workspace region lies.
// tk_plan() is the one place these are computed; the launchers, lr_topk_path() and lr_topk_workspace_bytes() read it.
// No HIP header: tests/topk_plan_sweep.cpp compiles this file with a plain C++ compiler and sweeps it.
#ifndef LRU_TOPK_PLAN_H
#define LRU_TOPK_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

static inline size_t lr_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

#define TK_USERS 128      // users per workgroup of the exact pass
#define TK_MAX_CHUNKS 256
#define TK_MAX_WGS 1024   // chunks are added only while user tiles x chunks stays below this
#define TK_CAND_CAP 1024  // candidate slots per user (1 M items: ~270 above the bound + ~40 % in the 2 delta band)

// the bound pre-pass runs for catalogs of TK_BOUND_MIN_TILES .. TK_BOUND_MAX_TILES tiles (LR_TOPK_BOUND=0 switches it off)
#define TK_BOUND_MIN_TILES 64
#define TK_BOUND_MAX_TILES 2048  // 32 maxima per lane in bound_select_kernel: one per tile for catalogs up to 65 536 items,
                                 // one per group of 2^gshift tiles beyond (bound_group_shift): the R-th largest GROUP maximum
                                 // still certifies R different items at or above it, so the bound's proof is unchanged; a
                                 // group of 512 items at rank R of 1 954 (1 M items, R = 251) sits at the same item quantile
                                 // (2.7e-4, ~270 items + the 2 delta band) as a 32-item tile at the same rank fraction
#define TK_BOUND_MAX_GSHIFT 6

// Split the item tiles into chunks so that (user tiles x chunks) fills the 256 CUs in whole rounds:
// minimise rounds x (tiles per chunk + the per-chunk fixed cost). The fixed cost -- the unfiltered first tiles
// while the thresholds settle, plus compaction + sort of 128 users' lists at the end -- measures ~130 tile-times
// (Beauty sweep: 1.41 / 1.97 / 2.27 / 2.00 / 2.28 ms for 1..5 chunks = rounds x (0.36 ms + 2.8 us x tiles)).
// With a seeded threshold (bound pre-pass) a chunk's fixed cost is what is left of that: the prologue and the final
// compaction + sort (~ TK_FIXED_SEEDED tile-times), so more, shorter chunks are worth it where they fill the last round.
#define TK_FIXED_PLAIN 128
#define TK_FIXED_SEEDED 24
static inline void topk_geometry(int n_tiles, int B, bool seeded, int* n_chunks, int* tiles_per_chunk) {
  const int n_ut = (B + TK_USERS - 1) / TK_USERS;
  int max_chunks = TK_MAX_WGS / n_ut;
  if (max_chunks > TK_MAX_CHUNKS) max_chunks = TK_MAX_CHUNKS;
  if (max_chunks > n_tiles) max_chunks = n_tiles;
  if (max_chunks < 1) max_chunks = 1;
  long best_cost = -1;
  int best = 1;
  for (int c = 1; c <= max_chunks; ++c) {
    const int tpc = (n_tiles + c - 1) / c;
    const int real = (n_tiles + tpc - 1) / tpc;
    const long rounds = ((long)n_ut * real + 255) / 256;
    const long cost = rounds * (tpc + (seeded ? TK_FIXED_SEEDED : TK_FIXED_PLAIN));
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  static int forced = -1;  // LR_TOPK_CHUNKS=n: tuning knob (0 / unset = the model above)
  if (forced < 0) {
    const char* e = getenv("LR_TOPK_CHUNKS");
    forced = e ? atoi(e) : 0;
  }
  if (forced > 0 && forced <= max_chunks) best = forced;
  *tiles_per_chunk = (n_tiles + best - 1) / best;
  *n_chunks = (n_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// tiles per maximum = 2^shift: the smallest shift (0, or >= 2 so that a group is whole float4 iterations of the kernel)
// that leaves at most TK_BOUND_MAX_TILES maxima per user; -1: the catalog is beyond 2^TK_BOUND_MAX_GSHIFT x that
static inline int bound_group_shift(int n_tiles) {
  int gs = 0;
  while (((n_tiles + (1 << gs) - 1) >> gs) > TK_BOUND_MAX_TILES) ++gs;
  if (gs == 1) gs = 2;
  return gs <= TK_BOUND_MAX_GSHIFT ? gs : -1;
}
static inline int bound_groups(int n_tiles) {
  const int gs = bound_group_shift(n_tiles);
  return gs < 0 ? 0 : (n_tiles + (1 << gs) - 1) >> gs;
}
// the catalog's tile count is one the pre-pass can serve at all, whatever K and L
static inline bool bound_in_range(int n_tiles) { return n_tiles >= TK_BOUND_MIN_TILES && bound_group_shift(n_tiles) >= 0; }
// ... and it runs only where EVERY user is sure to get a bound: rank R = K + masked ids <= K + L + 1 must not exceed the
// group count (ML-100k: L = 200 against 115 tiles -- its users keep the exact full pass)
static inline bool bound_enabled(int n_tiles, int K, int L) {
  static int env = -1;
  if (env < 0) {
    const char* e = getenv("LR_TOPK_BOUND");
    env = (e && e[0] == '0') ? 0 : 1;
  }
  return env && bound_in_range(n_tiles) && K + L + 1 <= bound_groups(n_tiles);
}

// users per workgroup of the two bf16 passes (8 waves x 2 MFMA column tiles of 32 users; 4 were measured and dropped:
// lru_topk_bf16.hip) and the longest chunk of tiles the candidate pass's per-chunk lists are sized for, both functions of
// the batch size only
static inline int lr_bf16_users_per_wg(int B) { (void)B; return 512; }
static inline int lr_bf16_max_chunk_tiles(int B) { return lr_bf16_users_per_wg(B) >= 1024 ? 256 : 512; }   // x 32 items < 65 536

// chunks of the two bf16 passes (the same for both: same operands -> the same approximate scores)
static inline void bf16_geometry(int n_tiles, int B, int gshift, int* n_chunks, int* tiles_per_chunk) {
  const int upw = lr_bf16_users_per_wg(B);
  const int n_ut = (B + upw - 1) / upw;
  int chunks = (1024 + n_ut - 1) / n_ut;                 // two rounds of the 512 resident workgroups (two per CU)
  // ... but never more than lr_bf16_max_chunk_tiles(B) tiles per chunk, however many user tiles there are: the candidate
  // pass's per-chunk LDS lists hold 20-40 entries per user with 16-bit offsets (16 k users used to get
  // 32 chunks of ~1 000 tiles at 1 M items, ~12 expected candidates per user and chunk against 24 slots)
  const int min_chunks = (n_tiles + lr_bf16_max_chunk_tiles(B) - 1) / lr_bf16_max_chunk_tiles(B);
  static int target_wgs = -1;   // LR_BF16_WGS=n: tuning knob (workgroups per launch; 0 / unset = 1024)
  if (target_wgs < 0) {
    const char* e = getenv("LR_BF16_WGS");
    target_wgs = e ? atoi(e) : 0;
  }
  if (target_wgs > 0) chunks = (target_wgs + n_ut - 1) / n_ut;
  if (chunks < min_chunks) chunks = min_chunks;
  const int unit = gshift >= 2 ? (4 << gshift) : 4;  // a chunk is whole float4 iterations / whole quads of tile groups
  const int units = (n_tiles + unit - 1) / unit;
  if (chunks > units) chunks = units;
  *tiles_per_chunk = unit * ((units + chunks - 1) / chunks);
  *n_chunks = (n_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

// The workspace: partial [B x chunks][K] rank keys | hist [B][L] sorted ids | and, for the bound path, tmax [B][ld] |
// thresh [B] | cand_thresh [B] | cand_count [B] + the overflow flag | cand [B][TK_CAND_CAP]. Every region is a multiple of
// 256 bytes, so every offset is 256-byte aligned.
enum TkRegion { TK_PARTIAL, TK_HIST, TK_TMAX, TK_THRESH, TK_CAND_THRESH, TK_CAND_COUNT, TK_CAND, TK_REGIONS };

// bytes of every region: partial_rows = B x chunks, hist_ids = B x L (0: no history to sort), ld = 0: no bound path
static inline void tk_region_bytes(size_t B, size_t partial_rows, int K, size_t hist_ids, size_t ld, size_t out[TK_REGIONS]) {
  const size_t b = ld ? B : 0;
  out[TK_PARTIAL] = partial_rows * K * sizeof(unsigned long long);
  out[TK_HIST] = hist_ids * sizeof(int32_t);
  out[TK_TMAX] = b * ld * sizeof(float);
  out[TK_THRESH] = b * sizeof(float);
  out[TK_CAND_THRESH] = b * sizeof(float);
  out[TK_CAND_COUNT] = ld ? (B + 1) * sizeof(int) : 0;
  out[TK_CAND] = b * TK_CAND_CAP * sizeof(int32_t);
  for (int i = 0; i < TK_REGIONS; ++i) out[i] = lr_align_up(out[i], 256);
}

struct TkPlan {
  bool seeded;                        // the bound -> candidates -> exact rescoring path serves this shape
  int n_chunks, tiles_per_chunk;      // exact pass (item_topk_kernel) and merge
  int gshift, n_groups, ld;           // bound: 2^gshift tiles per maximum, maxima per user, tmax row length (groups rounded up to 4)
  int bf16_chunks, bf16_tiles_per_chunk, n_user_groups;   // both bf16 passes
  size_t off[TK_REGIONS];             // byte offset of every region
  size_t overflow_flag;               // byte offset of the int behind cand_count's B entries
  size_t total;
};

// B >= 1
static inline TkPlan tk_plan(int n_tiles, int B, int K, int L, int exclude_history) {
  TkPlan p = {};
  p.seeded = bound_enabled(n_tiles, K, L);
  topk_geometry(n_tiles, B, p.seeded, &p.n_chunks, &p.tiles_per_chunk);
  if (p.seeded) {
    p.gshift = bound_group_shift(n_tiles);
    p.n_groups = bound_groups(n_tiles);
    p.ld = (int)lr_align_up((size_t)p.n_groups, 4);
    bf16_geometry(n_tiles, B, p.gshift, &p.bf16_chunks, &p.bf16_tiles_per_chunk);
    p.n_user_groups = (B + lr_bf16_users_per_wg(B) - 1) / lr_bf16_users_per_wg(B);
  }
  size_t bytes[TK_REGIONS];
  tk_region_bytes((size_t)B, (size_t)B * p.n_chunks, K, exclude_history ? (size_t)B * L : 0, (size_t)p.ld, bytes);
  for (int i = 0; i < TK_REGIONS; ++i) {
    p.off[i] = p.total;
    p.total += bytes[i];
  }
  p.overflow_flag = p.off[TK_CAND_COUNT] + (size_t)B * sizeof(int);
  return p;
}

// Sized for EVERY call of up to (B users, K, L): whether the bound pre-pass runs depends on K + L + 1 <= n_tiles, which a
// later call with a smaller K or L can satisfy when the sizing call did not -- so its scratch is included whenever the
// catalog's tile count is in the pre-pass's range, whatever K and L (the size is monotone in B, K and L).
static inline size_t lr_topk_workspace_bytes(int B, int K, int L, int n_tiles) {
  // user tiles x chunks <= TK_MAX_WGS (+ one chunk minimum) => B x chunks <= max(B, 128 * TK_MAX_WGS)
  size_t rows = (size_t)B;
  if (rows < (size_t)TK_USERS * TK_MAX_WGS) rows = (size_t)TK_USERS * TK_MAX_WGS;
  size_t bytes[TK_REGIONS], total = 0;
  tk_region_bytes((size_t)B, rows, K, (size_t)B * (L > 0 ? L : 1), bound_in_range(n_tiles) ? lr_align_up((size_t)bound_groups(n_tiles), 4) : 0,
                  bytes);
  for (int i = 0; i < TK_REGIONS; ++i) total += bytes[i];
  return total;
}

#endif  // LRU_TOPK_PLAN_H
