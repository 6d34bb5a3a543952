// topk_plan_sweep.cpp -- host-only sweep of llamarec_amd/csrc/lru_topk_plan.h, compiled and run by tests/test_topk_plan.py.
// Prints one FAIL line per broken property (the first 20) and a final "plans <n> pairs <m> fails <f>"; exit code 1 on any.
#include <stdio.h>

#include "lru_topk_plan.h"

static const int NT[] = {1, 2, 63, 64, 65, 71, 115, 126, 129, 378, 2048, 2049, 2188, 3125, 8193, 31251, 131072, 131073};
static const int BS[] = {1, 3, 127, 128, 129, 512, 513, 4096, 16384, 22332};
static const int KS[] = {1, 7, 20, 50, 64};
static const int LS[] = {1, 10, 50, 64, 65, 200};
static long fails = 0;
#define CHECK(c)                                                                                                    \
  do {                                                                                                              \
    if (!(c) && fails++ < 20) printf("FAIL %s: n_tiles=%d B=%d K=%d L=%d exclude=%d\n", #c, nt, B, K, L, ex);      \
  } while (0)

// `chunks` chunks of `tpc` tiles cover n tiles, and none of them is empty
static bool covers(int n, int chunks, int tpc) { return chunks >= 1 && (long)chunks * tpc >= n && (long)(chunks - 1) * tpc < n; }

static void check_plan(int nt, int B, int K, int L, int ex) {
  const TkPlan p = tk_plan(nt, B, K, L, ex);
  const size_t b = p.seeded ? (size_t)B : 0;   // the regions' sizes, restated here without rounding
  const size_t raw[TK_REGIONS] = {(size_t)B * p.n_chunks * K * 8, ex ? (size_t)B * L * 4 : 0, b * p.ld * 4, b * 4, b * 4,
                                  p.seeded ? b * 4 + 4 : 0, b * TK_CAND_CAP * 4};
  CHECK(p.off[0] == 0);
  for (int i = 0; i < TK_REGIONS; ++i) {
    const size_t end = i + 1 < TK_REGIONS ? p.off[i + 1] : p.total;
    CHECK(p.off[i] % 256 == 0 && p.off[i] + raw[i] <= end && end - (p.off[i] + raw[i]) < 256);
  }
  CHECK(p.total % 256 == 0);
  CHECK(covers(nt, p.n_chunks, p.tiles_per_chunk));
  CHECK(!(nt == 63 || nt == 131073 || K + L + 1 > bound_groups(nt)) || !p.seeded);
  if (!p.seeded) return;
  CHECK(p.overflow_flag == p.off[TK_CAND_COUNT] + (size_t)B * 4 && p.overflow_flag + 4 <= p.off[TK_CAND]);
  CHECK(p.gshift >= 0 && p.gshift != 1 && ((long)p.n_groups << p.gshift) >= nt && p.ld >= p.n_groups && p.ld % 4 == 0);
  CHECK(covers(nt, p.bf16_chunks, p.bf16_tiles_per_chunk));
  CHECK(p.bf16_tiles_per_chunk % (p.gshift >= 2 ? (4 << p.gshift) : 4) == 0 && p.bf16_tiles_per_chunk <= lr_bf16_max_chunk_tiles(B));
  CHECK((long)p.n_user_groups * lr_bf16_users_per_wg(B) >= B && (long)(p.n_user_groups - 1) * lr_bf16_users_per_wg(B) < B);
}

int main() {
  long plans = 0, pairs = 0;
  for (int nt : NT)
    for (int B : BS)
      for (int K : KS)
        for (int L : LS) {
          int ex = 0;
          for (; ex < 2; ++ex, ++plans) check_plan(nt, B, K, L, ex);
          // the claim above lr_topk_workspace_bytes: sized for (B, K, L), it serves every call it dominates
          const size_t sized = lr_topk_workspace_bytes(B, K, L, nt);
          for (int b : BS)
            for (int k : KS)
              for (int l : LS)
                for (ex = 0; ex < 2 && b <= B && k <= K && l <= L; ++ex, ++pairs)
                  if (tk_plan(nt, b, k, l, ex).total > sized && fails++ < 20)
                    printf("FAIL undersized: n_tiles=%d sized for B=%d K=%d L=%d, called with B=%d K=%d L=%d exclude=%d\n", nt, B, K, L, b, k, l, ex);
        }
  printf("plans %ld pairs %ld fails %ld\n", plans, pairs, fails);
  return fails ? 1 : 0;
}
