// lru_train_scores.h -- item GEMM + cross-entropy of the training step with stored logits (lru_train_scores.hip)
#pragma once
#include "lr_common.h"

size_t lr_train_scores_ws_floats(int R, int C);
// loss sum += into scal[0] (scal[1] = number of labelled rows, already counted); dX [R][64] is added to
// (pre-zeroed by the caller: the item splits of the d x pass use atomics);
// dE [C][64] and dbias [C] are added to with atomics (pre-zeroed gradient buffer)
int lr_launch_train_scores(const float* x, const float* E, const float* bias, const long long* labels, int R, int C, float* ws,
                           float* scal, float* dX, float* dE, float* dbias, hipStream_t st);
// the splits lr_launch_train_scores will use at a shape: item splits of the score pass / of the d x pass, row parts of the
// d E pass, 64-item super-blocks, rows padded to whole 16-row panels
struct LrTrainScoresPlan {
  int ns, ns2, nq, nsb, Rpad;
};
void lr_train_scores_plan(int R, int C, LrTrainScoresPlan* p);

// fused item GEMM + cross-entropy, logits never stored (lru_train_ce.hip)
struct LrTrainCePlan {
  int item_chunks, item_tiles_per_chunk;   // passes A and B: 32-item tiles per workgroup along grid.x
  int row_chunks, row_tiles_per_chunk;     // pass C: 32-row tiles
};
void lr_train_ce_plan(int R, int C, LrTrainCePlan* p);
size_t lr_train_ce_part_floats(int R, int C);
int lr_launch_train_ce(const float* X, const float* E, const float* bias, const long long* labels, int R, int C,
                       float* ws_part, float* scal, float* dX, float* dE, float* dbias, hipStream_t st);
