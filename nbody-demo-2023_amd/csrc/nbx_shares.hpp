// nbx_shares.hpp -- which rank of a group owns which bodies, and when nbx_group_retune moves them: the share planner of
// nbx_group.hip, host-only.  Standard library, include/nbx.h and nbx_plan.hpp only: no HIP call, no environment, no nbx_ctx and no
// last_error(), so that g++ compiles it without ROCm (tests/test_shares_cpu.py drives it against tests/golden/group_shares.json).
// Errors come back as NBX_ERR_* with the text of nbx_last_error() in *msg, as from plan_launch.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/nbx.h"
#include "nbx_plan.hpp"  // ceil_div, round_up, kTile: blocks are whole j tiles of the kernels

#pragma GCC visibility push(hidden)  // nothing of this is visible outside the library
namespace nbx {

// Who owns what: rank r of `ranks` owns the bodies [begin[r], begin[r] + count[r]) of the n_alloc records every rank holds.
struct Shares {
  int ranks = 0, n_alloc = 0;
  int block = 0;  // the common block size (the in-place all-gather needs one); 0 = the blocks are unequal
  std::vector<int> begin, count;
};

// Balanced, tile-aligned blocks; ranks that would own nothing are dropped (fewer ranks than n_ranks come back).  The same arithmetic
// as sharded.block_partition (tests/test_sharded_gloo.py::test_check_world_matches_the_native_partition compares them) with that
// reduction applied.
inline Shares equal_shares(int n, int n_ranks) {
  Shares s;
  int P = n_ranks, block = 0;
  for (;; --P) {
    block = round_up(ceil_div(n, P), kTile);
    if (P == 1 || (long long)(P - 1) * block < n) break;
  }
  s.ranks = P; s.block = block; s.n_alloc = P * block;
  for (int r = 0; r < P; ++r) { s.begin.push_back(r * block); s.count.push_back(std::min(n, (r + 1) * block) - r * block); }
  return s;
}

// Weighted shares: the ceil(n / 256) tiles of 256 records are handed out in proportion to the weights (NULL: equal; largest
// remainder, ties to the lower rank), every rank at least one tile; ranks beyond the number of tiles are dropped.  The reference's
// co-execution split gives device 0 `n * cpu_ratio` bodies and the rest to the other device (opencl/Compute.cpp:241-249); here every
// block stays a whole number of j tiles, which is what the kernels' zero-mass padding and the in-place exchange rely on.
inline int weighted_shares(int n, int n_ranks, const double* w, Shares* out, const char** msg) {
  const int tiles = ceil_div(n, kTile);
  const int P = std::min(n_ranks, tiles);
  double sum = 0.0;
  for (int r = 0; r < P; ++r) {
    const double x = w ? w[r] : 1.0;
    if (!(x > 0.0) || !std::isfinite(x)) { *msg = "weights must be finite and > 0"; return NBX_ERR_ARG; }
    sum += x;
  }
  std::vector<double> ideal((size_t)P);
  std::vector<int> t((size_t)P);
  long long total = 0;
  for (int r = 0; r < P; ++r) {
    ideal[r] = (double)tiles * (w ? w[r] : 1.0) / sum;
    t[r] = std::max(1, (int)std::floor(ideal[r]));
    total += t[r];
  }
  while (total != tiles) {  // at most P passes each way: every rank is within one tile of its ideal share afterwards (or at the 1-tile floor)
    int pick = -1;
    double best = 0.0;
    for (int r = 0; r < P; ++r) {
      const double d = total < tiles ? ideal[r] - t[r] : t[r] - ideal[r];
      if (total > tiles && t[r] <= 1) continue;
      if (pick < 0 || d > best) { pick = r; best = d; }
    }
    if (pick < 0) { *msg = "partition_weighted: cannot balance the tiles"; return NBX_ERR_STATE; }  // cannot happen: P <= tiles
    t[pick] += total < tiles ? 1 : -1;
    total += total < tiles ? 1 : -1;
  }
  out->ranks = P; out->n_alloc = tiles * kTile; out->block = 0;
  out->begin.assign((size_t)P, 0); out->count.assign((size_t)P, 0);
  int first = 0;
  for (int r = 0; r < P; ++r) {
    out->begin[r] = first * kTile;
    out->count[r] = std::min(n, (first + t[r]) * kTile) - first * kTile;
    first += t[r];
  }
  return NBX_OK;
}

// nbx_tune_weights: new weights from what every rank achieved -- its bodies per millisecond of force kernel, normalised to sum 1.
inline int tune_weights(int n_ranks, const int* i_count, const double* force_ms, double* weights_out, const char** msg) {
  if (n_ranks <= 0 || !i_count || !force_ms || !weights_out) { *msg = "nbx_tune_weights: NULL argument or no ranks"; return NBX_ERR_ARG; }
  double sum = 0.0;
  for (int r = 0; r < n_ranks; ++r) {
    if (i_count[r] <= 0 || !(force_ms[r] > 0.0) || !std::isfinite(force_ms[r]))
      { *msg = "nbx_tune_weights: every rank needs bodies and a positive measured time"; return NBX_ERR_ARG; }
    sum += (double)i_count[r] / force_ms[r];
  }
  for (int r = 0; r < n_ranks; ++r) weights_out[r] = ((double)i_count[r] / force_ms[r]) / sum;
  return NBX_OK;
}

// The tuner of nbx_group_retune.  The step lasts as long as the slowest rank.  A rank's time is NOT linear in its share: a
// reference-order launch lasts as long as its fullest SIMD, so one body more than a whole number of waves per SIMD costs a whole extra
// wave there (131072 bodies of 1M: 30 ms, 131073: 58 ms).  The rate-proportional move of tune_weights cannot know that, so it is judged
// by its result: if the window after a move was slower than the window before it by more than this factor, the move is taken back and
// the shares are left alone from then on.
constexpr double kTakeBackAbove = 1.01;
// Predict before moving: rank r's time under the new shares = its measured time x cost(new share) / cost(present share), with the
// library's own cost table as the model (a step function of the share in reference order).  A move that the model expects to leave
// the slowest rank above this fraction of its present time -- e.g. across a one-workgroup-per-CU boundary -- is not made.
constexpr double kMoveBelow = 0.99;

struct Tuner {
  std::vector<int> prev_begin, prev_count;  // the shares in force before the last move
  double prev_max_ms = 0.0;                 // the slowest rank's time under them; 0 = no move to judge
  bool frozen = false;                      // a move made the step slower and was taken back: the shares stay where they are
  std::vector<double> weight;               // the shares in force as weights: what the group was made with, count / n after a move
};

enum : int { SHARES_KEEP = 0, SHARES_MOVE = 1, SHARES_TAKE_BACK = 2 };

// One decision: `cur` are the shares in force, ms[r] the time of rank r's force launch under them, cost(r, own) the relative cost of
// that launch if rank r owned `own` bodies (only ratios of one rank's values are used).  SHARES_KEEP, or *next = the shares to move
// to (SHARES_MOVE) or to go back to (SHARES_TAKE_BACK); < 0: an NBX_ERR_* with its text in *msg.
template <typename Cost>
int tune_shares(Tuner* t, const Shares& cur, int n, const double* ms, Cost&& cost, Shares* next, const char** msg) {
  const int P = cur.ranks;
  double cur_max = 0.0;
  for (int r = 0; r < P; ++r) cur_max = std::max(cur_max, ms[r]);
  const double prev_max = t->prev_max_ms;
  t->prev_max_ms = 0.0;  // on every path: one window judges one move
  *next = cur;
  const bool take_back = prev_max > 0.0 && cur_max > kTakeBackAbove * prev_max;
  if (take_back) {
    next->begin = t->prev_begin; next->count = t->prev_count;  // back to the shares that were faster
    t->frozen = true;
  } else {
    if (t->frozen) return SHARES_KEEP;
    std::vector<double> w((size_t)P);
    int rc = tune_weights(P, cur.count.data(), ms, w.data(), msg);
    if (rc) return rc;
    rc = weighted_shares(n, P, w.data(), next, msg);
    if (rc) return rc;
    // same shares, or the 256-record tiles allow no finer step
    if (next->ranks != P || next->n_alloc != cur.n_alloc || next->count == cur.count) return SHARES_KEEP;
    double predicted = 0.0;
    for (int r = 0; r < P; ++r) {
      const double now = cost(r, cur.count[r]), then = cost(r, next->count[r]);
      predicted = std::max(predicted, now > 0.0 ? ms[r] * then / now : ms[r]);
    }
    if (predicted > kMoveBelow * cur_max) return SHARES_KEEP;
    t->prev_begin = cur.begin; t->prev_count = cur.count; t->prev_max_ms = cur_max;
  }
  t->weight.assign((size_t)P, 0.0);
  for (int r = 0; r < P; ++r) t->weight[r] = (double)next->count[r] / (double)n;
  return take_back ? SHARES_TAKE_BACK : SHARES_MOVE;
}

}  // namespace nbx
#pragma GCC visibility pop
