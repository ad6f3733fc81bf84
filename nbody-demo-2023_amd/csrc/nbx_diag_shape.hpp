// nbx_diag_shape.hpp -- the launch-shape rule of the physics diagnostics (diag_splits) and the constants it reads.  Host-only:
// no HIP, no include at all, so that the device code (nbx_diag_body.hpp) and the host-only planner (nbx_plan.hpp:
// plan_ragged_diag) read ONE rule -- a context, the members of an ensemble and the members of a ragged ensemble of the same
// size get the same columns, j splits and tiles per split, hence the same partial rows and the same bits.
#pragma once

namespace nbx {

template <typename T> constexpr int kDiagBodies = 2;  // bodies per lane (fp32: one packed pair)
constexpr int kDiagTargetGroups = 1024;  // workgroups the j split aims at: 4 per CU of a 256-CU MI355X, 4 waves per SIMD
constexpr int kDiagMinSplitTiles = 4;    // a split sums at least this many 256-record tiles

// Number of j splits for `body_blocks` workgroup columns over `tiles` j tiles, and the tiles per split (every split
// non-empty).  A function of the state's size only -- never of the context's force options -- so every context holding a
// state sums it in the same order.
inline void diag_splits(int body_blocks, int tiles, int* splits, int* tiles_per_split) {
  int s = (kDiagTargetGroups + body_blocks - 1) / body_blocks;
  const int max_s = tiles / kDiagMinSplitTiles;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  const int per = (tiles + s - 1) / s;
  *tiles_per_split = per;
  *splits = (tiles + per - 1) / per;
}

}  // namespace nbx
