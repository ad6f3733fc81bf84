// nbx_field_shape.hpp -- the launch-shape rule of the field at caller-supplied points (include/nbx_field.h).  Host-only in the
// sense of nbx_diag_shape.hpp: no HIP, no include at all.  Written as constexpr so that the ragged kernel and the finish kernel
// (nbx_field_kernels.hpp) evaluate the SAME rule on the device that the host evaluates for a context and for an ensemble.
//
// A function of (m, n) alone -- the points of one system and its bodies -- never of the CU count or of an object's options: the
// same state, the same points and the same m give the same columns, j splits and tiles per split, hence the same partial rows
// and the same bits, on every object that holds them.  Splits and tiles per split follow diag_splits (nbx_diag_shape.hpp): aim
// at kFieldTargetGroups workgroups, a split sums at least kFieldMinSplitTiles tiles, every split non-empty.
#pragma once

namespace nbx {

template <typename T> constexpr int kFieldPoints = 2;  // points per lane (fp32: one packed pair)
constexpr int kFieldBlock = 256;                       // = kBlock: threads per workgroup
constexpr int kFieldTile = 256;                        // = kTile: j records per LDS tile
constexpr int kFieldColumn = kFieldBlock * 2;          // points per workgroup column
constexpr int kFieldTargetGroups = 1024;               // = kDiagTargetGroups
constexpr int kFieldMinSplitTiles = 4;                 // = kDiagMinSplitTiles
constexpr long long kFieldMaxPoints = 1ll << 22;       // per call: count * m (include/nbx_field.h, status 5)

struct FieldShape {
  int columns;          // workgroup columns: ceil(m / 512)
  int tiles;            // j tiles: ceil(n / 256)
  int splits;           // j splits, every one non-empty
  int tiles_per_split;  // tiles of every split but possibly the last
};

constexpr FieldShape field_shape(int m, int n) {
  const int columns = (m + kFieldColumn - 1) / kFieldColumn;
  const int tiles = (n + kFieldTile - 1) / kFieldTile;
  int s = (kFieldTargetGroups + columns - 1) / columns;
  const int max_s = tiles / kFieldMinSplitTiles;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  const int per = (tiles + s - 1) / s;
  return FieldShape{columns, tiles, (tiles + per - 1) / per, per};
}

}  // namespace nbx
