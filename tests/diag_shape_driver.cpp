// diag_shape_driver.cpp -- prints the launch shape of the physics diagnostics for every "i_count n" pair on the command line:
// columns = ceil(i_count / 512), tiles = ceil(n / 256) and diag_splits(columns, tiles) of csrc/nbx_diag_shape.hpp, one line
// "i_count n columns tiles splits tiles_per_split" each.  Built with g++ alone (the header includes nothing) by
// tests/test_large_shapes_cpu.py, which holds the lines against the Python restatement tests/potential_ref.py: diag_shape at
// sizes beyond those a batch member has (tests/ragged_diag_plan_driver.cpp walks every member size).
#include <cstdio>
#include <cstdlib>

#include "nbx_diag_shape.hpp"

static_assert(nbx::kDiagBodies<float> == 2 && nbx::kDiagBodies<double> == 2, "two bodies per lane: a column is 512 bodies");

int main(int argc, char** argv) {
  for (int k = 1; k + 1 < argc; k += 2) {
    const int i_count = std::atoi(argv[k]), n = std::atoi(argv[k + 1]);
    const int columns = (i_count + 511) / 512, tiles = (n + 255) / 256;
    int splits = 0, per = 0;
    nbx::diag_splits(columns, tiles, &splits, &per);
    std::printf("%d %d %d %d %d %d\n", i_count, n, columns, tiles, splits, per);
  }
  return 0;
}
