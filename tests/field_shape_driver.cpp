// field_shape_driver.cpp -- prints field_shape(m, n) of csrc/nbx_field_shape.hpp for every "m n" pair on the command line, one
// line "m n columns tiles splits tiles_per_split" each.  Built with g++ alone (the header includes nothing) by
// tests/test_field_cpu.py, which holds the lines against the Python restatement tests/field_ref.py: field_shape.
#include <cstdio>
#include <cstdlib>

#include "nbx_field_shape.hpp"

static_assert(nbx::field_shape(1, 1).splits == 1 && nbx::field_shape(513, 16383).columns == 2, "usable in a constant expression");
static_assert(nbx::kFieldPoints<float> == 2 && nbx::kFieldPoints<double> == 2 && nbx::kFieldColumn == 512, "two points per lane");

int main(int argc, char** argv) {
  for (int k = 1; k + 1 < argc; k += 2) {
    const int m = std::atoi(argv[k]), n = std::atoi(argv[k + 1]);
    const nbx::FieldShape s = nbx::field_shape(m, n);
    std::printf("%d %d %d %d %d %d\n", m, n, s.columns, s.tiles, s.splits, s.tiles_per_split);
  }
  std::printf("max_points %lld\n", nbx::kFieldMaxPoints);
  return 0;
}
