// nlist_shape_driver.cpp -- prints, for every body count on the command line, one line "bodies blocks block_of_last
// place_of_last" from csrc/nbx_nlist_shape.hpp, then the constants.  Built with g++ alone (the header includes nothing) by
// tests/test_nlist_cpu.py, which holds the lines against the Python restatement tests/nlist_ref.py: scan.
#include <cstdio>
#include <cstdlib>

#include "nbx_nlist_shape.hpp"

static_assert(nbx::nl_scan_blocks(1) == 1 && nbx::nl_scan_blocks(2048) == 1 && nbx::nl_scan_blocks(2049) == 2, "usable in a constant expression");
static_assert(nbx::nl_scan_blocks(nbx::kNlMaxBodies) == nbx::kNlScanBlock, "two levels serve the largest call");

int main(int argc, char** argv) {
  for (int k = 1; k < argc; ++k) {
    const long long bodies = std::atoll(argv[k]);
    std::printf("%lld %d %d %d\n", bodies, nbx::nl_scan_blocks(bodies), nbx::nl_scan_block_of(bodies - 1), nbx::nl_scan_place_of(bodies - 1));
  }
  std::printf("block %d threads %d items %d max_bodies %lld max_capacity %lld first_guess %d\n", nbx::kNlScanBlock, nbx::kNlScanThreads,
              nbx::kNlScanItems, nbx::kNlMaxBodies, nbx::kNlMaxCapacity, nbx::kNlFirstGuess);
  return 0;
}
