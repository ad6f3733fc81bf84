// nbx_nlist_shape.hpp -- the sizes of the neighbour lists' device prefix sum (include/nbx_nlist.h).  Host-only in the sense of
// nbx_field_shape.hpp: no HIP, no include at all, constexpr throughout, so that the kernels (nbx_nlist_kernels.hpp), the host
// (nbx_nlist.hip) and a plain C++ test driver read the same numbers.
//
// The scan turns within[b], the length of body b's list, into offsets[b], where the list begins: an exclusive prefix sum in 64
// bits over the bodies of the call.  It has two levels.  A scan block is kNlScanBlock = 2048 consecutive bodies, 256 threads of 8;
// launch one writes every block's sum, launch two scans the block sums in ONE workgroup of the same shape, launch three adds a
// block's prefix to its bodies' own prefixes.  One workgroup scans at most 2048 values, so two levels serve 2048 * 2048 bodies:
// exactly the 2^22 a call may hold.  No kernel waits for another workgroup; the order is the stream's.
#pragma once

namespace nbx {

constexpr int kNlScanThreads = 256;                               // = kBlock
constexpr int kNlScanItems = 8;                                   // consecutive values per thread
constexpr int kNlScanBlock = kNlScanThreads * kNlScanItems;       // bodies per scan block
constexpr long long kNlMaxBodies = 1ll << 22;                     // per call (include/nbx_nlist.h, status 6) = kFieldMaxPoints
constexpr long long kNlMaxCapacity = 1ll << 28;                   // entries (status 3): 2^28 * (4 + 8) bytes = 3 GiB of lists in fp64
constexpr int kNlFirstGuess = 16;                                 // entries per body nbx.py's nlist() tries before it asks again

// scan blocks of a call of `bodies` bodies: the grid of launches one and three, the values of launch two
constexpr int nl_scan_blocks(long long bodies) { return (int)((bodies + kNlScanBlock - 1) / kNlScanBlock); }
// the scan block of body b and its place in it
constexpr int nl_scan_block_of(long long b) { return (int)(b / kNlScanBlock); }
constexpr int nl_scan_place_of(long long b) { return (int)(b % kNlScanBlock); }

static_assert(kNlScanBlock == 2048, "256 threads of 8");
static_assert(nl_scan_blocks(kNlMaxBodies) == kNlScanBlock, "2^22 bodies are exactly 2048 blocks of 2048: one workgroup scans the block sums");
static_assert(nl_scan_blocks(kNlMaxBodies) <= kNlScanBlock, "two levels suffice for every call that passes the bound");
static_assert(kNlMaxCapacity * 12 == 3ll << 30, "index and fp64 r2 of a full list are 3 GiB");

}  // namespace nbx
