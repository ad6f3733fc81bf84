// nbx_nlist_kernels.hpp -- the kernels of nbx_nlist, nbx_ensemble_nlist and nbx_ragged_nlist (include/nbx_nlist.h): for every
// body i of a system of n bodies the list of all j < n, j != i with
//     r2(i, j) = |x_j - x_i|^2 + eps^2 <= h2
// in ascending j, with their r2, lists end to end at offsets[].  Instantiated by nbx_nlist.hip alone.
//
// The size of the result depends on the state, so the pair work runs twice around a prefix sum:
//   nlist_kernel<T, FILL>            grid (columns, splits), block 256          a context (sliced or not: every position is resident)
//   ensemble_nlist_kernel<T, FILL>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_nlist_kernel<T, FILL>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads
//                                    its member's {pos_off, out_off, n} from the table, evaluates field_shape(n, n) itself and
//                                    returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three run nl_body, nbx_neighbours' loop: 256 threads, two bodies per lane, the j range of the workgroup's split in
//     256-record tiles staged in LDS (one array, read whole), the next tile prefetched into registers, masked and unmasked tile
//     loops.  FILL == false, the count pass: per pair the r2 arithmetic, one compare and one add, and per (split, body) the
//     segment record {0, hits}.  FILL == true, the fill pass: the same loop, the same compare on the same bits (nl_in serves
//     both), and behind a wave-wide __any() the stores of (j, r2) at the lane's write position, which starts at
//     offsets[body] + the segment's start and advances on every hit.
//   nlist_finish_kernel              one thread per body of the call: walks the body's segments in ascending split order, writes
//                                    every segment's start relative to the body's own offset and the body's total, within[b]
//   nlist_scan_sums_kernel, nlist_scan_blocks_kernel, nlist_scan_apply_kernel
//                                    offsets[] = the exclusive prefix sum of within[] in 64 bits, two levels of 2048
//                                    (nbx_nlist_shape.hpp); offsets[bodies] = the total
//
// Splits are ascending ranges of j, j ascends within a split and a lane walks its own body's pairs in that order: every list
// comes out in ascending j without a sort.  Every store is guarded by the end of its segment, so that a disagreement between the
// two passes would show as a wrong list and never as a write outside the lists.  No atomics; no kernel waits for another
// workgroup.  Nothing is summed in floating point.
//
// The mask is nbx_neighbours': a pair is dropped EXACTLY where j == i or j >= n.  Only tiles that meet the workgroup's own bodies
// or reach past n run the masked loop.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_nlist_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");
static_assert(kNlScanThreads == kBlock, "a scan block is one workgroup of kBlock threads");
static_assert(kNlMaxBodies == kFieldMaxPoints, "the bound of nbx_field.h");

constexpr int kNlBodies = 2;  // bodies per lane (fp32: one packed pair)

// a (split, body) segment of a list: where it begins, relative to the body's own offset (written by the finish kernel), and how
// many entries it has (written by the count pass)
struct NlSegment {
  int start;
  int hits;
};

// where the fill pass writes.  pos and end fit 32 bits: a fill runs only where the total is at most the capacity, at most 2^28.
template <typename T>
struct NlLists {
  const long long* offsets;  // [bodies of the call + 1]
  int* index;                // [total]
  T* r2;                     // [total]
};

// the decision both passes share.  MASK: the pair may be the body itself or a record at or beyond n (jg: the record's index,
// uniform over the wave).
template <typename T, bool MASK>
__device__ __forceinline__ bool nl_in(const T r2, const int jg, const int n, const int ig, const T h2) {
  bool in = r2 <= h2;
  if constexpr (MASK) in = in && jg < n && jg != ig;
  return in;
}

// a hit of the fill pass
template <typename T>
__device__ __forceinline__ void nl_put(const bool in, const int jg, const T r2, unsigned& pos, const unsigned end, const NlLists<T>& out) {
  if (in) {
    if (pos < end) {
      out.index[pos] = jg;
      out.r2[pos] = r2;
    }
    ++pos;
  }
}

// One LDS tile against the lane's B bodies (j_glob: index of tile record 0 in its system).
template <typename T, int B, bool MASK, bool FILL>
__device__ __forceinline__ void nl_tile(const typename V4<T>::type* tile, const int j_glob, const int n, const T (&xi)[B], const T (&yi)[B],
                                        const T (&zi)[B], const int (&ig)[B], const T h2, int (&cnt)[B], unsigned (&pos)[B],
                                        const unsigned (&end)[B], const NlLists<T>& out) {
  if constexpr (sizeof(T) == 4 && B == 2) {
    const f32x2 px = {xi[0], xi[1]}, py = {yi[0], yi[1]}, pz = {zi[0], zi[1]};
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = whole_record(tile, j);
      const int jg = j_glob + j;
      const f32x2 dx = f32x2{r.x, r.x} - px, dy = f32x2{r.y, r.y} - py, dz = f32x2{r.z, r.z} - pz;
      f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
      r2 = __builtin_elementwise_fma(dy, dy, r2);
      r2 = __builtin_elementwise_fma(dx, dx, r2);
      const bool in0 = nl_in<float, MASK>(r2.x, jg, n, ig[0], h2), in1 = nl_in<float, MASK>(r2.y, jg, n, ig[1], h2);
      if constexpr (!FILL) {
        cnt[0] += in0 ? 1 : 0;
        cnt[1] += in1 ? 1 : 0;
      } else {
        if (__any(in0 || in1)) {  // uniform over the wave
          nl_put<float>(in0, jg, r2.x, pos[0], end[0], out);
          nl_put<float>(in1, jg, r2.y, pos[1], end[1], out);
        }
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = tile[j];
      const int jg = j_glob + j;
      T c[B];
      bool in[B], some = false;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const T dx = r.x - xi[b], dy = r.y - yi[b], dz = r.z - zi[b];
        c[b] = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
        in[b] = nl_in<T, MASK>(c[b], jg, n, ig[b], h2);
        some = some || in[b];
        if constexpr (!FILL) cnt[b] += in[b] ? 1 : 0;
      }
      if constexpr (FILL) {
        if (__any(some)) {  // uniform over the wave
#pragma unroll
          for (int b = 0; b < B; ++b) nl_put<T>(in[b], jg, c[b], pos[b], end[b], out);
        }
      }
    }
  }
}

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding).  seg: the system's segment rows, record split * n + body.
// out.offsets: the system's first body.  The count pass writes the segments of the column's bodies below n; the fill pass reads
// them and writes list entries only.
template <typename T, int B, bool FILL>
__device__ __forceinline__ void nl_body(const typename V4<T>::type* __restrict__ posm, const int n, const int tiles_per_split, const T h2,
                                        NlSegment* __restrict__ seg, const NlLists<T> out, const int col, const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[B], yi[B], zi[B];
  int ig[B], cnt[B];
  unsigned pos[B], end[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < n) p = posm[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ig[b] = li;
    cnt[b] = 0;
    pos[b] = end[b] = 0u;  // a lane without a body stores nothing
    if constexpr (FILL) {
      if (li < n) {
        const NlSegment s = seg[(size_t)split * (size_t)n + (size_t)li];
        pos[b] = (unsigned)(out.offsets[li] + (long long)s.start);
        end[b] = pos[b] + (unsigned)s.hits;
      }
    }
  }
  const int g_lo = l0, g_hi = min(l0 + kBlock * B, n);  // the workgroup's bodies: a tile that meets them runs the masked loop
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  T4 next = zero;
  if (k0 < k1) next = posm[k0 * kTile + t];
  for (int k = k0; k < k1; ++k) {
    __syncthreads();  // every lane is done with the previous tile
    tile[t] = next;
    __syncthreads();
    if (k + 1 < k1) next = posm[(k + 1) * kTile + t];
    const int j0 = k * kTile;
    if ((j0 < g_hi && j0 + kTile > g_lo) || j0 + kTile > n)
      nl_tile<T, B, true, FILL>(tile, j0, n, xi, yi, zi, ig, h2, cnt, pos, end, out);
    else
      nl_tile<T, B, false, FILL>(tile, j0, n, xi, yi, zi, ig, h2, cnt, pos, end, out);
  }
  if constexpr (!FILL) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int li = l0 + b * kBlock + t;
      if (li < n) seg[(size_t)split * (size_t)n + (size_t)li] = NlSegment{0, cnt[b]};
    }
  }
}

template <typename T, bool FILL>
__global__ __launch_bounds__(kBlock) void nlist_kernel(const typename V4<T>::type* __restrict__ posm, int n, int tiles_per_split, T h2,
                                                       NlSegment* __restrict__ seg, const NlLists<T> out) {
  nl_body<T, kNlBodies, FILL>(posm, n, tiles_per_split, h2, seg, out, blockIdx.x, blockIdx.y);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread]; seg[count][gridDim.y][n].
template <typename T>
struct EnsembleNlArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  NlSegment* seg;                    // the segment rows of member `first`
  T h2;
  unsigned first;       // member of blockIdx.z == 0
  unsigned pos_stride;  // records between members in posm
  int n, tiles_per_split;
};

template <typename T, bool FILL>
__global__ __launch_bounds__(kBlock) void ensemble_nlist_kernel(const EnsembleNlArgs<T> e, const NlLists<T> out) {
  const size_t k = blockIdx.z;
  NlLists<T> mine = out;
  mine.offsets = out.offsets + k * (size_t)e.n;
  nl_body<T, kNlBodies, FILL>(e.posm + (e.first + k) * e.pos_stride, e.n, e.tiles_per_split, e.h2, e.seg + k * gridDim.y * (size_t)e.n, mine,
                              blockIdx.x, blockIdx.y);
}

struct NlMember : OutMember {};

template <typename T>
struct RaggedNlArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const NlMember* table;             // [members]
  NlSegment* seg;                    // the segment rows of member `first`
  T h2;
  unsigned first;  // member of blockIdx.z == 0
};

template <typename T, bool FILL>
__global__ __launch_bounds__(kBlock) void ragged_nlist_kernel(const RaggedNlArgs<T> r, const NlLists<T> out) {
  const MemberGroup<NlMember> g = member_group(r.table, r.first);
  if (g.elsewhere()) return;
  const size_t rel = g.rel();
  NlLists<T> mine = out;
  mine.offsets = out.offsets + rel;
  nl_body<T, kNlBodies, FILL>(r.posm + g.mem.pos_off, g.mem.n, g.shape.tiles_per_split, r.h2, r.seg + rel * gridDim.y, mine, blockIdx.x,
                              blockIdx.y);
}

// Body idx of the call's `total` bodies, its member found by member_at..  The member has field_shape(n, n).splits rows of n
// segments; its rows begin at (the bodies of the range before it) * row_splits, row_splits the gridDim.y of the pair-work
// launch.
__global__ __launch_bounds__(kBlock) void nlist_finish_kernel(NlSegment* __restrict__ seg, const NlMember* __restrict__ table, unsigned first,
                                                              int count, int n_all, int row_splits, unsigned total,
                                                              long long* __restrict__ within) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const MemberAt at = member_at(table, first, count, n_all, idx);
  const int n = at.n;
  const size_t rel = at.rel;  // the bodies of the range before the body's member
  const int splits = field_shape(n, n).splits;
  NlSegment* row = seg + rel * (size_t)row_splits + ((size_t)idx - rel);
  int sum = 0;  // below n <= 2^22
  for (int s = 0; s < splits; ++s) {
    NlSegment* v = row + (size_t)s * (size_t)n;
    v->start = sum;
    sum += v->hits;
  }
  within[idx] = (long long)sum;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the exclusive prefix sum of 64-bit values, two levels of kNlScanBlock (nbx_nlist_shape.hpp)
// ---------------------------------------------------------------------------------------------------------------------------
// The kNlScanThreads thread sums of a workgroup: returns the sum of the threads before this one; *all: of every thread.
__device__ __forceinline__ long long nl_scan_threads(const long long mine, long long* all) {
  __shared__ long long lds[kNlScanThreads];
  const int t = threadIdx.x;
  lds[t] = mine;
  __syncthreads();
  for (int d = 1; d < kNlScanThreads; d <<= 1) {
    const long long below = t >= d ? lds[t - d] : 0ll;
    __syncthreads();
    lds[t] += below;
    __syncthreads();
  }
  const long long upto = lds[t];
  *all = lds[kNlScanThreads - 1];
  return upto - mine;
}

// the thread's kNlScanItems consecutive values of v[0 .. count), zero beyond
__device__ __forceinline__ void nl_scan_load(const long long* __restrict__ v, const long long count, const long long at,
                                             long long (&x)[kNlScanItems]) {
#pragma unroll
  for (int q = 0; q < kNlScanItems; ++q) x[q] = at + q < count ? v[at + q] : 0ll;
}

// launch one: sums[blockIdx.x] = the sum of the block's values
__global__ __launch_bounds__(kNlScanThreads) void nlist_scan_sums_kernel(const long long* __restrict__ within, long long bodies,
                                                                        long long* __restrict__ sums) {
  long long x[kNlScanItems];
  nl_scan_load(within, bodies, (long long)blockIdx.x * kNlScanBlock + (long long)threadIdx.x * kNlScanItems, x);
  long long mine = 0;
#pragma unroll
  for (int q = 0; q < kNlScanItems; ++q) mine += x[q];
  long long all;
  (void)nl_scan_threads(mine, &all);
  if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// launch two, ONE workgroup: sums[0 .. blocks) become their exclusive prefix sums, *total their sum.  blocks <= kNlScanBlock.
__global__ __launch_bounds__(kNlScanThreads) void nlist_scan_blocks_kernel(long long* __restrict__ sums, int blocks, long long* __restrict__ total) {
  const long long at = (long long)threadIdx.x * kNlScanItems;
  long long x[kNlScanItems];
  nl_scan_load(sums, (long long)blocks, at, x);
  long long mine = 0;
#pragma unroll
  for (int q = 0; q < kNlScanItems; ++q) mine += x[q];
  long long all;
  long long run = nl_scan_threads(mine, &all);
#pragma unroll
  for (int q = 0; q < kNlScanItems; ++q) {
    if (at + q < blocks) sums[at + q] = run;
    run += x[q];
  }
  if (threadIdx.x == 0) *total = all;
}

// launch three: offsets[b] = the block's prefix + the values of the block before b
__global__ __launch_bounds__(kNlScanThreads) void nlist_scan_apply_kernel(const long long* __restrict__ within, long long bodies,
                                                                         const long long* __restrict__ sums, long long* __restrict__ offsets) {
  const long long at = (long long)blockIdx.x * kNlScanBlock + (long long)threadIdx.x * kNlScanItems;
  long long x[kNlScanItems];
  nl_scan_load(within, bodies, at, x);
  long long mine = 0;
#pragma unroll
  for (int q = 0; q < kNlScanItems; ++q) mine += x[q];
  long long all;
  long long run = sums[blockIdx.x] + nl_scan_threads(mine, &all);
#pragma unroll
  for (int q = 0; q < kNlScanItems; ++q) {
    if (at + q < bodies) offsets[at + q] = run;
    run += x[q];
  }
}

}  // namespace nbx
