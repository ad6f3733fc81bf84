// nbx_neighbours_kernels.hpp -- the kernels of nbx_neighbours, nbx_ensemble_neighbours and nbx_ragged_neighbours
// (include/nbx_neighbours.h): for every body i of a system of n bodies the partner j < n, j != i with the smallest
//     r2(i, j) = |x_j - x_i|^2 + eps^2
// (the lowest j among equal bit patterns), that r2, and the number of partners with r2(i, j) <= h2.  Instantiated by
// nbx_neighbours.hip alone.
//
//   neighbour_kernel<T, COUNT>            grid (columns, splits), block 256          a context (sliced or not: every position is resident)
//   ensemble_neighbour_kernel<T, COUNT>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_neighbour_kernel<T, COUNT>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads
//                                         its member's {pos_off, out_off, n} from the table, evaluates field_shape(n, n) itself and
//                                         returns at once where blockIdx.x or blockIdx.y is not one of its member's; no work list
//     All three run nb_body: 256 threads, two bodies per lane (the i side: the column's own position records), the j range of the
//     workgroup's split in 256-record tiles staged in LDS (ONE array, the position records, read whole), the next tile prefetched
//     into registers.  Columns, splits and tiles per split are field_shape(n, n) (nbx_field_shape.hpp): a performance choice only,
//     nothing below depends on it.  COUNT: the radius count is asked for; the other form does not compile its compare and add.
//   neighbour_finish_kernel<T>            one thread per body of the call: walks the body's split records in ascending order, takes
//                                         a split's candidate only on strict <, adds the counts, writes {r2, j, count}
//
// One pair, in T (the fp32 tile loop is the same operations on the lane's two bodies per packed instruction: 3 packed subtracts
// and 3 packed fma per two pairs; no reciprocal square root, no multiply):
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))           the force kernels' and ts_pair's r2
//   if (r2 < best) { best = r2; index = j; }         j ascends within a split and the compare is strict: the lowest j wins
//   count += r2 <= h2
// j is uniform over the wave, so the index operand of the select is a scalar.
//
// The mask: a pair is dropped EXACTLY where j == i or j >= n -- it is neither a candidate nor counted.  A padding record sits at
// the origin and would otherwise be somebody's nearest neighbour.  Only tiles that meet the workgroup's own bodies or reach past n
// run the masked loop; every other tile runs the loop without the mask compares (nb_tile<..., MASK>, as ts_tile).
//
// A minimum with a lowest-index tie-break and an integer sum do not depend on the order they are taken in: the three values are
// the same bits for every launch shape, and a member's are a lone context's.  parts[member of the range][split][body] records
// {r2, j, count}, a member's rows together; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kNbBodies = 2;                       // bodies per lane (fp32: one packed pair)
constexpr long long kNbMaxBodies = kFieldMaxPoints;  // per call (include/nbx_neighbours.h, status 4)

// what a (split, body) leaves behind, and what the finish kernel writes per body: j == -1, r2 == +inf, count == 0 where the
// body met no partner
template <typename T>
struct NbRecord {
  T r2;
  int j;
  int count;
};

template <typename T> __device__ __forceinline__ T nb_inf() { return (T)__builtin_huge_valf(); }

// one pair against the running minimum, its index and the count.  MASK: the pair may be the body itself or a record at or
// beyond n (jg: the record's index, uniform over the wave).
template <typename T, bool MASK, bool COUNT>
__device__ __forceinline__ void nb_take(const T r2, const int jg, const int n, const int ig, const T h2, T& best, int& bj, int& cnt) {
  bool lt = r2 < best;
  bool in = r2 <= h2;
  if constexpr (MASK) {
    const bool ok = jg < n && jg != ig;
    lt = lt && ok;
    in = in && ok;
  }
  best = lt ? r2 : best;
  bj = lt ? jg : bj;
  if constexpr (COUNT) cnt += in ? 1 : 0;
}

// One LDS tile against the lane's B bodies (j_glob: global index of tile record 0).
template <typename T, int B, bool MASK, bool COUNT>
__device__ __forceinline__ void nb_tile(const typename V4<T>::type* tile, const int j_glob, const int n, const T (&xi)[B], const T (&yi)[B],
                                        const T (&zi)[B], const int (&ig)[B], const T h2, T (&best)[B], int (&bj)[B], int (&cnt)[B]) {
  if constexpr (sizeof(T) == 4 && B % 2 == 0) {
    f32x2 px[B / 2], py[B / 2], pz[B / 2];
#pragma unroll
    for (int h = 0; h < B / 2; ++h) {
      px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
      py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
      pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
    }
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = whole_record(tile, j);
      const int jg = j_glob + j;
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        const f32x2 dx = f32x2{r.x, r.x} - px[h], dy = f32x2{r.y, r.y} - py[h], dz = f32x2{r.z, r.z} - pz[h];
        f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        r2 = __builtin_elementwise_fma(dx, dx, r2);
        nb_take<float, MASK, COUNT>(r2.x, jg, n, ig[2 * h], h2, best[2 * h], bj[2 * h], cnt[2 * h]);
        nb_take<float, MASK, COUNT>(r2.y, jg, n, ig[2 * h + 1], h2, best[2 * h + 1], bj[2 * h + 1], cnt[2 * h + 1]);
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = tile[j];
      const int jg = j_glob + j;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const T dx = r.x - xi[b], dy = r.y - yi[b], dz = r.z - zi[b];
        const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
        nb_take<T, MASK, COUNT>(r2, jg, n, ig[b], h2, best[b], bj[b], cnt[b]);
      }
    }
  }
}

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding).  Writes, for every body below n of the column, record
// split * n + body of parts.
template <typename T, int B, bool COUNT>
__device__ __forceinline__ void nb_body(const typename V4<T>::type* __restrict__ posm, const int n, const int tiles_per_split, const T h2,
                                        NbRecord<T>* __restrict__ parts, const int col, const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[B], yi[B], zi[B], best[B];
  int ig[B], bj[B], cnt[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < n) p = posm[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ig[b] = li;
    best[b] = nb_inf<T>();
    bj[b] = -1;
    cnt[b] = 0;
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
    if (tile_masked(j0, g_lo, g_hi, n))
      nb_tile<T, B, true, COUNT>(tile, j0, n, xi, yi, zi, ig, h2, best, bj, cnt);
    else
      nb_tile<T, B, false, COUNT>(tile, j0, n, xi, yi, zi, ig, h2, best, bj, cnt);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) {
      NbRecord<T> o;
      o.r2 = best[b]; o.j = bj[b]; o.count = cnt[b];
      parts[(size_t)split * (size_t)n + (size_t)li] = o;
    }
  }
}

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlock) void neighbour_kernel(const typename V4<T>::type* __restrict__ posm, int n, int tiles_per_split, T h2,
                                                           NbRecord<T>* __restrict__ parts) {
  nb_body<T, kNbBodies, COUNT>(posm, n, tiles_per_split, h2, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread]; parts[count][gridDim.y][n].
template <typename T>
struct EnsembleNbArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  NbRecord<T>* parts;                // the partial rows of member `first`
  T h2;
  unsigned first;       // member of blockIdx.z == 0
  unsigned pos_stride;  // records between members in posm
  int n, tiles_per_split;
};

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlock) void ensemble_neighbour_kernel(const EnsembleNbArgs<T> e) {
  const size_t k = blockIdx.z;
  nb_body<T, kNbBodies, COUNT>(e.posm + (e.first + k) * e.pos_stride, e.n, e.tiles_per_split, e.h2, e.parts + k * gridDim.y * (size_t)e.n,
                               blockIdx.x, blockIdx.y);
}

struct NbMember : OutMember {};

template <typename T>
struct RaggedNbArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const NbMember* table;             // [members]
  NbRecord<T>* parts;                // the partial rows of member `first`
  T h2;
  unsigned first;  // member of blockIdx.z == 0
};

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlock) void ragged_neighbour_kernel(const RaggedNbArgs<T> r) {
  const MemberGroup<NbMember> g = member_group(r.table, r.first);
  if (g.elsewhere()) return;
  nb_body<T, kNbBodies, COUNT>(r.posm + g.mem.pos_off, g.mem.n, g.shape.tiles_per_split, r.h2, r.parts + g.rel() * gridDim.y, blockIdx.x,
                               blockIdx.y);
}

// Body idx of the call's `total` bodies, its member found by member_at..  The member has field_shape(n, n).splits rows of n
// records; its rows begin at (the bodies of the range before it) * row_splits, row_splits the gridDim.y of the pair-work
// launch.
template <typename T>
__global__ __launch_bounds__(kBlock) void neighbour_finish_kernel(const NbRecord<T>* __restrict__ parts, const NbMember* __restrict__ table,
                                                                  unsigned first, int count, int n_all, int row_splits, unsigned total,
                                                                  NbRecord<T>* __restrict__ out) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const MemberAt at = member_at(table, first, count, n_all, idx);
  const int n = at.n;
  const size_t rel = at.rel;  // the bodies of the range before the body's member
  const int splits = field_shape(n, n).splits;
  const NbRecord<T>* row = parts + rel * (size_t)row_splits + ((size_t)idx - rel);
  NbRecord<T> o;
  o.r2 = nb_inf<T>(); o.j = -1; o.count = 0;
  for (int s = 0; s < splits; ++s) {
    const NbRecord<T> v = row[(size_t)s * (size_t)n];
    if (v.r2 < o.r2) { o.r2 = v.r2; o.j = v.j; }
    o.count += v.count;
  }
  out[idx] = o;
}

}  // namespace nbx
