// nbx_knn_kernels.hpp -- the kernels of nbx_knn, nbx_ensemble_knn and nbx_ragged_knn (include/nbx_knn.h): for every body i of a
// system of n bodies the k partners j < n, j != i that are smallest under the order (r2 bits, j),
//     r2(i, j) = |x_j - x_i|^2 + eps^2,
// ascending, with their r2.  Instantiated by nbx_knn.hip alone.
//
//   knn_kernel<T, K>            grid (columns, splits), block 256          a context (sliced or not: every position is resident)
//   ensemble_knn_kernel<T, K>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_knn_kernel<T, K>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads its
//                               member's {pos_off, out_off, n} from the table, evaluates field_shape(n, n) itself and returns at
//                               once where blockIdx.x or blockIdx.y is not one of its member's; no work list
//     All three run knn_body: 256 threads, two bodies per lane (the i side: the column's own position records), the j range of
//     the workgroup's split in 256-record tiles staged in LDS (ONE array, the position records, read whole), the next tile
//     prefetched into registers.  Columns, splits and tiles per split are field_shape(n, n) (nbx_field_shape.hpp): a performance
//     choice only, nothing below depends on it.
//   knn_finish_kernel<T, K>     one thread per body of the call: merges the body's split rows in ascending split order into
//                               the final k entries
//
// K is a compiled list capacity (4, 8 or 16), k <= K the width asked for: a lane keeps, per body, its K best (r2, j) sorted
// ascending in registers -- every index into the list is a compile-time constant, so nothing goes to scratch -- and a (split,
// body) leaves the first k behind.  The first k of the K best are the k best, so the capacity does not show in the result.
//
// One pair, in T (the fp32 tile loop is the same operations on the lane's two bodies per packed instruction: 3 packed subtracts
// and 3 packed fma per two pairs; no reciprocal square root, no multiply):
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))           nbx_neighbours' r2, restated here
//   fast path:  r2 < r[K - 1], ONE strict compare against the body's current K-th value
//   slow path:  knn_insert, a compare and a conditional shift per slot, unrolled -- under a wave-uniform branch: the condition is
//               __any() of the lanes' compares, so a wave none of whose lanes has a candidate skips the block as a whole
// j ascends within a split and every compare is strict, so an equal r2 with a higher j never displaces an entry: the list is
// in (r2, j) order.  knn_insert of a value that is not below r[K - 1] changes nothing, so lanes without a candidate may run it
// along with the lane that has one.
//
// The mask: a pair is dropped EXACTLY where j == i or j >= n, by turning its r2 into +infinity, which no strict compare passes.
// A padding record sits at the origin and would otherwise be somebody's neighbour.  Only tiles that meet the workgroup's own
// bodies or reach past n run the masked loop; every other tile runs the loop without the mask compares (knn_tile<..., MASK>).
//
// A selection under a total order does not depend on the order the candidates come in: the rows are the same bits for every
// launch shape and capacity, and a member's are a lone context's.  parts[member of the range][split][body][k] records {r2, j},
// a member's rows together, entries never reached {+inf, -1}; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kKnnBodies = 2;                          // bodies per lane (fp32: one packed pair), every (T, capacity)
constexpr int kKnnMax = 16;                            // NBX_KNN_MAX: the largest compiled capacity
constexpr long long kKnnMaxEntries = kFieldMaxPoints;  // bodies * k per call (include/nbx_knn.h, status 4)

// the smallest compiled capacity that holds k
constexpr int knn_capacity(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : 16; }

// an entry of a partial row and of a result row
template <typename T>
struct KnnRecord {
  T r2;
  int j;
};

template <typename T> __device__ __forceinline__ T knn_inf() { return (T)__builtin_huge_valf(); }

// (c, jg) into the ascending list (r, jx): slot q takes its lower neighbour where c is below that one, c where c is below the
// slot's own value alone, and stays otherwise; from the top down, so that every slot reads its neighbour's old value.  The last
// entry falls out.  Strict compares: c goes behind every entry equal to it.
template <typename T, int K>
__device__ __forceinline__ void knn_insert(const T c, const int jg, T (&r)[K], int (&jx)[K]) {
#pragma unroll
  for (int q = K - 1; q >= 0; --q) {
    const bool here = c < r[q];
    bool below = false;
    if (q > 0) below = c < r[q - 1];
    r[q] = below ? r[q > 0 ? q - 1 : 0] : (here ? c : r[q]);
    jx[q] = below ? jx[q > 0 ? q - 1 : 0] : (here ? jg : jx[q]);
  }
}

// One LDS tile against the lane's B bodies (j_glob: global index of tile record 0).  MASK: a pair may be the body itself or a
// record at or beyond n.
template <typename T, int K, int B, bool MASK>
__device__ __forceinline__ void knn_tile(const typename V4<T>::type* tile, const int j_glob, const int n, const T (&xi)[B], const T (&yi)[B],
                                         const T (&zi)[B], const int (&ig)[B], T (&r)[B][K], int (&jx)[B][K]) {
  if constexpr (sizeof(T) == 4 && B == 2) {
    const f32x2 px = {xi[0], xi[1]}, py = {yi[0], yi[1]}, pz = {zi[0], zi[1]};
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 rec = whole_record(tile, j);
      const int jg = j_glob + j;
      const f32x2 dx = f32x2{rec.x, rec.x} - px, dy = f32x2{rec.y, rec.y} - py, dz = f32x2{rec.z, rec.z} - pz;
      f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
      r2 = __builtin_elementwise_fma(dy, dy, r2);
      r2 = __builtin_elementwise_fma(dx, dx, r2);
      float c0 = r2.x, c1 = r2.y;
      if constexpr (MASK) {
        c0 = (jg < n && jg != ig[0]) ? c0 : knn_inf<float>();
        c1 = (jg < n && jg != ig[1]) ? c1 : knn_inf<float>();
      }
      const bool t0 = c0 < r[0][K - 1], t1 = c1 < r[1][K - 1];
      if (__any(t0 || t1)) {  // uniform over the wave
        if (__any(t0)) knn_insert<float, K>(c0, jg, r[0], jx[0]);
        if (__any(t1)) knn_insert<float, K>(c1, jg, r[1], jx[1]);
      }
    }
  } else {
#pragma unroll 2
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type rec = tile[j];
      const int jg = j_glob + j;
      T c[B];
      bool some = false;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const T dx = rec.x - xi[b], dy = rec.y - yi[b], dz = rec.z - zi[b];
        c[b] = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
        if constexpr (MASK) c[b] = (jg < n && jg != ig[b]) ? c[b] : knn_inf<T>();
        some = some || c[b] < r[b][K - 1];
      }
      if (__any(some)) {  // uniform over the wave
#pragma unroll
        for (int b = 0; b < B; ++b)
          if (__any(c[b] < r[b][K - 1])) knn_insert<T, K>(c[b], jg, r[b], jx[b]);
      }
    }
  }
}

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding).  Writes, for every body below n of the column, the k records
// of row split * n + body of parts.
template <typename T, int K, int B>
__device__ __forceinline__ void knn_body(const typename V4<T>::type* __restrict__ posm, const int n, const int tiles_per_split, const int k,
                                         KnnRecord<T>* __restrict__ parts, const int col, const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[B], yi[B], zi[B], r[B][K];
  int ig[B], jx[B][K];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < n) p = posm[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ig[b] = li;
#pragma unroll
    for (int q = 0; q < K; ++q) {
      r[b][q] = knn_inf<T>();
      jx[b][q] = -1;
    }
  }
  const int g_lo = l0, g_hi = min(l0 + kBlock * B, n);  // the workgroup's bodies: a tile that meets them runs the masked loop
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  T4 next = zero;
  if (k0 < k1) next = posm[k0 * kTile + t];
  for (int kt = k0; kt < k1; ++kt) {
    __syncthreads();  // every lane is done with the previous tile
    tile[t] = next;
    __syncthreads();
    if (kt + 1 < k1) next = posm[(kt + 1) * kTile + t];
    const int j0 = kt * kTile;
    if (tile_masked(j0, g_lo, g_hi, n))
      knn_tile<T, K, B, true>(tile, j0, n, xi, yi, zi, ig, r, jx);
    else
      knn_tile<T, K, B, false>(tile, j0, n, xi, yi, zi, ig, r, jx);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) {
      KnnRecord<T>* row = parts + ((size_t)split * (size_t)n + (size_t)li) * (size_t)k;
#pragma unroll
      for (int q = 0; q < K; ++q)
        if (q < k) {
          KnnRecord<T> o;
          o.r2 = r[b][q]; o.j = jx[b][q];
          row[q] = o;
        }
    }
  }
}

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void knn_kernel(const typename V4<T>::type* __restrict__ posm, int n, int tiles_per_split, int k,
                                                     KnnRecord<T>* __restrict__ parts) {
  knn_body<T, K, kKnnBodies>(posm, n, tiles_per_split, k, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread]; parts[count][gridDim.y][n][k].
template <typename T>
struct EnsembleKnnArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  KnnRecord<T>* parts;               // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  int n, tiles_per_split, k;
};

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void ensemble_knn_kernel(const EnsembleKnnArgs<T> e) {
  const size_t m = blockIdx.z;
  knn_body<T, K, kKnnBodies>(e.posm + (e.first + m) * e.pos_stride, e.n, e.tiles_per_split, e.k,
                             e.parts + m * gridDim.y * (size_t)e.n * (size_t)e.k, blockIdx.x, blockIdx.y);
}

struct KnnMember : OutMember {};

template <typename T>
struct RaggedKnnArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const KnnMember* table;            // [members]
  KnnRecord<T>* parts;               // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  int k;
};

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void ragged_knn_kernel(const RaggedKnnArgs<T> a) {
  const KnnMember mem = a.table[a.first + blockIdx.z];
  const FieldShape s = field_shape(mem.n, mem.n);
  if ((int)blockIdx.x >= s.columns || (int)blockIdx.y >= s.splits) return;  // the whole workgroup: another, larger member's
  const size_t rel = (size_t)(mem.out_off - a.table[a.first].out_off);     // the bodies of the range before this member
  knn_body<T, K, kKnnBodies>(a.posm + mem.pos_off, mem.n, s.tiles_per_split, a.k, a.parts + rel * gridDim.y * (size_t)a.k, blockIdx.x,
                             blockIdx.y);
}

// Body idx of the call's `total` bodies, its member found by member_at..  The member has field_shape(n, n).splits rows of n * k
// records; its rows begin at (the bodies of the range before it) * row_splits * k, row_splits the gridDim.y of the pair-work
// launch..  The split rows are merged in ascending split order with knn_insert: a row is ascending, so it is left at its first
// entry that is not below the list's last; a later split's j are the higher ones and the compares are strict, so the merged
// list is in (r2, j) order.
template <typename T, int K>
__global__ __launch_bounds__(kBlock) void knn_finish_kernel(const KnnRecord<T>* __restrict__ parts, const KnnMember* __restrict__ table,
                                                            unsigned first, int count, int n_all, int row_splits, int k, unsigned total,
                                                            KnnRecord<T>* __restrict__ out) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const MemberAt at = member_at(table, first, count, n_all, idx);
  const int n = at.n;
  const size_t rel = at.rel;  // the bodies of the range before the body's member
  const int splits = field_shape(n, n).splits;
  const KnnRecord<T>* row = parts + (rel * (size_t)row_splits + ((size_t)idx - rel)) * (size_t)k;
  T r[K];
  int jx[K];
#pragma unroll
  for (int q = 0; q < K; ++q) {
    r[q] = knn_inf<T>();
    jx[q] = -1;
  }
  for (int s = 0; s < splits; ++s) {
    const KnnRecord<T>* v = row + (size_t)s * (size_t)n * (size_t)k;
    for (int q = 0; q < k; ++q) {
      const KnnRecord<T> e = v[q];
      if (!(e.r2 < r[K - 1])) break;
      knn_insert<T, K>(e.r2, e.j, r, jx);
    }
  }
  KnnRecord<T>* o = out + (size_t)idx * (size_t)k;
#pragma unroll
  for (int q = 0; q < K; ++q)
    if (q < k) {
      KnnRecord<T> e;
      e.r2 = r[q]; e.j = jx[q];
      o[q] = e;
    }
}

}  // namespace nbx
