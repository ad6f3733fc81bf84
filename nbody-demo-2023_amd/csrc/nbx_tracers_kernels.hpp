// nbx_tracers_kernels.hpp -- the kernels of include/nbx_tracers.h: m massless test particles per system, resident on the device,
// that feel every body and are felt by none.  Instantiated by nbx_tracers.hip alone.
//
//   tracer_kernel<T>            grid (columns, splits), block 256            a context
//   ensemble_tracer_kernel<T>   grid (columns, splits, members), block 256   member blockIdx.z, its tracers at blockIdx.z * m
//   ragged_tracer_kernel<T>     grid (columns, largest splits of any member, members), block 256: the workgroup reads its member's
//                               {pos_off, n} from the table, evaluates field_shape(m, n) itself and returns at once where
//                               blockIdx.y is not one of its member's splits
//     All three run tracer_body: the pair loop of the field at caller-supplied points (nbx_field_kernels.hpp) without the
//     potential.  256 threads, kFieldPoints<T> = 2 tracers per lane, the j range of the workgroup's split in 256-record tiles
//     staged in LDS (the position records, read whole), the next tile prefetched into registers.  Columns, splits and tiles per
//     split are field_shape(m, n) (nbx_field_shape.hpp), a function of (m, n) alone.  The i side is the RESIDENT tracer position
//     buffer ({x, y, z, 0} records), not an uploaded copy.
//   tracer_update_kernel<T, KICK>   one thread per tracer of the call: adds the tracer's partial rows in fp64 in split order,
//                               rounds once to T -- the bits nbx_field returns for the same state and the same m points -- and
//                               applies euler_update (KICK: kick_update, nbx_pair.hpp) to the tracer's own two records in place.
//                               The velocity record's .w is 0: the energy term the update returns is discarded.
//
// One pair, in T: pair2 (fp32: 12 packed VALU and 2 v_rsq_f32 per two pairs, the lane's two tracers per packed instruction) and
// pair<double> (nbx_pair.hpp).  These are the operations, in the order and association, that the field's pair function applies to
// its three acceleration sums; its fourth sum and the fma (fp64: the second polynomial) that feeds it are not here.
//
// Every body counts: a tracer is not a body, so nothing is masked.  A record at or beyond n -- the zero padding -- has gm = 0 and
// a finite r2 >= eps2: its terms are exact zeros.  A tracer on body i gets d = 0, a zero term.
//
// Partials: parts[member][split][tracer] records {ax, ay, az, 0} of T, a member's rows together (stride gridDim.y * m records);
// a tracer's three accumulators are T, j ascending within the split.  No atomics.  The update is safe in place: the pair work of
// the step has finished in stream order, and each thread touches only its own records.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");

// The work of one workgroup: tracer column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), at the m tracers trp[0 .. m).  Writes, for every tracer below m
// of the column, record split * m + tracer of parts.
template <typename T, int B>
__device__ __forceinline__ void tracer_body(const typename V4<T>::type* __restrict__ posm, const int n,
                                            const typename V4<T>::type* __restrict__ trp, const int m, const int tiles_per_split,
                                            typename V4<T>::type* __restrict__ parts, const int col, const int split) {
  using T4 = typename V4<T>::type;
  static_assert(B % 2 == 0, "the fp32 loop takes the lane's tracers two at a time");
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first tracer of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[B], yi[B], zi[B], ax[B], ay[B], az[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < m) p = trp[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ax[b] = ay[b] = az[b] = (T)0;
  }
  TileWalk<T4> walk(posm, n, split, tiles_per_split);
  for (int k = walk.k0; k < walk.k1; ++k) {
    walk.stage(tile, k);
    if constexpr (sizeof(T) == 4) {
      f32x2 px[B / 2], py[B / 2], pz[B / 2], qx[B / 2], qy[B / 2], qz[B / 2];
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
        py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
        pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
        qx[h] = f32x2{ax[2 * h], ax[2 * h + 1]};
        qy[h] = f32x2{ay[2 * h], ay[2 * h + 1]};
        qz[h] = f32x2{az[2 * h], az[2 * h + 1]};
      }
#pragma unroll 4
      for (int j = 0; j < kTile; ++j) {
        const float4 r = tile[j];
#pragma unroll
        for (int h = 0; h < B / 2; ++h) pair2(r.x, r.y, r.z, r.w, px[h], py[h], pz[h], qx[h], qy[h], qz[h]);
      }
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        ax[2 * h] = qx[h].x; ax[2 * h + 1] = qx[h].y;
        ay[2 * h] = qy[h].x; ay[2 * h + 1] = qy[h].y;
        az[2 * h] = qz[h].x; az[2 * h + 1] = qz[h].y;
      }
    } else {
#pragma unroll 4
      for (int j = 0; j < kTile; ++j) {
        const T4 r = tile[j];
#pragma unroll
        for (int b = 0; b < B; ++b) pair<T>(r.x, r.y, r.z, r.w, xi[b], yi[b], zi[b], ax[b], ay[b], az[b]);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < m) {
      T4 o;
      o.x = ax[b]; o.y = ay[b]; o.z = az[b]; o.w = (T)0;
      parts[(size_t)split * (size_t)m + (size_t)li] = o;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void tracer_kernel(const typename V4<T>::type* __restrict__ posm, int n,
                                                        const typename V4<T>::type* __restrict__ trp, int m, int tiles_per_split,
                                                        typename V4<T>::type* __restrict__ parts) {
  tracer_body<T, kFieldPoints<T>>(posm, n, trp, m, tiles_per_split, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major: posm[S][n_alloc + kSgprOverread]; trp[S][m]; parts[S][gridDim.y][m].
template <typename T>
struct EnsembleTracerArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* trp;   // member 0's tracers
  typename V4<T>::type* parts;       // member 0's partial rows
  unsigned pos_stride;               // records between members in posm
  int n, m, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_tracer_kernel(const EnsembleTracerArgs<T> e) {
  const size_t k = blockIdx.z;
  tracer_body<T, kFieldPoints<T>>(e.posm + k * e.pos_stride, e.n, e.trp + k * (size_t)e.m, e.m, e.tiles_per_split,
                                  e.parts + k * gridDim.y * (size_t)e.m, blockIdx.x, blockIdx.y);
}

// built by the first tracer upload
struct TracerMember : PosMember {};

template <typename T>
struct RaggedTracerArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const TracerMember* table;         // [members]
  const typename V4<T>::type* trp;   // member 0's tracers
  typename V4<T>::type* parts;       // member 0's partial rows
  int m;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_tracer_kernel(const RaggedTracerArgs<T> r) {
  const size_t k = blockIdx.z;
  const MemberGroup<TracerMember> g = member_group(r.table, 0u, r.m);
  if ((int)blockIdx.y >= g.shape.splits) return;  // the whole workgroup: this split is another, larger member's
  tracer_body<T, kFieldPoints<T>>(r.posm + g.mem.pos_off, g.mem.n, r.trp + k * (size_t)r.m, r.m, g.shape.tiles_per_split,
                                  r.parts + k * gridDim.y * (size_t)r.m, blockIdx.x, blockIdx.y);
}

// Tracer idx of the object's `total` = members * m tracers: member idx / m, tracer idx % m.  The member has
// field_shape(m, n).splits rows, n from the table (a ragged ensemble) or n_all (table == nullptr); its rows begin at
// member * row_splits * m, row_splits the gridDim.y of the pair-work launch.  h: dt of a step, the kick's h.
template <typename T, bool KICK>
__global__ __launch_bounds__(kBlock) void tracer_update_kernel(const typename V4<T>::type* __restrict__ parts,
                                                               const TracerMember* __restrict__ table, int n_all, int m, int row_splits,
                                                               unsigned total, T h, typename V4<T>::type* __restrict__ trp,
                                                               typename V4<T>::type* __restrict__ trv) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const unsigned k = idx / (unsigned)m, p = idx - k * (unsigned)m;
  const int n = table ? table[k].n : n_all;
  const int splits = field_shape(m, n).splits;
  const T4* row = parts + (size_t)k * (size_t)row_splits * (size_t)m + p;
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (int s = 0; s < splits; ++s) {
    const T4 v = row[(size_t)s * (size_t)m];
    ax += (double)v.x;
    ay += (double)v.y;
    az += (double)v.z;
  }
  T4 w = trv[idx];
  if constexpr (KICK) {
    (void)kick_update<T>((T)ax, (T)ay, (T)az, h, w);
  } else {
    T4 q = trp[idx];
    (void)euler_update<T>((T)ax, (T)ay, (T)az, h, q, w);
    trp[idx] = q;
  }
  trv[idx] = w;
}

}  // namespace nbx
