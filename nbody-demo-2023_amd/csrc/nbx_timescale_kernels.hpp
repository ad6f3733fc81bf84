// nbx_timescale_kernels.hpp -- the kernels of nbx_timescale, nbx_ensemble_timescale and nbx_ragged_timescale
// (include/nbx_timescale.h): over all pairs i < n, j < n, j != i of a system the largest approach rate |v_j - v_i|^2 / r2, the
// largest free-fall rate G (m_i + m_j) / r2^(3/2) and the smallest r2 = |x_j - x_i|^2 + eps^2.  Instantiated by
// nbx_timescale.hip alone.
//
//   timescale_kernel<T>            grid (columns, splits), block 256            a context that owns all n bodies
//   ensemble_timescale_kernel<T>   grid (columns, splits, count), block 256     member first + blockIdx.z
//   ragged_timescale_kernel<T>     grid = the workgroups of the members asked for (1-D): workgroup blockIdx.x reads the
//                                  RaggedDiagWork descriptor work[base + blockIdx.x] (plan_ragged_diag, nbx_plan.hpp)
//     All three run ts_body, the shape of diag_body (nbx_diag_body.hpp): 256 threads, kDiagBodies<T> bodies per lane, the j
//     range of the workgroup's split in 256-record tiles staged in LDS -- here TWO arrays per tile, the position records and the
//     velocity records of the same j (a velocity is loaded only where j < n: what lies behind a member's last velocity is never
//     read).  The columns, j splits and tiles per split are diag_splits' (nbx_diag_shape.hpp), for a context and for every member.
//   timescale_reduce_kernel        grid count, block 256   workgroup k: max, max, min over system first + k's `nparts` rows
//   ragged_timescale_reduce_kernel grid count, block 256   the same over the rows the member's {row_off, rows} entry names
//
// One pair, in T (ts_pair; the fp32 tile loop is the same operations on two bodies per packed instruction):
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))           the force kernels' r2
//   ux,uy,uz = v_j - v_i;  w  = fma(ux,ux, fma(uy,uy, uz*uz))
//   inv = rsq(r2);  inv2 = inv*inv;  approach = w*inv2;  freefall = ((gm_i + gm_j)*inv)*inv2
// gm is the position record's .w = G*m * gm_prescale<T>(), the body's own as well as its partner's, so the velocity record's
// mass is not read.  rsq<double>() is 2/sqrt and gm_prescale<double>() is 1/8: the fp64 approach rate comes out x4 and the
// free-fall rate x(8/8) = x1; ts_body undoes that with exact powers of two after its reduction (max commutes with a positive
// scale).  Every multiply that is not part of a specified fused operation goes through mul_rn / add_rn, so no build contracts
// one.
//
// The mask: a pair is dropped EXACTLY -- rates 0, r2 +infinity, the neutral elements -- where j == i or j >= n.  A padding
// record has G*m = 0 but a position (the origin) and a velocity (zero): it would give a small, wrong approach rate and, for a
// system far from the origin, nothing else would remove it.  Only tiles that meet the workgroup's own bodies or reach past n run
// the masked loop; every other tile runs the loop without the compares (ts_tile<..., MASK>, as diag_tile).
//
// Nothing is summed: a maximum or minimum does not depend on the order it is taken in, so the three values are the same bits
// for every launch shape, and a member's are a lone context's.  parts[row][3] with row = split * columns + column within a
// system; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_diag_shape.hpp"  // kDiagBodies, diag_splits (host side)
#include "nbx_pair.hpp"
#include "nbx_plan.hpp"  // RaggedDiagWork, RaggedDiagRows

namespace nbx {

constexpr int kTsFields = 3;  // approach_rate2, freefall_rate2 (maxima), min_r2 (a minimum)

__device__ __forceinline__ float ts_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double ts_max(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float ts_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double ts_min(double a, double b) { return __builtin_fmin(a, b); }
template <typename T> __device__ __forceinline__ T ts_inf() { return (T)__builtin_huge_valf(); }

// The pair arithmetic of include/nbx_timescale.h for one pair, in T.  gmi, gmj: the records' .w.  approach and freefall carry
// the scales of rsq<T>() and gm_prescale<T>() (see above).
template <typename T>
__device__ __forceinline__ void ts_pair(T xj, T yj, T zj, T gmj, T uj, T vj, T wj, T xi, T yi, T zi, T gmi, T ui, T vi, T wi,
                                        T& approach, T& freefall, T& r2) {
  const T dx = xj - xi, dy = yj - yi, dz = zj - zi;
  r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
  const T ux = uj - ui, uy = vj - vi, uz = wj - wi;
  const T w = fmaT(ux, ux, fmaT(uy, uy, mul_rn(uz, uz)));
  const T inv = rsq(r2);
  const T inv2 = mul_rn(inv, inv);
  approach = mul_rn(w, inv2);
  freefall = mul_rn(mul_rn(add_rn(gmi, gmj), inv), inv2);
}

// One LDS tile against the lane's B bodies: running maxima / minimum per body.  MASK: the tile holds one of this workgroup's
// bodies or records at or beyond n -- such a pair leaves the three values as they were (j_glob: global index of tile record 0).
template <typename T, int B, bool MASK>
__device__ __forceinline__ void ts_tile(const typename V4<T>::type* ptile, const typename V4<T>::type* vtile, int j_glob, int n,
                                        const T (&xi)[B], const T (&yi)[B], const T (&zi)[B], const T (&gi)[B], const T (&ui)[B],
                                        const T (&vi)[B], const T (&wi)[B], const int (&ig)[B], T (&ap)[B], T (&ff)[B], T (&mr)[B]) {
  if constexpr (sizeof(T) == 4 && B % 2 == 0) {
    f32x2 px[B / 2], py[B / 2], pz[B / 2], pg[B / 2], pu[B / 2], pv[B / 2], pw[B / 2];
#pragma unroll
    for (int h = 0; h < B / 2; ++h) {
      px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
      py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
      pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
      pg[h] = f32x2{gi[2 * h], gi[2 * h + 1]};
      pu[h] = f32x2{ui[2 * h], ui[2 * h + 1]};
      pv[h] = f32x2{vi[2 * h], vi[2 * h + 1]};
      pw[h] = f32x2{wi[2 * h], wi[2 * h + 1]};
    }
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = ptile[j];
      const float4 s = vtile[j];
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        const f32x2 dx = f32x2{r.x, r.x} - px[h], dy = f32x2{r.y, r.y} - py[h], dz = f32x2{r.z, r.z} - pz[h];
        f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        r2 = __builtin_elementwise_fma(dx, dx, r2);
        const f32x2 ux = f32x2{s.x, s.x} - pu[h], uy = f32x2{s.y, s.y} - pv[h], uz = f32x2{s.z, s.z} - pw[h];
        f32x2 w = mul_rn(uz, uz);
        w = __builtin_elementwise_fma(uy, uy, w);
        w = __builtin_elementwise_fma(ux, ux, w);
        f32x2 inv;
        inv.x = __builtin_amdgcn_rsqf(r2.x);
        inv.y = __builtin_amdgcn_rsqf(r2.y);
        const f32x2 inv2 = mul_rn(inv, inv);
        f32x2 a = mul_rn(w, inv2);
        f32x2 f = mul_rn(mul_rn(add_rn(pg[h], f32x2{r.w, r.w}), inv), inv2);
        if constexpr (MASK) {
          const int jg = j_glob + j;
          if (jg >= n || jg == ig[2 * h]) { a.x = 0.f; f.x = 0.f; r2.x = ts_inf<float>(); }
          if (jg >= n || jg == ig[2 * h + 1]) { a.y = 0.f; f.y = 0.f; r2.y = ts_inf<float>(); }
        }
        ap[2 * h] = ts_max(ap[2 * h], a.x);
        ap[2 * h + 1] = ts_max(ap[2 * h + 1], a.y);
        ff[2 * h] = ts_max(ff[2 * h], f.x);
        ff[2 * h + 1] = ts_max(ff[2 * h + 1], f.y);
        mr[2 * h] = ts_min(mr[2 * h], r2.x);
        mr[2 * h + 1] = ts_min(mr[2 * h + 1], r2.y);
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = ptile[j];
      const typename V4<T>::type s = vtile[j];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        T a, f, r2;
        ts_pair<T>(r.x, r.y, r.z, r.w, s.x, s.y, s.z, xi[b], yi[b], zi[b], gi[b], ui[b], vi[b], wi[b], a, f, r2);
        if constexpr (MASK) {
          const int jg = j_glob + j;
          if (jg >= n || jg == ig[b]) { a = (T)0; f = (T)0; r2 = ts_inf<T>(); }
        }
        ap[b] = ts_max(ap[b], a);
        ff[b] = ts_max(ff[b], f);
        mr[b] = ts_min(mr[b], r2);
      }
    }
  }
}

// The work of one workgroup: body column `col` of `cols`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding) and whose velocity records velm[0 .. n) are read.  Writes row
// split * cols + col of parts: {max approach, max freefall, min r2} over the workgroup's pairs, widened and unscaled.
template <typename T, int B>
__device__ __forceinline__ void ts_body(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                        const int n, const int tiles_per_split, double* __restrict__ parts, const int col,
                                        const int split, const int cols) {
  using T4 = typename V4<T>::type;
  __shared__ T4 ptile[kTile];
  __shared__ T4 vtile[kTile];
  __shared__ double red[kTsFields][4];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  T4 zero;
  zero.x = zero.y = zero.z = zero.w = (T)0;
  T xi[B], yi[B], zi[B], gi[B], ui[B], vi[B], wi[B];
  int ig[B];
  T ap[B], ff[B], mr[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero, v = zero;
    if (li < n) {
      p = posm[li];
      v = velm[li];
    }
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z; gi[b] = p.w;
    ui[b] = v.x; vi[b] = v.y; wi[b] = v.z;
    ig[b] = li;
    ap[b] = (T)0;
    ff[b] = (T)0;
    mr[b] = ts_inf<T>();
  }
  const int g_lo = l0, g_hi = min(l0 + kBlock * B, n);  // the workgroup's bodies: a tile that meets them runs the masked loop
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  T4 next_p = zero, next_v = zero;
  if (k0 < k1) {
    const int j = k0 * kTile + t;
    next_p = posm[j];
    if (j < n) next_v = velm[j];
  }
  for (int k = k0; k < k1; ++k) {
    __syncthreads();  // every lane is done with the previous tile
    ptile[t] = next_p;
    vtile[t] = next_v;
    __syncthreads();
    if (k + 1 < k1) {
      const int j = (k + 1) * kTile + t;
      next_p = posm[j];
      next_v = zero;
      if (j < n) next_v = velm[j];
    }
    const int j0 = k * kTile;
    if ((j0 < g_hi && j0 + kTile > g_lo) || j0 + kTile > n)
      ts_tile<T, B, true>(ptile, vtile, j0, n, xi, yi, zi, gi, ui, vi, wi, ig, ap, ff, mr);
    else
      ts_tile<T, B, false>(ptile, vtile, j0, n, xi, yi, zi, gi, ui, vi, wi, ig, ap, ff, mr);
  }

  // the lane's bodies (those below n), widened exactly; then the workgroup: wave64 shuffle tree, the four wave values through LDS
  double f[kTsFields] = {0.0, 0.0, (double)ts_inf<float>()};
#pragma unroll
  for (int b = 0; b < B; ++b) {
    if (l0 + b * kBlock + t < n) {
      f[0] = ts_max(f[0], (double)ap[b]);
      f[1] = ts_max(f[1], (double)ff[b]);
      f[2] = ts_min(f[2], (double)mr[b]);
    }
  }
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int q = 0; q < kTsFields; ++q) {
    double v = f[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(v, off, 64);
      v = q == 2 ? ts_min(v, o) : ts_max(v, o);
    }
    if (lane == 0) red[q][wave] = v;
  }
  __syncthreads();
  if (t < kTsFields) {
    // rsq<double>() is 2/sqrt (inv2 is x4) and the fp64 records carry G*m/8: approach x4, freefall x(8/8); fp32 needs nothing
    constexpr double rs = sizeof(T) == 8 ? 2.0 : 1.0;
    const double unscale = t == 0 ? 1.0 / (rs * rs) : t == 1 ? 1.0 / ((double)gm_prescale<T>() * rs * rs * rs) : 1.0;
    const double v = t == 2 ? ts_min(ts_min(red[2][0], red[2][1]), ts_min(red[2][2], red[2][3]))
                            : ts_max(ts_max(red[t][0], red[t][1]), ts_max(red[t][2], red[t][3]));
    parts[((size_t)split * cols + col) * kTsFields + t] = v * unscale;
  }
}

// rows[k * 3 + q], k < nparts -> out[q]: max, max, min.  One workgroup of kBlock.
__device__ __forceinline__ void ts_reduce_rows(const double* __restrict__ rows, const int nparts, double* __restrict__ out) {
  __shared__ double red[kTsFields][4];
  double f[kTsFields] = {0.0, 0.0, (double)ts_inf<float>()};
  for (int k = threadIdx.x; k < nparts; k += kBlock) {
    f[0] = ts_max(f[0], rows[(size_t)k * kTsFields + 0]);
    f[1] = ts_max(f[1], rows[(size_t)k * kTsFields + 1]);
    f[2] = ts_min(f[2], rows[(size_t)k * kTsFields + 2]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kTsFields; ++q) {
    double v = f[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(v, off, 64);
      v = q == 2 ? ts_min(v, o) : ts_max(v, o);
    }
    if (lane == 0) red[q][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < kTsFields) {
    const int q = threadIdx.x;
    out[q] = q == 2 ? ts_min(ts_min(red[2][0], red[2][1]), ts_min(red[2][2], red[2][3]))
                    : ts_max(ts_max(red[q][0], red[q][1]), ts_max(red[q][2], red[q][3]));
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void timescale_kernel(const typename V4<T>::type* __restrict__ posm,
                                                           const typename V4<T>::type* __restrict__ velm, int n, int tiles_per_split,
                                                           double* __restrict__ parts) {
  ts_body<T, kDiagBodies<T>>(posm, velm, n, tiles_per_split, parts, blockIdx.x, blockIdx.y, gridDim.x);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread], velm[S][own_pad], parts[S][nparts][3].
template <typename T>
struct EnsembleTsArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* velm;  // member 0's velocities
  double* parts;                     // member 0's partial rows
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  unsigned vel_stride;               // records between members in velm
  unsigned part_stride;              // doubles between members in parts: nparts * 3
  int n, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_timescale_kernel(const EnsembleTsArgs<T> e) {
  const size_t m = e.first + blockIdx.z;
  ts_body<T, kDiagBodies<T>>(e.posm + m * e.pos_stride, e.velm + m * e.vel_stride, e.n, e.tiles_per_split, e.parts + m * e.part_stride,
                             blockIdx.x, blockIdx.y, gridDim.x);
}

template <typename T>
struct RaggedTsArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  double* parts;                     // the partial rows of all members, a member's together at its row_off
  const RaggedDiagWork* work;        // plan_ragged_diag's list, member order
  unsigned base;                     // descriptor of blockIdx.x == 0: work_begin[first]
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_timescale_kernel(const RaggedTsArgs<T> r) {
  const RaggedDiagWork w = r.work[(size_t)r.base + blockIdx.x];
  ts_body<T, kDiagBodies<T>>(r.posm + w.pos_off, r.velm + w.vel_off, w.n, w.tiles_per_split, r.parts + (size_t)w.row_off * kTsFields,
                             w.col, w.split, w.cols);
}

// system first + blockIdx.x of systems that have `nparts` rows each (a context: one system, first = 0)
__global__ __launch_bounds__(kBlock) void timescale_reduce_kernel(const double* __restrict__ parts, int nparts, unsigned first,
                                                                  double* __restrict__ out) {
  ts_reduce_rows(parts + ((size_t)first + blockIdx.x) * nparts * kTsFields, nparts, out + (size_t)blockIdx.x * kTsFields);
}

__global__ __launch_bounds__(kBlock) void ragged_timescale_reduce_kernel(const double* __restrict__ parts,
                                                                         const RaggedDiagRows* __restrict__ rows, unsigned first,
                                                                         double* __restrict__ out) {
  const RaggedDiagRows m = rows[(size_t)first + blockIdx.x];
  ts_reduce_rows(parts + (size_t)m.row_off * kTsFields, m.rows, out + (size_t)blockIdx.x * kTsFields);
}

}  // namespace nbx
