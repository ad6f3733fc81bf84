// nbx_diag_body.hpp -- the device code of the physics diagnostics that more than one translation unit runs: the launch-shape
// rule (diag_splits, by way of nbx_diag_shape.hpp), the pair loop over one LDS tile (diag_tile), the work of one workgroup of diag_kernel (diag_body) and
// the fixed-order sum of a block of partial rows (diag_reduce_rows).  nbx_diag_kernels.hpp wraps them in the kernels of a
// context, nbx_ensemble_diag_kernels.hpp in the kernels of an ensemble, nbx_ragged_diag_kernels.hpp in those of a ragged
// ensemble; this header defines no kernel, so each of those translation units compiles exactly the kernels it names.  What the code does is described in nbx_diag_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_diag_shape.hpp"  // diag_splits and its constants, kDiagBodies: host-only, shared with nbx_plan.hpp
#include "nbx_pair.hpp"

namespace nbx {

constexpr int kDiagFields = 9;

// sum_{j in tile} G m_j / sqrt(|x_j - x_i|^2 + eps^2) for the lane's B bodies, in T.  MASK: the tile holds one of this
// workgroup's bodies -- the term j == i is replaced by an exact 0 (j_glob is the global index of tile record 0).
// The fp32 form runs two bodies per packed instruction (v_pk_add/fma_f32); the record is a scalar splat.
template <typename T, int B, bool MASK>
__device__ __forceinline__ void diag_tile(const typename V4<T>::type* tile, int j_glob, const T (&xi)[B], const T (&yi)[B],
                                          const T (&zi)[B], const int (&ig)[B], T (&s)[B]) {
  if constexpr (sizeof(T) == 4 && B % 2 == 0) {
    f32x2 px[B / 2], py[B / 2], pz[B / 2], ps[B / 2];
#pragma unroll
    for (int h = 0; h < B / 2; ++h) {
      px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
      py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
      pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
      ps[h] = f32x2{0.f, 0.f};
    }
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 8
    for (int j = 0; j < kTile; ++j) {
      const float4 r = tile[j];
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        const f32x2 dx = f32x2{r.x, r.x} - px[h], dy = f32x2{r.y, r.y} - py[h], dz = f32x2{r.z, r.z} - pz[h];
        f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        r2 = __builtin_elementwise_fma(dx, dx, r2);
        f32x2 inv;
        inv.x = __builtin_amdgcn_rsqf(r2.x);
        inv.y = __builtin_amdgcn_rsqf(r2.y);
        f32x2 gm = {r.w, r.w};
        if constexpr (MASK) {
          if (j_glob + j == ig[2 * h]) gm.x = 0.f;
          if (j_glob + j == ig[2 * h + 1]) gm.y = 0.f;
        }
        ps[h] = __builtin_elementwise_fma(gm, inv, ps[h]);
      }
    }
#pragma unroll
    for (int h = 0; h < B / 2; ++h) {
      s[2 * h] = ps[h].x;
      s[2 * h + 1] = ps[h].y;
    }
  } else {
#pragma unroll
    for (int b = 0; b < B; ++b) s[b] = (T)0;
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = tile[j];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const T dx = r.x - xi[b], dy = r.y - yi[b], dz = r.z - zi[b];
        const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
        const T inv = rsq(r2);
        T gm = r.w;
        if constexpr (MASK) {
          if (j_glob + j == ig[b]) gm = (T)0;
        }
        s[b] = fmaT(gm, inv, s[b]);
      }
    }
  }
}

// The work of one workgroup of diag_kernel: body column `col` of `cols`, j split `split`.  Shared with ensemble_diag_kernel
// (nbx_ensemble_diag_kernels.hpp), which runs it on one member's records with i_begin = 0, i_count = n.
template <typename T, int B>
__device__ __forceinline__ void diag_body(const typename V4<T>::type* __restrict__ posm,
                                          const typename V4<T>::type* __restrict__ velm, const int i_begin, const int i_count,
                                          const int n, const int tiles_per_split, double* __restrict__ parts, const int col,
                                          const int split, const int cols) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  __shared__ double red[kDiagFields][4];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first owned body (local index) of this workgroup
  T xi[B], yi[B], zi[B];
  int ig[B];
  double acc[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p;
    p.x = p.y = p.z = p.w = (T)0;
    if (li < i_count) p = posm[i_begin + li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ig[b] = i_begin + li;
    acc[b] = 0.0;
  }
  // the workgroup's bodies span global indices [g_lo, g_hi): a tile that meets that range runs the masked loop
  const int g_lo = i_begin + l0, g_hi = i_begin + min(l0 + kBlock * B, i_count);
  const int tiles = (n + kTile - 1) / kTile;  // records [n, tiles * kTile) are zero padding (< n_alloc)
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);  // this workgroup's j split
  T4 next;
  next.x = next.y = next.z = next.w = (T)0;
  if (k0 < k1) next = posm[k0 * kTile + t];
  for (int k = k0; k < k1; ++k) {
    __syncthreads();  // every lane is done with the previous tile
    tile[t] = next;
    __syncthreads();
    if (k + 1 < k1) next = posm[(k + 1) * kTile + t];
    const int j0 = k * kTile;
    T s[B];
    if (j0 < g_hi && j0 + kTile > g_lo)
      diag_tile<T, B, true>(tile, j0, xi, yi, zi, ig, s);
    else
      diag_tile<T, B, false>(tile, j0, xi, yi, zi, ig, s);
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b] += (double)s[b];
  }

  // rsq<double>() is 2/sqrt and the fp64 records carry G*m/8: undo both (x4, exact); fp32 needs nothing
  const double unscale = 1.0 / ((double)gm_prescale<T>() * (sizeof(T) == 8 ? 2.0 : 1.0));
  double f[kDiagFields];
#pragma unroll
  for (int q = 0; q < kDiagFields; ++q) f[q] = 0.0;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < i_count && split == 0) {
      const T4 v = velm[li];
      const double m = (double)v.w;
      const T v2 = add_rn(add_rn(mul_rn(v.x, v.x), mul_rn(v.y, v.y)), mul_rn(v.z, v.z));  // as euler_update
      f[0] += m;
      f[1] += (double)mul_rn(v.w, v2);
      f[2] += m * (acc[b] * unscale);
      f[3] += m * (double)v.x;
      f[4] += m * (double)v.y;
      f[5] += m * (double)v.z;
      f[6] += m * (double)xi[b];
      f[7] += m * (double)yi[b];
      f[8] += m * (double)zi[b];
    } else if (li < i_count) {  // j splits > 0: the potential only
      f[2] += (double)velm[li].w * (acc[b] * unscale);
    }
  }
  // workgroup sum, fixed order: wave64 shuffle tree, then the four wave sums
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int q = 0; q < kDiagFields; ++q) {
    double v = f[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[q][wave] = v;
  }
  __syncthreads();
  const size_t row = (size_t)split * cols + col;
  if (t < kDiagFields) parts[row * kDiagFields + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}

// rows[k * kDiagFields + q], k < nparts, summed per field q into out[q]: thread t adds rows t, t + 256, ..., then the block
// tree (wave64 shuffle tree, then the four wave sums) -- the same fixed order as ke_reduce_kernel.  One workgroup of kBlock.
__device__ __forceinline__ void diag_reduce_rows(const double* __restrict__ rows, const int nparts, double* __restrict__ out) {
  __shared__ double red[kDiagFields][4];
  double f[kDiagFields];
#pragma unroll
  for (int q = 0; q < kDiagFields; ++q) f[q] = 0.0;
  for (int k = threadIdx.x; k < nparts; k += kBlock)
#pragma unroll
    for (int q = 0; q < kDiagFields; ++q) f[q] += rows[(size_t)k * kDiagFields + q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kDiagFields; ++q) {
    double v = f[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[q][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < kDiagFields) {
    const int q = threadIdx.x;
    out[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
  }
}

}  // namespace nbx
