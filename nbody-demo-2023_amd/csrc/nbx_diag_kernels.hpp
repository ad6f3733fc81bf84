// nbx_diag_kernels.hpp -- gfx950 kernels of the physics diagnostics (include/nbx_diag.h): the all-pairs potential energy
// and the O(n) sums (mass, kinetic energy, momentum, mass moment) of the owned bodies, in one pass, plus the fixed-order
// reduce of the per-workgroup partials.
//
//   diag_kernel         workgroup (x, y) owns bodies [i_begin + x*256*B, i_begin + (x+1)*256*B): lane t holds bodies
//                       t, t+256, ... (B of them); it sums j split y, a contiguous range of whole tiles (diag_splits: a
//                       fixed split that fills the GPU at sizes with few body blocks).  One pass over those j records in 256-record LDS tiles (broadcast
//                       ds_read_b128, the next tile prefetched into registers while the current one is summed).  Per pair:
//                       3 sub, 3 FMA (r^2 + eps^2), v_rsq, 1 FMA (sum += G*m_j * inv).  A tile's terms are summed in T,
//                       the tile sum is added to the body's fp64 accumulator.  Only the tiles that hold one of the
//                       workgroup's own bodies run the masked loop that drops j == i; all others pay nothing for it.
//                       Padding records (j >= n) carry G*m = 0 and add exactly 0.  Bodies are then weighted by m_i in
//                       fp64 and the nine per-body values are reduced over the workgroup in fixed order: one fp64
//                       partial of each per workgroup (the O(n) fields from split 0 only, the others write 0 there).
//                       No atomics anywhere: the result is the same bits on every call.
//   diag_reduce_kernel  one workgroup: partial k of field f at parts[k * kDiagFields + f], thread t sums k = t, t+256, ...,
//                       then the block tree -- the same fixed order as ke_reduce_kernel.
//
// Field order of the partials and of the reduced result (kDiagFields doubles):
//   0 mass  1 sum m v^2 (the kinetic energy's terms, computed in T exactly as euler_update computes them)
//   2 sum_i m_i phi_i with phi_i = sum_{j != i} G m_j / sqrt(r_ij^2 + eps^2)  (potential = -1/2 of it)
//   3..5 momentum  6..8 mass moment
//
// The device code itself is in nbx_diag_body.hpp (diag_body, diag_reduce_rows), which the ensemble form of these kernels
// (nbx_ensemble_diag_kernels.hpp) runs too; the kernels here are its callers for one context.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_diag_body.hpp"

namespace nbx {

template <typename T, int B>
__global__ __launch_bounds__(kBlock) void diag_kernel(const typename V4<T>::type* __restrict__ posm,
                                                      const typename V4<T>::type* __restrict__ velm, int i_begin, int i_count,
                                                      int n, int tiles_per_split, double* __restrict__ parts) {
  diag_body<T, B>(posm, velm, i_begin, i_count, n, tiles_per_split, parts, blockIdx.x, blockIdx.y, gridDim.x);
}

__global__ __launch_bounds__(kBlock) void diag_reduce_kernel(const double* __restrict__ parts, int nparts,
                                                             double* __restrict__ out) {
  diag_reduce_rows(parts, nparts, out);
}

}  // namespace nbx
