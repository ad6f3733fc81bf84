// nbx_ensemble_kernels.hpp -- the kernels of an ensemble (include/nbx_ensemble.h): S independent systems of n bodies each,
// advanced by ONE launch per time step.
//
//   ensemble_step_kernel<NB, D, LOOP> / ensemble_step_kernel_f64<NB, D>   grid (workgroups per member, S), block 256
//     Member m = blockIdx.y (wave-uniform).  The kernel points the ensemble's ForceArgs at member m -- scalar arithmetic on
//     four pointers -- and runs jlane_step / jlane_step_f64 (nbx_jlane.hpp), the body of force_jlane_kernel, with workgroup
//     index blockIdx.x: the very code a context of n bodies with the same NB and loop runs, over the same grid.x.  Workgroups
//     never straddle members, so positions, velocities and energy partials of a member are the bits a lone context produces.
//   ensemble_ke_reduce_kernel   grid S, block 256
//     Workgroup m adds member m's energy partials in ke_reduce_kernel's order (thread t: partials t, t + 256, ...; then the
//     block tree) into out[m].
//
// Layout in HBM, member-major:
//   posm[2][S][n_alloc + kSgprOverread]  {x, y, z, G*m}; records [n, n_alloc) of a member are zero (zero mass: no force), and so
//                                        are the kSgprOverread spare records behind them -- the prefetch of the jlane body asks
//                                        for up to D blocks of 64 records past a member's end and never applies them; with the
//                                        spare records they are mapped memory and never a neighbour's live data
//   velm[S][own_pad]                     {vx, vy, vz, m}, own_pad = n rounded up to 256
//   ke_part[S][grid.x]                   one fp64 partial of sum m v^2 per workgroup
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_jlane.hpp"

namespace nbx {

template <typename T>
struct EnsembleArgs {
  ForceArgs<T> member0;           // the arguments of member 0; accp and posm_pairs are unused (an ensemble only steps)
  unsigned pos_stride;            // records between members in posm and posm_next: n_alloc + kSgprOverread
  unsigned vel_stride;            // records between members in velm: own_pad
  unsigned ke_stride;             // partials between members in ke_part: gridDim.x
};

template <typename T>
__device__ __forceinline__ ForceArgs<T> ensemble_member_args(const EnsembleArgs<T>& e, const unsigned m) {
  ForceArgs<T> a = e.member0;
  a.posm += (size_t)m * e.pos_stride;
  a.posm_next += (size_t)m * e.pos_stride;
  a.velm += (size_t)m * e.vel_stride;
  a.ke_part += (size_t)m * e.ke_stride;
  return a;
}

template <int NB, int D, int LOOP>
__global__ __launch_bounds__(kBlock, 1) void ensemble_step_kernel(const EnsembleArgs<float> e) {
  jlane_step<NB, D, LOOP>(ensemble_member_args(e, blockIdx.y), 0, blockIdx.x);
}

template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void ensemble_step_kernel_f64(const EnsembleArgs<double> e) {
  jlane_step_f64<NB, D>(ensemble_member_args(e, blockIdx.y), 0, blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void ensemble_ke_reduce_kernel(const double* __restrict__ ke_part, int nparts, double* __restrict__ out) {
  __shared__ double ksum[4];
  const double* part = ke_part + (size_t)blockIdx.x * nparts;
  double v = 0.0;
  for (int k = threadIdx.x; k < nparts; k += kBlock) v += part[k];
  const double s = block_sum(v, ksum);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace nbx
