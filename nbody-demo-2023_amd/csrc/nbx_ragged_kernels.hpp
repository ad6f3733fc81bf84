// nbx_ragged_kernels.hpp -- the kernels of a ragged ensemble (include/nbx_ragged.h): independent systems of DIFFERENT size,
// advanced by ONE launch per time step.
//
//   ragged_step_kernel<NB, D, LOOP> / ragged_step_kernel_f64<NB, D>   grid W = sum of the members' workgroups, block 256
//     Workgroup blockIdx.x reads its RaggedWork descriptor (nbx_plan.hpp: 32 bytes at a wave-uniform index, i.e. one scalar
//     load): where its member lives, how long it is, and which workgroup `wg` of that member this one is.  It builds the
//     member's ForceArgs from it and runs jlane_step / jlane_step_f64 (nbx_jlane.hpp) with workgroup index wg: the very code
//     a context of n_k bodies with the same NB and loop runs, over the same workgroups.  Workgroups never straddle members,
//     so positions, velocities and energy partials of a member are the bits a lone context produces.  The descriptor is
//     self-contained: one dependent fetch at the head of a launch that lasts a few microseconds, where a (workgroup -> member)
//     entry followed by a (member -> offsets) entry would cost two.
//   ragged_ke_reduce_kernel   grid members, block 256
//     Workgroup m adds member m's energy partials in ke_reduce_kernel's order (thread t: partials t, t + 256, ...; then the
//     block tree) into out[m]; where they lie and how many they are comes from a table of one {offset, count} per member.
//
// Layout in HBM, members one behind the other (member k at the offsets of its descriptors):
//   posm[2][sum (n_alloc_k + kSgprOverread)]  {x, y, z, G*m}; n_alloc_k = n_k rounded up to 256; records [n_k, n_alloc_k) are zero
//                                             (zero mass: no force), and so are the kSgprOverread spare records behind them --
//                                             the guarantee an ensemble gives the prefetch of the jlane body
//   velm[sum n_alloc_k]                       {vx, vy, vz, m}
//   ke_part[W]                                one fp64 partial of sum m v^2 per workgroup, a member's grid_k partials together
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_jlane.hpp"

namespace nbx {

template <typename T>
struct RaggedArgs {
  const typename V4<T>::type* posm;  // the buffers of all members
  typename V4<T>::type* posm_next;
  typename V4<T>::type* velm;
  double* ke_part;
  const RaggedWork* work;            // [gridDim.x]
  T dt;
};

template <typename T>
__device__ __forceinline__ ForceArgs<T> ragged_member_args(const RaggedArgs<T>& r, const RaggedWork& w) {
  ForceArgs<T> a{};  // accp and posm_pairs are unused (a ragged ensemble only steps)
  a.posm = r.posm + w.pos_off;
  a.posm_next = r.posm_next + w.pos_off;
  a.velm = r.velm + w.vel_off;
  a.ke_part = r.ke_part + w.ke_off;
  a.i_begin = 0; a.i_count = w.n; a.own_pad = w.n_alloc; a.j_per_split = w.n_alloc; a.n_alloc = w.n_alloc;
  a.dt = r.dt;
  return a;
}

template <int NB, int D, int LOOP>
__global__ __launch_bounds__(kBlock, 1) void ragged_step_kernel(const RaggedArgs<float> r) {
  const RaggedWork w = r.work[blockIdx.x];
  jlane_step<NB, D, LOOP>(ragged_member_args(r, w), 0, w.wg);
}

template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void ragged_step_kernel_f64(const RaggedArgs<double> r) {
  const RaggedWork w = r.work[blockIdx.x];
  jlane_step_f64<NB, D>(ragged_member_args(r, w), 0, w.wg);
}

struct RaggedParts { unsigned ke_off; int count; };  // member m's partials: ke_part[ke_off, ke_off + count)

__global__ __launch_bounds__(kBlock) void ragged_ke_reduce_kernel(const double* __restrict__ ke_part, const RaggedParts* __restrict__ parts,
                                                                  double* __restrict__ out) {
  __shared__ double ksum[4];
  const RaggedParts p = parts[blockIdx.x];
  const double* part = ke_part + p.ke_off;
  double v = 0.0;
  for (int k = threadIdx.x; k < p.count; k += kBlock) v += part[k];
  const double s = block_sum(v, ksum);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace nbx
