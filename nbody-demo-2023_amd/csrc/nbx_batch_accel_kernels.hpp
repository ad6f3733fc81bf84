// nbx_batch_accel_kernels.hpp -- the kernels of nbx_ensemble_accel and nbx_ragged_accel (include/nbx_batch_accel.h): the
// accelerations of any range of members at the current positions, ONE launch for all of them, no integration.
//
//   ensemble_accel_kernel<NB, D, LOOP> / ensemble_accel_kernel_f64<NB, D>   grid (workgroups per member, count), block 256
//     Member m = first + blockIdx.y (wave-uniform).  As ensemble_step_kernel (nbx_ensemble_kernels.hpp) the kernel points the
//     ensemble's ForceArgs at member m, accp at the member's records of the acceleration slab besides, and runs jlane_step /
//     jlane_step_f64 (nbx_jlane.hpp) with acc_only = 1 and workgroup index blockIdx.x: the very code force_jlane_kernel runs for
//     nbx_accel on a context of n bodies with the same NB and loop, over the same grid.x -- the same bits.
//   ragged_accel_kernel<NB, D, LOOP> / ragged_accel_kernel_f64<NB, D>       grid = the workgroups of the members asked for, block 256
//     Workgroup blockIdx.x reads descriptor base + blockIdx.x of the member-order list of plan_ragged_accel (nbx_plan.hpp; a
//     RaggedWork, as the step reads: one scalar load at a wave-uniform index) and does the same for its member, with workgroup
//     index w.wg.
//
// acc_only is the literal 1, so the integrating branch of the body is not compiled into these kernels: they store
// {ax, ay, az, 0} to accp[li], li < n_k, and nothing else -- posm_next and ke_part stay NULL in their ForceArgs.  velm is read (the
// body requests the velocity of the body a lane would integrate before it looks at acc_only) and never written.
//
// The slab: accm[sum n_alloc_k], member k's records at its vel_off -- the size and layout of velm.  Records [n_k, n_alloc_k) are
// never written.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_jlane.hpp"

namespace nbx {

template <typename T>
struct EnsembleAccelArgs {
  ForceArgs<T> member0;  // the arguments of member 0: posm, velm, accp and the sizes; posm_next and ke_part are NULL
  unsigned pos_stride;   // records between members in posm: n_alloc + kSgprOverread
  unsigned vel_stride;   // records between members in velm and in the slab: own_pad
  unsigned first;        // blockIdx.y = 0 is this member
};

template <typename T>
__device__ __forceinline__ ForceArgs<T> ensemble_accel_member_args(const EnsembleAccelArgs<T>& e, const unsigned m) {
  ForceArgs<T> a = e.member0;
  a.posm += (size_t)m * e.pos_stride;
  a.velm += (size_t)m * e.vel_stride;
  a.accp += (size_t)m * e.vel_stride;
  return a;
}

template <int NB, int D, int LOOP>
__global__ __launch_bounds__(kBlock, 1) void ensemble_accel_kernel(const EnsembleAccelArgs<float> e) {
  jlane_step<NB, D, LOOP>(ensemble_accel_member_args(e, e.first + blockIdx.y), 1, blockIdx.x);
}

template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void ensemble_accel_kernel_f64(const EnsembleAccelArgs<double> e) {
  jlane_step_f64<NB, D>(ensemble_accel_member_args(e, e.first + blockIdx.y), 1, blockIdx.x);
}

template <typename T>
struct RaggedAccelArgs {
  const typename V4<T>::type* posm;  // the buffers of all members
  typename V4<T>::type* velm;        // read only
  typename V4<T>::type* accm;        // the slab
  const RaggedWork* work;            // the whole member-order list
  unsigned base;                     // blockIdx.x = 0 is this entry: work_begin[first]
};

template <typename T>
__device__ __forceinline__ ForceArgs<T> ragged_accel_member_args(const RaggedAccelArgs<T>& r, const RaggedWork& w) {
  ForceArgs<T> a{};  // posm_next, ke_part and posm_pairs are unused
  a.posm = r.posm + w.pos_off;
  a.velm = r.velm + w.vel_off;
  a.accp = r.accm + w.vel_off;
  a.i_begin = 0; a.i_count = w.n; a.own_pad = w.n_alloc; a.j_per_split = w.n_alloc; a.n_alloc = w.n_alloc;
  a.dt = (T)0;
  return a;
}

template <int NB, int D, int LOOP>
__global__ __launch_bounds__(kBlock, 1) void ragged_accel_kernel(const RaggedAccelArgs<float> r) {
  const RaggedWork w = r.work[r.base + blockIdx.x];
  jlane_step<NB, D, LOOP>(ragged_accel_member_args(r, w), 1, w.wg);
}

template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void ragged_accel_kernel_f64(const RaggedAccelArgs<double> r) {
  const RaggedWork w = r.work[r.base + blockIdx.x];
  jlane_step_f64<NB, D>(ragged_accel_member_args(r, w), 1, w.wg);
}

}  // namespace nbx
