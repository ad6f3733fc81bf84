// nbx_kick_kernels.hpp -- the kernels of include/nbx_kick.h: v += a(x) * h for every owned body at the current positions, the
// positions untouched.
//
//   ensemble_kick_kernel<NB, D, LOOP> / ensemble_kick_kernel_f64<NB, D>   grid (workgroups per member, S), block 256
//   ragged_kick_kernel<NB, D, LOOP> / ragged_kick_kernel_f64<NB, D>       grid W = the step's own work list, block 256
//     The step kernels of nbx_ensemble_kernels.hpp / nbx_ragged_kernels.hpp over again -- same grid, same member arithmetic, same
//     descriptor -- around jlane_step / jlane_step_f64 (nbx_jlane.hpp) with the epilogue JLANE_EPI_KICK, a compile-time choice:
//     the j loop and the LDS transpose are the step's and the accel kernels', so the acceleration is the bits *_accel returns;
//     lane t < NB then updates the velocity alone (kick_update, nbx_pair.hpp), stores velm[li] and adds m v^2 of the kicked
//     velocity to the workgroup's ke_part.  Neither the integrating nor the storing epilogue is in the code: these kernels write
//     one velocity record per body and one double per workgroup, and nothing else -- posm_next and accp stay NULL in their
//     ForceArgs.  ForceArgs::dt carries h.
//   kick_kernel<T>   grid ceil(i_count / 256), block 256 -- a context's second launch
//     One body per thread, as integrate_kernel (nbx_kernels.hpp): adds the S partial accelerations the acc-only force launch left
//     in the slabs in split order (the order integrate_kernel and nbx_accel add them in), applies kick_update and writes one
//     ke_part per workgroup.  Reads no position.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_jlane.hpp"

namespace nbx {

template <typename T>
struct EnsembleKickArgs {
  ForceArgs<T> member0;  // the arguments of member 0: posm, velm, ke_part, the sizes and dt = h; posm_next and accp are NULL
  unsigned pos_stride;   // records between members in posm: n_alloc + kSgprOverread
  unsigned vel_stride;   // records between members in velm: own_pad
  unsigned ke_stride;    // partials between members in ke_part: gridDim.x
};

template <typename T>
__device__ __forceinline__ ForceArgs<T> ensemble_kick_member_args(const EnsembleKickArgs<T>& e, const unsigned m) {
  ForceArgs<T> a = e.member0;
  a.posm += (size_t)m * e.pos_stride;
  a.velm += (size_t)m * e.vel_stride;
  a.ke_part += (size_t)m * e.ke_stride;
  return a;
}

template <int NB, int D, int LOOP>
__global__ __launch_bounds__(kBlock, 1) void ensemble_kick_kernel(const EnsembleKickArgs<float> e) {
  jlane_step<NB, D, LOOP, JLANE_EPI_KICK>(ensemble_kick_member_args(e, blockIdx.y), 0, blockIdx.x);
}

template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void ensemble_kick_kernel_f64(const EnsembleKickArgs<double> e) {
  jlane_step_f64<NB, D, JLANE_EPI_KICK>(ensemble_kick_member_args(e, blockIdx.y), 0, blockIdx.x);
}

template <typename T>
struct RaggedKickArgs {
  const typename V4<T>::type* posm;  // the buffers of all members
  typename V4<T>::type* velm;
  double* ke_part;
  const RaggedWork* work;            // [gridDim.x]: the step's list
  T h;
};

template <typename T>
__device__ __forceinline__ ForceArgs<T> ragged_kick_member_args(const RaggedKickArgs<T>& r, const RaggedWork& w) {
  ForceArgs<T> a{};  // posm_next, accp and posm_pairs are unused
  a.posm = r.posm + w.pos_off;
  a.velm = r.velm + w.vel_off;
  a.ke_part = r.ke_part + w.ke_off;
  a.i_begin = 0; a.i_count = w.n; a.own_pad = w.n_alloc; a.j_per_split = w.n_alloc; a.n_alloc = w.n_alloc;
  a.dt = r.h;
  return a;
}

template <int NB, int D, int LOOP>
__global__ __launch_bounds__(kBlock, 1) void ragged_kick_kernel(const RaggedKickArgs<float> r) {
  const RaggedWork w = r.work[blockIdx.x];
  jlane_step<NB, D, LOOP, JLANE_EPI_KICK>(ragged_kick_member_args(r, w), 0, w.wg);
}

template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void ragged_kick_kernel_f64(const RaggedKickArgs<double> r) {
  const RaggedWork w = r.work[blockIdx.x];
  jlane_step_f64<NB, D, JLANE_EPI_KICK>(ragged_kick_member_args(r, w), 0, w.wg);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void kick_kernel(typename V4<T>::type* __restrict__ velm, const typename V4<T>::type* __restrict__ accp,
                                                      int nsplit, int own_pad, int i_count, T h, double* __restrict__ ke_part) {
  using T4 = typename V4<T>::type;
  __shared__ double ksum[4];
  const int li = blockIdx.x * kBlock + threadIdx.x;
  double ke = 0.0;
  if (li < i_count) {
    T ax = (T)0, ay = (T)0, az = (T)0;
    for (int s = 0; s < nsplit; ++s) {
      const T4 q = accp[(size_t)s * own_pad + li];
      ax += q.x; ay += q.y; az += q.z;
    }
    T4 v = velm[li];
    ke = (double)kick_update<T>(ax, ay, az, h, v);
    velm[li] = v;
  }
  const double s = block_sum(ke, ksum);
  if (threadIdx.x == 0) ke_part[blockIdx.x] = s;
}

}  // namespace nbx
