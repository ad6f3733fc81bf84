// nbx_ensemble_diag_kernels.hpp -- the kernels of nbx_ensemble_diagnostics (include/nbx_ensemble_diag.h): the physics
// diagnostics of nbx_diag_kernels.hpp (device code: nbx_diag_body.hpp) for `count` members of an ensemble in ONE pair-work
// launch and one reduce launch.
//
//   ensemble_diag_kernel<T>       grid (columns, splits, count), block 256
//     Member m = first + blockIdx.z (wave-uniform).  The kernel points posm, velm and the partials at member m -- scalar
//     arithmetic on three pointers -- and runs diag_body, the body of diag_kernel, with i_begin = 0, i_count = n and workgroup
//     (blockIdx.x, blockIdx.y) of (gridDim.x, gridDim.y): the very code, over the very grid, that a context of n bodies owning
//     all of them runs.  Workgroups never straddle members and the j != i mask compares member-local indices, so a member's
//     partials are the bits a lone context produces.  A member's tiles [0, ceil(n / 256)) lie inside its n_alloc records, whose
//     tail [n, n_alloc) is zero (G*m = 0: adds exactly 0).
//   ensemble_diag_reduce_kernel   grid count, block 256
//     Workgroup k adds member first + k's `nparts` rows of kDiagFields doubles in diag_reduce_kernel's order (thread t: rows
//     t, t + 256, ...; then the block tree) into out[k * kDiagFields ...].
//
// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread], velm[S][own_pad],
// parts[S][nparts][kDiagFields] with row = split * columns + column.  No atomics: the same state gives the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_diag_body.hpp"

namespace nbx {

template <typename T>
struct EnsembleDiagArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* velm;  // member 0's velocities
  double* parts;                     // member 0's partials
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm: n_alloc + kSgprOverread
  unsigned vel_stride;               // records between members in velm: own_pad
  unsigned part_stride;              // doubles between members in parts: nparts * kDiagFields
  int n, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_diag_kernel(const EnsembleDiagArgs<T> e) {
  const size_t m = e.first + blockIdx.z;
  diag_body<T, kDiagBodies<T>>(e.posm + m * e.pos_stride, e.velm + m * e.vel_stride, 0, e.n, e.n, e.tiles_per_split,
                               e.parts + m * e.part_stride, blockIdx.x, blockIdx.y, gridDim.x);
}

__global__ __launch_bounds__(kBlock) void ensemble_diag_reduce_kernel(const double* __restrict__ parts, int nparts, unsigned first,
                                                                      double* __restrict__ out) {
  diag_reduce_rows(parts + ((size_t)first + blockIdx.x) * nparts * kDiagFields, nparts, out + (size_t)blockIdx.x * kDiagFields);
}

}  // namespace nbx
