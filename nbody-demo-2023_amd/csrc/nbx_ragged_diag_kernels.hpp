// nbx_ragged_diag_kernels.hpp -- the kernels of nbx_ragged_diagnostics (include/nbx_ragged_diag.h): the physics diagnostics of
// nbx_diag_kernels.hpp (device code: nbx_diag_body.hpp) for `count` members of a ragged ensemble -- members of DIFFERENT size --
// in ONE pair-work launch and one reduce launch.
//
//   ragged_diag_kernel<T>       grid = the workgroups of the members asked for (1-D), block 256
//     Workgroup blockIdx.x reads its RaggedDiagWork descriptor work[base + blockIdx.x] (nbx_plan.hpp: 32 bytes at a wave-uniform
//     index, i.e. one scalar load; base = the first workgroup of member `first` in the list, which is in member order): where
//     its member lives, how long it is, and which (column, split) of the member's `cols` columns this workgroup is.  It points
//     posm, velm and the partials at the member and runs diag_body, the body of diag_kernel, with i_begin = 0, i_count = n:
//     the very code, over the very (column, split) pairs, that a context of n bodies owning all of them runs.  Workgroups never
//     straddle members and the j != i mask compares member-local indices, so a member's partials are the bits a lone context
//     produces.  A member's tiles [0, ceil(n / 256)) lie inside its n_alloc records, whose tail [n, n_alloc) is zero (G*m = 0:
//     adds exactly 0) -- the layout of nbx_ragged_kernels.hpp.
//   ragged_diag_reduce_kernel   grid count, block 256
//     Workgroup k reads member first + k's {row_off, rows} and adds those rows of kDiagFields doubles in diag_reduce_kernel's
//     order (thread t: rows t, t + 256, ...; then the block tree) into out[k * kDiagFields ...].
//
// parts[total rows][kDiagFields], a member's rows together at row_off, row = split * cols + column within the member: a member's
// rows are where they are whatever range is asked for.  No atomics: the same state gives the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_diag_body.hpp"
#include "nbx_plan.hpp"  // RaggedDiagWork, RaggedDiagRows

namespace nbx {

template <typename T>
struct RaggedDiagArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  double* parts;                     // the partial rows of all members
  const RaggedDiagWork* work;        // the whole list, member order
  unsigned base;                     // descriptor of blockIdx.x == 0: work_begin[first]
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_diag_kernel(const RaggedDiagArgs<T> r) {
  const RaggedDiagWork w = r.work[(size_t)r.base + blockIdx.x];
  diag_body<T, kDiagBodies<T>>(r.posm + w.pos_off, r.velm + w.vel_off, 0, w.n, w.n, w.tiles_per_split,
                               r.parts + (size_t)w.row_off * kDiagFields, w.col, w.split, w.cols);
}

__global__ __launch_bounds__(kBlock) void ragged_diag_reduce_kernel(const double* __restrict__ parts, const RaggedDiagRows* __restrict__ rows,
                                                                    unsigned first, double* __restrict__ out) {
  const RaggedDiagRows m = rows[(size_t)first + blockIdx.x];
  diag_reduce_rows(parts + (size_t)m.row_off * kDiagFields, m.rows, out + (size_t)blockIdx.x * kDiagFields);
}

}  // namespace nbx
