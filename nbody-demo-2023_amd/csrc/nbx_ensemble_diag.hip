// nbx_ensemble_diag.hip -- nbx_ensemble_diagnostics (include/nbx_ensemble_diag.h) over the kernels of
// nbx_ensemble_diag_kernels.hpp: the diagnostics of nbx_diag.hip for any range of an ensemble's members, one pair-work launch,
// one reduce launch and one read-back for all of them.
//
// A translation unit of its own: nbx_diag.hip and nbx_ensemble.hip each compile to a pinned kernel set.  The launch shape of a
// member is the one enqueue_diag_t (nbx_diag.hip) gives a context of n bodies that owns all of them -- columns, j splits and
// tiles per split from (n, precision) alone -- so a member's partial rows and their reduce order are a lone context's, and so
// are the bits.  The call reads posm[cur] and velm and writes buffers of its own: the trajectory does not see it.
#include <hip/hip_runtime.h>

#include "../../include/nbx_ensemble_diag.h"
#include "nbx_ensemble_diag_kernels.hpp"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: batch_diagnostics, device_alloc

using namespace nbx;
using namespace nbx_detail;

namespace {

constexpr const char* kWhere = "nbx_ensemble_diagnostics";

// members [first, first + count) -> e->diag_dev[k * kDiagFields ...], k = 0 .. count - 1, on the ensemble's stream
template <typename T>
int enqueue_ensemble_diag_t(nbx_ensemble* e, int first, int count) {
  using T4 = typename V4<T>::type;
  constexpr int B = kDiagBodies<T>;
  const int columns = ceil_div(e->n, kBlock * B);
  int splits = 1, per = 0;
  diag_splits(columns, ceil_div(e->n, kTile), &splits, &per);
  const int parts = columns * splits;  // n is fixed for the ensemble's life: so are the sizes of diag_part and diag_dev
  if (!e->diag_part) {
    const int rc = device_alloc(&e->diag_part, (size_t)e->members * parts * kDiagFields, kWhere, "the partials");
    if (rc) return rc;
  }
  if (!e->diag_dev) {
    const int rc = device_alloc(&e->diag_dev, (size_t)e->members * kDiagFields, kWhere, "the reduced fields");
    if (rc) return rc;
  }
  EnsembleDiagArgs<T> a{};
  a.posm = (const T4*)e->posm[e->cur];
  a.velm = (const T4*)e->velm;
  a.parts = e->diag_part;
  a.first = (unsigned)first;
  a.pos_stride = (unsigned)e->pos_stride;
  a.vel_stride = (unsigned)e->own_pad;
  a.part_stride = (unsigned)(parts * kDiagFields);
  a.n = e->n;
  a.tiles_per_split = per;
  hipLaunchKernelGGL(ensemble_diag_kernel<T>, dim3(columns, splits, count), dim3(kBlock), 0, e->stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ensemble_diag_reduce_kernel, dim3(count), dim3(kBlock), 0, e->stream, (const double*)e->diag_part, parts,
                     (unsigned)first, e->diag_dev);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

}  // namespace

extern "C" {

int nbx_ensemble_diagnostics(nbx_ensemble* e, int32_t first, int32_t count, nbx_diag_t* out) {
  return batch_diagnostics<kDiagFields>(e, kWhere, first, count, out, [](auto t, nbx_ensemble* e, int first, int count) {
    return enqueue_ensemble_diag_t<decltype(t)>(e, first, count);
  });
}

}  // extern "C"
