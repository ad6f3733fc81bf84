// nbx_ragged_diag.hip -- nbx_ragged_diagnostics (include/nbx_ragged_diag.h) over the kernels of nbx_ragged_diag_kernels.hpp: the
// diagnostics of nbx_diag.hip for any range of a ragged ensemble's members, one pair-work launch, one reduce launch and one
// read-back for all of them.
//
// A translation unit of its own: nbx_diag.hip, nbx_ensemble_diag.hip and nbx_ragged.hip each compile to a pinned kernel set.
// The launch shape of a member is the one enqueue_diag_t (nbx_diag.hip) gives a context of n_k bodies that owns all of them
// (plan_ragged_diag, nbx_plan.hpp, over the same diag_splits), so a member's partial rows and their reduce order are a lone
// context's, and so are the bits.  The work list is in member order: the workgroups of members [first, first + count) are a
// contiguous slice of it, so a call uploads nothing.  The call reads posm[cur] and velm and writes buffers of its own: the
// trajectory, ke_part and have_parts do not see it.
#include <hip/hip_runtime.h>

#include "../../include/nbx_ragged_diag.h"
#include "nbx_ragged_diag_kernels.hpp"
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged; nbx_batch.hpp: batch_diagnostics, device_alloc, device_table

using namespace nbx;
using namespace nbx_detail;

namespace {

constexpr const char* kWhere = "nbx_ragged_diagnostics";

// first use: the plan, its two tables on the device, the partials and the reduced fields -- sizes fixed for the object's life
int ensure_diag_buffers(nbx_ragged* r) {
  if (!r->have_diag_plan) {
    plan_ragged_diag(r->plan, r->precision, &r->diag_plan);
    r->have_diag_plan = true;
  }
  const RaggedDiagPlan& d = r->diag_plan;
  int rc;
  if (!r->diag_part && (rc = device_alloc(&r->diag_part, (size_t)d.total_rows * kDiagFields, kWhere, "the partials"))) return rc;
  if (!r->diag_dev && (rc = device_alloc(&r->diag_dev, (size_t)r->members * kDiagFields, kWhere, "the reduced fields"))) return rc;
  if (!r->diag_rows_dev && (rc = device_table(r, &r->diag_rows_dev, d.rows, kWhere, "the members' row table"))) return rc;
  if (!r->diag_work_dev && (rc = device_table(r, &r->diag_work_dev, d.work, kWhere, "the work list"))) return rc;
  return NBX_OK;
}

// members [first, first + count) -> r->diag_dev[k * kDiagFields ...], k = 0 .. count - 1, on the ragged ensemble's stream
template <typename T>
int enqueue_ragged_diag_t(nbx_ragged* r, int first, int count) {
  using T4 = typename V4<T>::type;
  const int rc = ensure_diag_buffers(r);
  if (rc) return rc;
  const RaggedDiagPlan& d = r->diag_plan;
  const unsigned base = d.work_begin[(size_t)first], groups = d.work_begin[(size_t)first + count] - base;  // >= count: every member has a row
  RaggedDiagArgs<T> a{};
  a.posm = (const T4*)r->posm[r->cur];
  a.velm = (const T4*)r->velm;
  a.parts = r->diag_part;
  a.work = r->diag_work_dev;
  a.base = base;
  hipLaunchKernelGGL(ragged_diag_kernel<T>, dim3(groups), dim3(kBlock), 0, r->stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ragged_diag_reduce_kernel, dim3(count), dim3(kBlock), 0, r->stream, (const double*)r->diag_part,
                     (const RaggedDiagRows*)r->diag_rows_dev, (unsigned)first, r->diag_dev);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

}  // namespace

extern "C" {

int nbx_ragged_diagnostics(nbx_ragged* r, int32_t first, int32_t count, nbx_diag_t* out) {
  return batch_diagnostics<kDiagFields>(r, kWhere, first, count, out, [](auto t, nbx_ragged* r, int first, int count) {
    return enqueue_ragged_diag_t<decltype(t)>(r, first, count);
  });
}

}  // extern "C"
