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

#include <string>
#include <vector>

#include "../../include/nbx_ragged_diag.h"
#include "nbx_ragged_diag_kernels.hpp"
#include "nbx_ragged_internal.hpp"

using namespace nbx;
using namespace nbx_detail;

static_assert(kDiagFields == kDiagFieldCount, "diag_fill reads kDiagFieldCount raw sums per member");

namespace {

template <typename P>
int device_alloc(P** p, size_t count, const char* what) {
  const hipError_t err = hipMalloc(p, sizeof(P) * count);
  if (err == hipSuccess) return NBX_OK;
  *p = nullptr;
  return fail(err == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE,
              std::string("nbx_ragged_diagnostics: hipMalloc of ") + what + ": " + hipGetErrorString(err));
}

// a host table (which lives in r->diag_plan as long as the object) -> a device copy, on the stream the launches follow on; *p is
// set only once the copy has been enqueued
template <typename P>
int device_table(nbx_ragged* r, P** p, const std::vector<P>& src, const char* what) {
  P* dev = nullptr;
  const int rc = device_alloc(&dev, src.size(), what);
  if (rc) return rc;
  const hipError_t err = hipMemcpyAsync(dev, src.data(), sizeof(P) * src.size(), hipMemcpyHostToDevice, r->stream);
  if (err != hipSuccess) {
    (void)hipFree(dev);
    return fail(NBX_ERR_DEVICE, std::string("nbx_ragged_diagnostics: copy of ") + what + ": " + hipGetErrorString(err));
  }
  *p = dev;
  return NBX_OK;
}

// first use: the plan, its two tables on the device, the partials and the reduced fields -- sizes fixed for the object's life
int ensure_diag_buffers(nbx_ragged* r) {
  if (!r->have_diag_plan) {
    plan_ragged_diag(r->plan, r->precision, &r->diag_plan);
    r->have_diag_plan = true;
  }
  const RaggedDiagPlan& d = r->diag_plan;
  int rc;
  if (!r->diag_part && (rc = device_alloc(&r->diag_part, (size_t)d.total_rows * kDiagFields, "the partials"))) return rc;
  if (!r->diag_dev && (rc = device_alloc(&r->diag_dev, (size_t)r->members * kDiagFields, "the reduced fields"))) return rc;
  if (!r->diag_rows_dev && (rc = device_table(r, &r->diag_rows_dev, d.rows, "the members' row table"))) return rc;
  if (!r->diag_work_dev && (rc = device_table(r, &r->diag_work_dev, d.work, "the work list"))) return rc;
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
  return guarded("nbx_ragged_diagnostics", [&]() -> int {
  if (!r || !out) return fail(NBX_ERR_ARG, "nbx_ragged_diagnostics: NULL argument");
  if (first < 0 || count < 0 || (long long)first + count > r->members)
    return fail(NBX_ERR_ARG, "nbx_ragged_diagnostics: members [first, first + count) are outside [0, members)");
  for (int k = 0; k < count; ++k)
    if (out[k].struct_size != 0 && out[k].struct_size != (int32_t)sizeof(nbx_diag_t))
      return fail(NBX_ERR_ARG, "nbx_ragged_diagnostics: out[" + std::to_string(k) + "].struct_size does not match this library");
  for (int k = first; k < first + count; ++k)
    if (!r->uploaded[k]) return fail(NBX_ERR_STATE, "nbx_ragged_diagnostics: member " + std::to_string(k) + " has not been uploaded");
  if (count == 0) return NBX_OK;
  HIP_TRY(hipSetDevice(r->device));
  const int rc = r->precision == 32 ? enqueue_ragged_diag_t<float>(r, first, count) : enqueue_ragged_diag_t<double>(r, first, count);
  if (rc) return rc;
  std::vector<double> raw((size_t)count * kDiagFields);
  HIP_TRY(hipMemcpyAsync(raw.data(), r->diag_dev, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  for (int k = 0; k < count; ++k)
    diag_fill(raw.data() + (size_t)k * kDiagFields, r->plan.member[(size_t)first + k].n, r->steps_done, out + k);
  return NBX_OK;
  });
}

}  // extern "C"
