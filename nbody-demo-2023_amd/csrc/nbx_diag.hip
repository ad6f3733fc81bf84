// nbx_diag.hip -- nbx_diagnostics (include/nbx_diag.h) over the kernels of nbx_diag_kernels.hpp: mass, kinetic and potential
// energy, momentum and mass moment of a context's owned bodies at its current state.  nbx_group_diagnostics, which needs
// the group object, lives in nbx_group.hip and uses enqueue_diagnostics / diag_fill from here.
//
// The launch shape depends on the state's size only (i_count, n, precision), never on the context's force options, so
// every context holding the same state returns the same bits.  The call reads posm[cur] and velm and writes buffers of its
// own: the trajectory does not see it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "nbx_diag_kernels.hpp"
#include "nbx_internal.hpp"

using namespace nbx;
using namespace nbx_detail;

static_assert(kDiagFields == kDiagFieldCount, "nbx_group.hip sizes the all-gather of the partials by kDiagFieldCount");

namespace {

template <typename T>
int enqueue_diag_t(nbx_ctx* c, const char* where) {
  using T4 = typename V4<T>::type;
  constexpr int B = kDiagBodies<T>;
  const int blocks = ceil_div(c->i_count, kBlock * B);
  int splits = 1, per = 0;
  diag_splits(blocks, ceil_div(c->n, kTile), &splits, &per);
  const int parts = blocks * splits;  // i_count and n are fixed for the context's life: so is the size of diag_part
  int rc = NBX_OK;
  if (!c->diag_part && (rc = device_alloc(&c->diag_part, kDiagFields * (size_t)parts, where, "the partials"))) return rc;
  if (!c->diag_dev && (rc = device_alloc(&c->diag_dev, (size_t)kDiagFields, where, "the reduced fields"))) return rc;
  hipLaunchKernelGGL((diag_kernel<T, B>), dim3(blocks, splits), dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur],
                     (const T4*)c->velm, c->i_begin, c->i_count, c->n, per, c->diag_part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(diag_reduce_kernel, dim3(1), dim3(kBlock), 0, c->stream, (const double*)c->diag_part, parts, c->diag_dev);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

}  // namespace

int nbx_detail::enqueue_diagnostics(nbx_ctx* c, const char* where) {
  if (!c->uploaded) return fail(NBX_ERR_STATE, std::string(where) + ": nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, std::string(where) + ": a local step awaits nbx_commit");
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? enqueue_diag_t<float>(c, where) : enqueue_diag_t<double>(c, where);
}

void nbx_detail::diag_fill(const double* raw, int32_t i_count, int64_t steps_done, nbx_diag_t* out) {
  std::memset(out, 0, sizeof(*out));
  out->struct_size = (int32_t)sizeof(nbx_diag_t);
  out->i_count = i_count;
  out->steps_done = steps_done;
  out->mass = raw[0];
  out->kenergy = 0.5 * raw[1];  // ver7/GSimulation.cpp:200, as nbx_step
  out->potential = -0.5 * raw[2];
  for (int k = 0; k < 3; ++k) {
    out->momentum[k] = raw[3 + k];
    out->mass_moment[k] = raw[6 + k];
  }
}

extern "C" {

int nbx_diagnostics(nbx_ctx* c, nbx_diag_t* out) {
  return guarded("nbx_diagnostics", [&]() -> int {
  if (!c || !out) return fail(NBX_ERR_ARG, "nbx_diagnostics: NULL argument");
  if (out->struct_size != 0 && out->struct_size != (int32_t)sizeof(nbx_diag_t))
    return fail(NBX_ERR_ARG, "nbx_diagnostics: nbx_diag_t.struct_size does not match this library");
  int rc = enqueue_diagnostics(c, "nbx_diagnostics");
  if (rc) return rc;
  double raw[kDiagFields];
  HIP_TRY(hipMemcpyAsync(raw, c->diag_dev, sizeof(raw), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  diag_fill(raw, c->i_count, c->steps_done, out);
  return NBX_OK;
  });
}

}  // extern "C"
