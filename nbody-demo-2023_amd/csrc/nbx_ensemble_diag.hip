// nbx_ensemble_diag.hip -- nbx_ensemble_diagnostics (include/nbx_ensemble_diag.h) over the kernels of
// nbx_ensemble_diag_kernels.hpp: the diagnostics of nbx_diag.hip for any range of an ensemble's members, one pair-work launch,
// one reduce launch and one read-back for all of them.
//
// A translation unit of its own: nbx_diag.hip and nbx_ensemble.hip each compile to a pinned kernel set.  The launch shape of a
// member is the one enqueue_diag_t (nbx_diag.hip) gives a context of n bodies that owns all of them -- columns, j splits and
// tiles per split from (n, precision) alone -- so a member's partial rows and their reduce order are a lone context's, and so
// are the bits.  The call reads posm[cur] and velm and writes buffers of its own: the trajectory does not see it.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/nbx_ensemble_diag.h"
#include "nbx_ensemble_diag_kernels.hpp"
#include "nbx_ensemble_internal.hpp"

using namespace nbx;
using namespace nbx_detail;

static_assert(kDiagFields == kDiagFieldCount, "diag_fill reads kDiagFieldCount raw sums per member");

namespace {

int device_alloc(double** p, size_t doubles, const char* what) {
  const hipError_t err = hipMalloc(p, sizeof(double) * doubles);
  if (err == hipSuccess) return NBX_OK;
  *p = nullptr;
  return fail(err == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE,
              std::string("nbx_ensemble_diagnostics: hipMalloc of ") + what + ": " + hipGetErrorString(err));
}

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
    const int rc = device_alloc(&e->diag_part, (size_t)e->members * parts * kDiagFields, "the partials");
    if (rc) return rc;
  }
  if (!e->diag_dev) {
    const int rc = device_alloc(&e->diag_dev, (size_t)e->members * kDiagFields, "the reduced fields");
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
  return guarded("nbx_ensemble_diagnostics", [&]() -> int {
  if (!e || !out) return fail(NBX_ERR_ARG, "nbx_ensemble_diagnostics: NULL argument");
  if (first < 0 || count < 0 || (long long)first + count > e->members)
    return fail(NBX_ERR_ARG, "nbx_ensemble_diagnostics: members [first, first + count) are outside [0, members)");
  for (int k = 0; k < count; ++k)
    if (out[k].struct_size != 0 && out[k].struct_size != (int32_t)sizeof(nbx_diag_t))
      return fail(NBX_ERR_ARG, "nbx_ensemble_diagnostics: out[" + std::to_string(k) + "].struct_size does not match this library");
  for (int k = first; k < first + count; ++k)
    if (!e->uploaded[k]) return fail(NBX_ERR_STATE, "nbx_ensemble_diagnostics: member " + std::to_string(k) + " has not been uploaded");
  if (count == 0) return NBX_OK;
  HIP_TRY(hipSetDevice(e->device));
  const int rc = e->precision == 32 ? enqueue_ensemble_diag_t<float>(e, first, count) : enqueue_ensemble_diag_t<double>(e, first, count);
  if (rc) return rc;
  std::vector<double> raw((size_t)count * kDiagFields);
  HIP_TRY(hipMemcpyAsync(raw.data(), e->diag_dev, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < count; ++k) diag_fill(raw.data() + (size_t)k * kDiagFields, e->n, e->steps_done, out + k);
  return NBX_OK;
  });
}

}  // extern "C"
