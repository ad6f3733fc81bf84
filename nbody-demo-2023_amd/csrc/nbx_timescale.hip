// nbx_timescale.hip -- nbx_timescale, nbx_ensemble_timescale and nbx_ragged_timescale (include/nbx_timescale.h) over the kernels
// of nbx_timescale_kernels.hpp: the pair approach rate, the pair free-fall rate and the closest softened separation of a
// context's state or of any range of members, from the resident state: one pair-work launch, one reduce launch and one read-back
// for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair function is compiled once for the
// three kinds.  The launch shape of a system is the one the diagnostics give it (diag_splits, nbx_diag_shape.hpp; a ragged
// ensemble: plan_ragged_diag's work list and row table, which count ROWS and so serve rows of 3 doubles as they serve rows of
// 9) -- but nothing here depends on it: the three values are maxima and a minimum.  The call reads posm[cur] and velm and writes
// ts_part and ts_dev, buffers of its own: the trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/nbx_timescale.h"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged
#include "nbx_timescale_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

bool size_ok(const nbx_timescale_t& t) { return t.struct_size == 0 || t.struct_size == (int32_t)sizeof(nbx_timescale_t); }

// the reduced values of one system -> the public struct
void ts_fill(const double* raw, int32_t n, int64_t steps_done, nbx_timescale_t* out) {
  std::memset(out, 0, sizeof(*out));
  out->struct_size = (int32_t)sizeof(nbx_timescale_t);
  out->n = n;
  out->steps_done = steps_done;
  out->approach_rate2 = raw[0];
  out->freefall_rate2 = raw[1];
  out->min_r2 = raw[2];
}

// ts_part ([rows][3]) and ts_dev ([systems][3]): allocated on first use, of a size that is fixed for the object's life
int ensure_ts_buffers(Object* o, size_t rows, size_t systems, const char* where) {
  int rc;
  if (!o->ts_part && (rc = device_alloc(&o->ts_part, rows * kTsFields, where, "the partials"))) return rc;
  if (!o->ts_dev && (rc = device_alloc(&o->ts_dev, systems * kTsFields, where, "the reduced values"))) return rc;
  return NBX_OK;
}

template <typename T>
int enqueue_ctx_t(nbx_ctx* c, const char* where) {
  using T4 = typename V4<T>::type;
  const int columns = ceil_div(c->n, kBlock * kDiagBodies<T>);
  int splits = 1, per = 0;
  diag_splits(columns, ceil_div(c->n, kTile), &splits, &per);
  const int parts = columns * splits;
  const int rc = ensure_ts_buffers(c, (size_t)parts, 1, where);
  if (rc) return rc;
  hipLaunchKernelGGL(timescale_kernel<T>, dim3(columns, splits), dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur],
                     (const T4*)c->velm, c->n, per, c->ts_part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(timescale_reduce_kernel, dim3(1), dim3(kBlock), 0, c->stream, (const double*)c->ts_part, parts, 0u, c->ts_dev);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

// members [first, first + count) -> e->ts_dev[k * 3 ...], k = 0 .. count - 1, on the ensemble's stream
template <typename T>
int enqueue_members_t(nbx_ensemble* e, int first, int count, const char* where) {
  using T4 = typename V4<T>::type;
  const int columns = ceil_div(e->n, kBlock * kDiagBodies<T>);
  int splits = 1, per = 0;
  diag_splits(columns, ceil_div(e->n, kTile), &splits, &per);
  const int parts = columns * splits;
  const int rc = ensure_ts_buffers(e, (size_t)e->members * parts, (size_t)e->members, where);
  if (rc) return rc;
  EnsembleTsArgs<T> a{};
  a.posm = (const T4*)e->posm[e->cur];
  a.velm = (const T4*)e->velm;
  a.parts = e->ts_part;
  a.first = (unsigned)first;
  a.pos_stride = (unsigned)e->pos_stride;
  a.vel_stride = (unsigned)e->own_pad;
  a.part_stride = (unsigned)(parts * kTsFields);
  a.n = e->n;
  a.tiles_per_split = per;
  hipLaunchKernelGGL(ensemble_timescale_kernel<T>, dim3(columns, splits, count), dim3(kBlock), 0, e->stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(timescale_reduce_kernel, dim3(count), dim3(kBlock), 0, e->stream, (const double*)e->ts_part, parts, (unsigned)first,
                     e->ts_dev);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

// The work list and the row table are the diagnostics' (whichever call comes first builds them and puts them on the device).
template <typename T>
int enqueue_members_t(nbx_ragged* r, int first, int count, const char* where) {
  using T4 = typename V4<T>::type;
  if (!r->have_diag_plan) {
    plan_ragged_diag(r->plan, r->precision, &r->diag_plan);
    r->have_diag_plan = true;
  }
  const RaggedDiagPlan& d = r->diag_plan;
  int rc = ensure_ts_buffers(r, (size_t)d.total_rows, (size_t)r->members, where);
  if (rc) return rc;
  if (!r->diag_rows_dev && (rc = device_table(r, &r->diag_rows_dev, d.rows, where, "the members' row table"))) return rc;
  if (!r->diag_work_dev && (rc = device_table(r, &r->diag_work_dev, d.work, where, "the work list"))) return rc;
  const unsigned base = d.work_begin[(size_t)first], groups = d.work_begin[(size_t)first + count] - base;  // >= count: every member has a row
  RaggedTsArgs<T> a{};
  a.posm = (const T4*)r->posm[r->cur];
  a.velm = (const T4*)r->velm;
  a.parts = r->ts_part;
  a.work = r->diag_work_dev;
  a.base = base;
  hipLaunchKernelGGL(ragged_timescale_kernel<T>, dim3(groups), dim3(kBlock), 0, r->stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ragged_timescale_reduce_kernel, dim3(count), dim3(kBlock), 0, r->stream, (const double*)r->ts_part,
                     (const RaggedDiagRows*)r->diag_rows_dev, (unsigned)first, r->ts_dev);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

// nbx_ensemble_timescale and nbx_ragged_timescale: every check before the first HIP call, in the header's order
template <typename O>
int batch_timescale(O* o, const char* where, int32_t first, int32_t count, nbx_timescale_t* out) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!out) return fail(NBX_ERR_ARG, std::string(where) + ": out is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  for (int k = 0; k < count; ++k)
    if (!size_ok(out[k]))
      return fail(NBX_ERR_ARG, std::string(where) + ": out[" + std::to_string(k) + "].struct_size does not match this library");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  rc = o->precision == 32 ? enqueue_members_t<float>(o, first, count, where) : enqueue_members_t<double>(o, first, count, where);
  if (rc) return rc;
  std::vector<double> raw((size_t)count * kTsFields);
  HIP_TRY(hipMemcpyAsync(raw.data(), o->ts_dev, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  for (int k = 0; k < count; ++k) ts_fill(raw.data() + (size_t)k * kTsFields, o->layout(first + k).n, o->steps_done, out + k);
  return NBX_OK;
  });
}

}  // namespace

extern "C" {

int nbx_timescale(nbx_ctx* c, nbx_timescale_t* out) {
  constexpr const char* where = "nbx_timescale";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_timescale: ctx is NULL");
  if (!out) return fail(NBX_ERR_ARG, "nbx_timescale: out is NULL");
  if (!size_ok(*out)) return fail(NBX_ERR_ARG, "nbx_timescale: nbx_timescale_t.struct_size does not match this library");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_timescale: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_timescale: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_timescale: the context owns a slice of the bodies (the velocities of the others are not resident)");
  int rc = use_device(c);
  if (rc) return rc;
  rc = c->precision == 32 ? enqueue_ctx_t<float>(c, where) : enqueue_ctx_t<double>(c, where);
  if (rc) return rc;
  double raw[kTsFields];
  HIP_TRY(hipMemcpyAsync(raw, c->ts_dev, sizeof(raw), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  ts_fill(raw, c->n, c->steps_done, out);
  return NBX_OK;
  });
}

int nbx_ensemble_timescale(nbx_ensemble* e, int32_t first, int32_t count, nbx_timescale_t* out) {
  return batch_timescale(e, "nbx_ensemble_timescale", first, count, out);
}

int nbx_ragged_timescale(nbx_ragged* r, int32_t first, int32_t count, nbx_timescale_t* out) {
  return batch_timescale(r, "nbx_ragged_timescale", first, count, out);
}

}  // extern "C"
