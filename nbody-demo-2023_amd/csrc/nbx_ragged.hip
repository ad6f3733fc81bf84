// nbx_ragged.hip -- include/nbx_ragged.h over the kernels of nbx_ragged_kernels.hpp: independent systems of different size, one
// launch per time step for all of them.  The layout, the work list and the kernel instance come from plan_ragged
// (nbx_plan.hpp); this file instantiates exactly kEnsembleInstances -- the shapes a jlane context can run -- as
// ragged_step_kernel and launches the one the plan names.  The host plumbing -- the step loop, upload and download, profiling,
// the shared part of create and destroy -- is nbx_batch.hpp's and, under it, nbx_object.hpp's; here are the kernel arguments, the launches and what of create,
// destroy and stats belongs to a ragged ensemble.
//
// Plain launches on the object's own non-blocking stream, no graph capture, as for an ensemble (nbx_ensemble.hip).
#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "nbx_ragged_internal.hpp"  // struct nbx_ragged; nbx_batch.hpp; nbx_plan.hpp: nbx::RaggedPlan
#include "nbx_ragged_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

template <typename T>
RaggedArgs<T> ragged_args(const nbx_ragged* r, double dt) {
  using T4 = typename V4<T>::type;
  RaggedArgs<T> a{};
  a.posm = (const T4*)r->posm[r->cur]; a.posm_next = (T4*)r->posm[r->cur ^ 1];
  a.velm = (T4*)r->velm; a.ke_part = r->ke_part; a.work = r->work_dev; a.dt = (T)dt;
  return a;
}

// entry I of kEnsembleInstances as a ragged_step_kernel: the only instances of it this library compiles
struct RaggedLaunch {
  template <int I>
  static void run(nbx_ragged* r, double dt) {
    constexpr Instance k = kEnsembleInstances[I];
    const dim3 grid(r->plan.W);
    if constexpr (k.precision == 32)
      hipLaunchKernelGGL((ragged_step_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, r->stream, ragged_args<float>(r, dt));
    else
      hipLaunchKernelGGL((ragged_step_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, r->stream, ragged_args<double>(r, dt));
  }
};

}  // namespace

// every member's partials -> ke_dev[slot * members + m], fixed order (the step loop of nbx_batch.hpp calls it)
int nbx_detail::enqueue_ke_reduce(nbx_ragged* r, int slot) {
  hipLaunchKernelGGL(ragged_ke_reduce_kernel, dim3(r->members), dim3(kBlock), 0, r->stream, (const double*)r->ke_part,
                     (const RaggedParts*)r->parts_dev, r->ke_dev + (size_t)slot * r->members);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

extern "C" {

int nbx_ragged_create(nbx_ragged** out, int32_t members, const int32_t* n, int32_t precision, const nbx_opts* opts) {
  constexpr const char* where = "nbx_ragged_create";
  return guarded(where, [&]() -> int {
  nbx_opts o;
  int rc = create_opts(where, out, opts, &o);
  if (rc) return rc;
  // every argument check before the first HIP call: whether a plan exists does not depend on the device (its CU count only
  // moves the choice of bodies per wave, and auto never picks a shape without an instance)
  static_assert(std::is_same<int32_t, int>::value, "plan_ragged reads the sizes as int");
  const char* msg = nullptr;
  {
    RaggedPlan plan;
    if (plan_ragged(n, members, precision, 0, o, &plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);
  }

  BatchOwner<nbx_ragged> owner{nbx_ragged_destroy};
  rc = batch_open(where, o, precision, &owner);
  if (rc) return rc;
  nbx_ragged* r = owner.o;
  set_members(r, members);
  if (plan_ragged(n, members, precision, r->prop.multiProcessorCount, o, &r->plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);
  rc = resolve_launcher<nbx_ragged, RaggedLaunch>(r, where);
  if (rc) return rc;

  const RaggedPlan& p = r->plan;
  std::vector<RaggedParts> parts((size_t)members);
  for (int m = 0; m < members; ++m) parts[(size_t)m] = {p.member[(size_t)m].ke_off, p.member[(size_t)m].grid};
  const size_t pos_bytes = r->rec * (size_t)p.pos_records, vel_bytes = r->rec * (size_t)p.vel_records;
  const size_t part_bytes = sizeof(double) * (size_t)p.ke_parts, work_bytes = sizeof(RaggedWork) * p.work.size();
  CREATE_TRY(where, hipMalloc(&r->posm[0], pos_bytes));
  CREATE_TRY(where, hipMalloc(&r->posm[1], pos_bytes));
  CREATE_TRY(where, hipMalloc(&r->velm, vel_bytes));
  CREATE_TRY(where, hipMalloc(&r->ke_part, part_bytes));
  CREATE_TRY(where, hipMalloc(&r->work_dev, work_bytes));
  CREATE_TRY(where, hipMalloc(&r->parts_dev, sizeof(RaggedParts) * parts.size()));
  CREATE_TRY(where, hipMemsetAsync(r->posm[0], 0, pos_bytes, r->stream));
  CREATE_TRY(where, hipMemsetAsync(r->posm[1], 0, pos_bytes, r->stream));
  CREATE_TRY(where, hipMemsetAsync(r->velm, 0, vel_bytes, r->stream));
  CREATE_TRY(where, hipMemsetAsync(r->ke_part, 0, part_bytes, r->stream));
  CREATE_TRY(where, hipMemcpyAsync(r->work_dev, p.work.data(), work_bytes, hipMemcpyHostToDevice, r->stream));
  CREATE_TRY(where, hipMemcpyAsync(r->parts_dev, parts.data(), sizeof(RaggedParts) * parts.size(), hipMemcpyHostToDevice, r->stream));
  CREATE_TRY(where, hipStreamSynchronize(r->stream));
  *out = owner.release();
  last_error().clear();
  return NBX_OK;
  });
}

void nbx_ragged_destroy(nbx_ragged* r) {
  if (!r) return;
  batch_quiesce(r);
  if (r->work_dev) (void)hipFree(r->work_dev);
  if (r->parts_dev) (void)hipFree(r->parts_dev);
  if (r->diag_work_dev) (void)hipFree(r->diag_work_dev);  // the tables of nbx_ragged_diag.hip
  if (r->diag_rows_dev) (void)hipFree(r->diag_rows_dev);
  if (r->accel_work_dev) (void)hipFree(r->accel_work_dev);  // the table and the slab of nbx_batch_accel.hip
  if (r->accm) (void)hipFree(r->accm);
  batch_release(r);
  delete r;
}

int nbx_ragged_upload(nbx_ragged* r, int32_t first, int32_t count, const void* px, const void* py, const void* pz, const void* vx,
                      const void* vy, const void* vz, const void* m) {
  return batch_upload(r, "nbx_ragged_upload", first, count, px, py, pz, vx, vy, vz, m);
}

int nbx_ragged_step(nbx_ragged* r, double dt, int32_t nsteps, double* kenergy_out) {
  return step_common(r, "nbx_ragged_step", dt, nsteps, kenergy_out, nullptr);
}

int nbx_ragged_step_trace(nbx_ragged* r, double dt, int32_t nsteps, double* ke_trace) {
  return step_trace(r, "nbx_ragged_step_trace", dt, nsteps, ke_trace);
}

int nbx_ragged_download(nbx_ragged* r, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return batch_download(r, "nbx_ragged_download", first, count, px, py, pz, vx, vy, vz);
}

int nbx_ragged_sync(nbx_ragged* r) { return batch_sync(r, "nbx_ragged_sync"); }

int nbx_ragged_profile(nbx_ragged* r, int32_t enable) { return batch_profile(r, "nbx_ragged_profile", enable); }

int nbx_ragged_stats(nbx_ragged* r, nbx_ragged_stats_t* s) {
  return batch_stats(r, s, "nbx_ragged_stats", [r](nbx_ragged_stats_t* s) {
    s->n_min = r->plan.n_min; s->n_max = r->plan.n_max; s->bodies_total = (int32_t)r->plan.bodies_total;
    s->bodies_per_lane = r->plan.NB; s->inner_loop = r->plan.loop == LOOP_ASM ? NBX_LOOP_ASM : NBX_LOOP_CXX;
    s->grid_x = r->plan.W; s->pairs_per_step = r->plan.pairs_per_step;
  });
}

}  // extern "C"
