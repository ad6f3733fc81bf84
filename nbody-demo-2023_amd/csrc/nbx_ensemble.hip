// nbx_ensemble.hip -- include/nbx_ensemble.h over the kernels of nbx_ensemble_kernels.hpp: S independent systems of n bodies,
// one launch per time step for all of them.  The launch shape and the kernel instance come from plan_ensemble (nbx_plan.hpp);
// this file instantiates exactly kEnsembleInstances and launches the one the plan names.  The host plumbing -- the step loop,
// upload and download, profiling, the shared part of create and destroy -- is nbx_batch.hpp's and, under it, nbx_object.hpp's; here are the kernel arguments,
// the launches and what of create and stats belongs to an ensemble.
//
// Plain launches on the ensemble's own non-blocking stream, no graph capture: one launch per step costs the host 3-4 us, and
// an ensemble worth creating has more pair work per step than that (64 members of 2048 bodies: 2.7e8 pairs).
#include <hip/hip_runtime.h>

#include "nbx_ensemble_internal.hpp"
#include "nbx_ensemble_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

template <typename T>
EnsembleArgs<T> ensemble_args(const nbx_ensemble* e, double dt) {
  using T4 = typename V4<T>::type;
  EnsembleArgs<T> a{};
  a.member0.posm = (const T4*)e->posm[e->cur]; a.member0.posm_next = (T4*)e->posm[e->cur ^ 1];
  a.member0.velm = (T4*)e->velm; a.member0.ke_part = e->ke_part;
  a.member0.i_begin = 0; a.member0.i_count = e->n; a.member0.own_pad = e->own_pad; a.member0.j_per_split = e->plan.n_alloc;
  a.member0.n_alloc = e->plan.n_alloc; a.member0.dt = (T)dt;
  a.pos_stride = (unsigned)e->pos_stride; a.vel_stride = (unsigned)e->own_pad; a.ke_stride = (unsigned)e->plan.grid_x;
  return a;
}

// entry I of kEnsembleInstances as an ensemble_step_kernel: the only instances of it this library compiles
struct EnsembleLaunch {
  template <int I>
  static void run(nbx_ensemble* e, double dt) {
    constexpr Instance k = kEnsembleInstances[I];
    const dim3 grid(e->plan.grid_x, e->plan.grid_y);
    if constexpr (k.precision == 32)
      hipLaunchKernelGGL((ensemble_step_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, e->stream, ensemble_args<float>(e, dt));
    else
      hipLaunchKernelGGL((ensemble_step_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, e->stream, ensemble_args<double>(e, dt));
  }
};

}  // namespace

// every member's partials -> ke_dev[slot * members + m], fixed order (the step loop of nbx_batch.hpp calls it)
int nbx_detail::enqueue_ke_reduce(nbx_ensemble* e, int slot) {
  hipLaunchKernelGGL(ensemble_ke_reduce_kernel, dim3(e->members), dim3(kBlock), 0, e->stream, (const double*)e->ke_part, e->plan.grid_x,
                     e->ke_dev + (size_t)slot * e->members);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

extern "C" {

int nbx_ensemble_create(nbx_ensemble** out, int32_t n, int32_t precision, int32_t members, const nbx_opts* opts) {
  constexpr const char* where = "nbx_ensemble_create";
  return guarded(where, [&]() -> int {
  nbx_opts o;
  int rc = create_opts(where, out, opts, &o);
  if (rc) return rc;
  // every argument check before the first HIP call: whether a plan exists does not depend on the device (its CU count only
  // moves the choice of bodies per wave, and auto never picks a shape without an instance)
  EnsemblePlan plan;
  const char* msg = nullptr;
  if (plan_ensemble(n, precision, members, 0, o, &plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);

  BatchOwner<nbx_ensemble> owner{nbx_ensemble_destroy};
  rc = batch_open(where, o, precision, &owner);
  if (rc) return rc;
  nbx_ensemble* e = owner.o;
  set_members(e, members);
  e->n = n;
  e->own_pad = round_up(n, kBlock);
  if (plan_ensemble(n, precision, members, e->prop.multiProcessorCount, o, &e->plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);
  rc = resolve_launcher<nbx_ensemble, EnsembleLaunch>(e, where);
  if (rc) return rc;

  e->pos_stride = (size_t)e->plan.n_alloc + kSgprOverread;
  const size_t pos_bytes = e->rec * e->pos_stride * (size_t)members, vel_bytes = e->rec * (size_t)e->own_pad * (size_t)members;
  const size_t part_bytes = sizeof(double) * (size_t)e->plan.grid_x * (size_t)members;
  CREATE_TRY(where, hipMalloc(&e->posm[0], pos_bytes));
  CREATE_TRY(where, hipMalloc(&e->posm[1], pos_bytes));
  CREATE_TRY(where, hipMalloc(&e->velm, vel_bytes));
  CREATE_TRY(where, hipMalloc(&e->ke_part, part_bytes));
  CREATE_TRY(where, hipMemsetAsync(e->posm[0], 0, pos_bytes, e->stream));
  CREATE_TRY(where, hipMemsetAsync(e->posm[1], 0, pos_bytes, e->stream));
  CREATE_TRY(where, hipMemsetAsync(e->velm, 0, vel_bytes, e->stream));
  CREATE_TRY(where, hipMemsetAsync(e->ke_part, 0, part_bytes, e->stream));
  CREATE_TRY(where, hipStreamSynchronize(e->stream));
  *out = owner.release();
  last_error().clear();
  return NBX_OK;
  });
}

void nbx_ensemble_destroy(nbx_ensemble* e) {
  if (!e) return;
  batch_quiesce(e);
  if (e->accm) (void)hipFree(e->accm);  // the slab of nbx_batch_accel.hip
  batch_release(e);                     // every other device buffer of an ensemble is one every object has
  delete e;
}

int nbx_ensemble_upload(nbx_ensemble* e, int32_t first, int32_t count, const void* px, const void* py, const void* pz, const void* vx,
                        const void* vy, const void* vz, const void* m) {
  return batch_upload(e, "nbx_ensemble_upload", first, count, px, py, pz, vx, vy, vz, m);
}

int nbx_ensemble_step(nbx_ensemble* e, double dt, int32_t nsteps, double* kenergy_out) {
  return step_common(e, "nbx_ensemble_step", dt, nsteps, kenergy_out, nullptr);
}

int nbx_ensemble_step_trace(nbx_ensemble* e, double dt, int32_t nsteps, double* ke_trace) {
  return step_trace(e, "nbx_ensemble_step_trace", dt, nsteps, ke_trace);
}

int nbx_ensemble_download(nbx_ensemble* e, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return batch_download(e, "nbx_ensemble_download", first, count, px, py, pz, vx, vy, vz);
}

int nbx_ensemble_sync(nbx_ensemble* e) { return batch_sync(e, "nbx_ensemble_sync"); }

int nbx_ensemble_profile(nbx_ensemble* e, int32_t enable) { return batch_profile(e, "nbx_ensemble_profile", enable); }

int nbx_ensemble_stats(nbx_ensemble* e, nbx_ensemble_stats_t* s) {
  return batch_stats(e, s, "nbx_ensemble_stats", [e](nbx_ensemble_stats_t* s) {
    s->n = e->n; s->n_alloc = e->plan.n_alloc;
    s->bodies_per_lane = e->plan.NB; s->inner_loop = e->plan.loop == LOOP_ASM ? NBX_LOOP_ASM : NBX_LOOP_CXX;
    s->grid_x = e->plan.grid_x; s->grid_y = e->plan.grid_y;
  });
}

}  // extern "C"
