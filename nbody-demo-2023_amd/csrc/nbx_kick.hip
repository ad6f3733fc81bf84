// nbx_kick.hip -- nbx_kick, nbx_ensemble_kick and nbx_ragged_kick (include/nbx_kick.h) over the kernels of nbx_kick_kernels.hpp:
// v += a(x) * h for every owned body at the current positions.  (nbx_group_kick is nbx_group.hip's: it loops over the ranks.)
//
// A translation unit of its own: nbx_api.hip, nbx_ensemble.hip, nbx_ragged.hip and nbx_batch_accel.hip each compile to a pinned
// kernel set.  This one instantiates exactly kEnsembleInstances as ensemble_kick_kernel and as ragged_kick_kernel, through the
// launcher table of kick_common (nbx_batch.hpp), and kick_kernel in the two precisions.
//   An ensemble or a ragged ensemble: one launch of the entry the object's plan names for its step, over the step's grid (the
//   step's work list).  The checks, have_parts and the energy read-back are kick_common's; here are the kernel arguments.
//   A context: the acc-only force launch nbx_accel reads back (enqueue_accel_slabs, nbx_api.hip -- every kernel variant and both
//   summation orders), then kick_kernel over the slabs.  ke_parts then counts kick_kernel's workgroups, as after a step that
//   ended in integrate_kernel.
// A kick reads posm[cur] and writes velm and ke_part: cur, steps_done, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/nbx_kick.h"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: kick_common
#include "nbx_internal.hpp"           // struct nbx_ctx; enqueue_accel_slabs, enqueue_ke_reduce
#include "nbx_kick_kernels.hpp"
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

template <typename T>
EnsembleKickArgs<T> ensemble_kick_args(const nbx_ensemble* e, double h) {
  using T4 = typename V4<T>::type;
  EnsembleKickArgs<T> a{};
  a.member0.posm = (const T4*)e->posm[e->cur]; a.member0.velm = (T4*)e->velm; a.member0.ke_part = e->ke_part;
  a.member0.i_begin = 0; a.member0.i_count = e->n; a.member0.own_pad = e->own_pad; a.member0.j_per_split = e->plan.n_alloc;
  a.member0.n_alloc = e->plan.n_alloc; a.member0.dt = (T)h;
  a.pos_stride = (unsigned)e->pos_stride; a.vel_stride = (unsigned)e->own_pad; a.ke_stride = (unsigned)e->plan.grid_x;
  return a;
}

// entry I of kEnsembleInstances as an ensemble_kick_kernel: the step's grid
struct EnsembleKickLaunch {
  template <int I>
  static void run(nbx_ensemble* e, double h) {
    constexpr Instance k = kEnsembleInstances[I];
    const dim3 grid(e->plan.grid_x, e->plan.grid_y);
    if constexpr (k.precision == 32)
      hipLaunchKernelGGL((ensemble_kick_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, e->stream, ensemble_kick_args<float>(e, h));
    else
      hipLaunchKernelGGL((ensemble_kick_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, e->stream, ensemble_kick_args<double>(e, h));
  }
};

template <typename T>
RaggedKickArgs<T> ragged_kick_args(const nbx_ragged* r, double h) {
  using T4 = typename V4<T>::type;
  RaggedKickArgs<T> a{};
  a.posm = (const T4*)r->posm[r->cur]; a.velm = (T4*)r->velm; a.ke_part = r->ke_part; a.work = r->work_dev; a.h = (T)h;
  return a;
}

// entry I of kEnsembleInstances as a ragged_kick_kernel: the step's work list
struct RaggedKickLaunch {
  template <int I>
  static void run(nbx_ragged* r, double h) {
    constexpr Instance k = kEnsembleInstances[I];
    const dim3 grid(r->plan.W);
    if constexpr (k.precision == 32)
      hipLaunchKernelGGL((ragged_kick_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, r->stream, ragged_kick_args<float>(r, h));
    else
      hipLaunchKernelGGL((ragged_kick_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, r->stream, ragged_kick_args<double>(r, h));
  }
};

// a context's two launches, beside accel_t (nbx_api.hip): what that reads back and adds on the host, this adds on the device
template <typename T>
int kick_t(nbx_ctx* c, double h) {
  using T4 = typename V4<T>::type;
  const int rc = enqueue_accel_slabs(c);
  if (rc) return rc;
  const int blocks = ceil_div(c->i_count, kBlock);  // <= the partials ke_part was allocated for (nbx_create)
  hipLaunchKernelGGL((kick_kernel<T>), dim3(blocks), dim3(kBlock), 0, c->stream, (T4*)c->velm, (const T4*)c->accp, c->plan.S, c->own_pad,
                     c->i_count, (T)h, c->ke_part);
  HIP_TRY(hipGetLastError());
  c->ke_parts = blocks;
  return NBX_OK;
}

}  // namespace

extern "C" {

int nbx_kick(nbx_ctx* c, double h, double* kenergy_out) {
  return guarded("nbx_kick", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_kick: ctx is NULL");
  if (!std::isfinite(h)) return fail(NBX_ERR_ARG, "nbx_kick: h is not finite");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_kick: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_kick: a local step awaits nbx_commit");
  int rc = use_device(c);
  if (rc) return rc;
  rc = c->precision == 32 ? kick_t<float>(c, h) : kick_t<double>(c, h);
  if (rc) return rc;
  if (kenergy_out) {  // ke_dev holds at least one sum from nbx_create on
    rc = enqueue_ke_reduce(c, 0);
    if (rc) return rc;
  }
  return read_energies(c, 1, 1, true, kenergy_out, nullptr, [] { return (int)NBX_OK; });
  });
}

int nbx_ensemble_kick(nbx_ensemble* e, double h, double* kenergy_out) {
  return kick_common<nbx_ensemble, EnsembleKickLaunch>(e, "nbx_ensemble_kick", h, kenergy_out);
}

int nbx_ragged_kick(nbx_ragged* r, double h, double* kenergy_out) {
  return kick_common<nbx_ragged, RaggedKickLaunch>(r, "nbx_ragged_kick", h, kenergy_out);
}

}  // extern "C"
