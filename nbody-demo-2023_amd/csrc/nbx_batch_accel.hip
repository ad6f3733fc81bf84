// nbx_batch_accel.hip -- nbx_ensemble_accel and nbx_ragged_accel (include/nbx_batch_accel.h) over the kernels of
// nbx_batch_accel_kernels.hpp: what nbx_accel does for a context, for any range of the members of an ensemble or a ragged
// ensemble -- one launch, one read-back and one synchronisation for all of them.
//
// A translation unit of its own: nbx_ensemble.hip and nbx_ragged.hip each compile to a pinned kernel set.  This one instantiates
// exactly kEnsembleInstances as ensemble_accel_kernel and as ragged_accel_kernel, through the launcher table of nbx_batch.hpp,
// and launches the entry the object's plan names for its step: a member's accelerations come from the kernel body its steps run,
// over the same workgroups.  The checks, the slab, the copy and the unpack are batch_accel's (nbx_batch.hpp); here are the kernel
// arguments, the launches and a ragged ensemble's work list.  A call reads posm[cur] and velm and writes the slab alone: the
// trajectory, ke_part, have_parts, steps_done and the profile of the step kernel do not see it.
#include <hip/hip_runtime.h>

#include "../../include/nbx_batch_accel.h"
#include "nbx_batch_accel_kernels.hpp"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: batch_accel, device_table
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged; nbx_plan.hpp: plan_ragged_accel

using namespace nbx;
using namespace nbx_detail;

namespace {

// batch_accel launches only after ensure_accel_slab and the kind's prepare have succeeded: e->accm / r->accm and
// r->accel_work_dev are set in every launch below.
template <typename T>
EnsembleAccelArgs<T> ensemble_accel_args(const nbx_ensemble* e, int first) {
  using T4 = typename V4<T>::type;
  EnsembleAccelArgs<T> a{};
  a.member0.posm = (const T4*)e->posm[e->cur]; a.member0.velm = (T4*)e->velm; a.member0.accp = (T4*)e->accm;
  a.member0.i_begin = 0; a.member0.i_count = e->n; a.member0.own_pad = e->own_pad; a.member0.j_per_split = e->plan.n_alloc;
  a.member0.n_alloc = e->plan.n_alloc; a.member0.dt = (T)0;
  a.pos_stride = (unsigned)e->pos_stride; a.vel_stride = (unsigned)e->own_pad; a.first = (unsigned)first;
  return a;
}

// entry I of kEnsembleInstances as an ensemble_accel_kernel: grid (workgroups per member, members asked for)
struct EnsembleAccelLaunch {
  template <int I>
  static void run(nbx_ensemble* e, int first, int count) {
    constexpr Instance k = kEnsembleInstances[I];
    const dim3 grid(e->plan.grid_x, count);
    if constexpr (k.precision == 32)
      hipLaunchKernelGGL((ensemble_accel_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, e->stream, ensemble_accel_args<float>(e, first));
    else
      hipLaunchKernelGGL((ensemble_accel_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, e->stream, ensemble_accel_args<double>(e, first));
  }
};

template <typename T>
RaggedAccelArgs<T> ragged_accel_args(const nbx_ragged* r, unsigned base) {
  using T4 = typename V4<T>::type;
  RaggedAccelArgs<T> a{};
  a.posm = (const T4*)r->posm[r->cur]; a.velm = (T4*)r->velm; a.accm = (T4*)r->accm; a.work = r->accel_work_dev; a.base = base;
  return a;
}

// entry I of kEnsembleInstances as a ragged_accel_kernel: the slice of the member-order list that holds the members asked for
struct RaggedAccelLaunch {
  template <int I>
  static void run(nbx_ragged* r, int first, int count) {
    constexpr Instance k = kEnsembleInstances[I];
    const std::vector<unsigned>& begin = r->accel_plan.work_begin;
    const unsigned base = begin[(size_t)first], groups = begin[(size_t)first + count] - base;  // >= count: every member has a workgroup
    if constexpr (k.precision == 32)
      hipLaunchKernelGGL((ragged_accel_kernel<k.B, jlane_depth(32, k.B), k.loop>), dim3(groups), dim3(kBlock), 0, r->stream, ragged_accel_args<float>(r, base));
    else
      hipLaunchKernelGGL((ragged_accel_kernel_f64<k.B, jlane_depth(64, k.B)>), dim3(groups), dim3(kBlock), 0, r->stream, ragged_accel_args<double>(r, base));
  }
};

// first use: the member-order work list and its copy on the device -- a size fixed for the object's life
int ensure_accel_work(nbx_ragged* r, const char* where) {
  if (!r->have_accel_plan) {
    plan_ragged_accel(r->plan, &r->accel_plan);
    r->have_accel_plan = true;
  }
  if (r->accel_work_dev) return NBX_OK;
  return device_table(r, &r->accel_work_dev, r->accel_plan.work, where, "the work list");
}

}  // namespace

extern "C" {

int nbx_ensemble_accel(nbx_ensemble* e, int32_t first, int32_t count, void* acc_x, void* acc_y, void* acc_z) {
  return batch_accel<nbx_ensemble, EnsembleAccelLaunch>(e, "nbx_ensemble_accel", first, count, acc_x, acc_y, acc_z,
                                                        [](nbx_ensemble*) { return (int)NBX_OK; });
}

int nbx_ragged_accel(nbx_ragged* r, int32_t first, int32_t count, void* acc_x, void* acc_y, void* acc_z) {
  return batch_accel<nbx_ragged, RaggedAccelLaunch>(r, "nbx_ragged_accel", first, count, acc_x, acc_y, acc_z,
                                                    [](nbx_ragged* r) { return ensure_accel_work(r, "nbx_ragged_accel"); });
}

}  // extern "C"
