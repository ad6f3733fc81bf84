// nbx_ensemble_internal.hpp -- the ensemble object, shared by the translation units that serve it: nbx_ensemble.hip (create,
// upload, step, download), nbx_ensemble_diag.hip (diagnostics) nbx_batch_accel.hip (accelerations) and nbx_kick.hip (kicks).  Not part of the C-ABI (include/nbx_ensemble.h is).  What an
// ensemble has in common with a ragged ensemble -- most of its fields and all of its host plumbing -- is nbx_batch.hpp.
#pragma once
#include "../../include/nbx_ensemble.h"
#include "nbx_batch.hpp"  // nbx_detail::Batch; error plumbing; nbx_plan.hpp: nbx::EnsemblePlan

struct nbx_ensemble : nbx_detail::Batch {
  static constexpr nbx_detail::BatchNames names{"nbx_ensemble", "ensemble"};
  int n = 0, own_pad = 0;  // bodies per member; records between members in velm: n rounded up to the workgroup
  size_t pos_stride = 0;   // records between members in posm: n_alloc + kSgprOverread
  nbx::EnsemblePlan plan;
  void (*launch_step)(nbx_ensemble*, double dt) = nullptr;  // plan.step, resolved by nbx_ensemble_create
  // ke_part is [members][plan.grid_x], diag_part [members][parts][9]
  nbx_detail::MemberSpan layout(int k) const { return {(size_t)k * pos_stride, (size_t)k * (size_t)own_pad, n, plan.n_alloc}; }
};
static_assert(nbx::kTile == nbx::kBlock, "own_pad == plan.n_alloc: a member's velocity records end where the next member's begin");

#pragma GCC visibility push(hidden)  // internal to libnbx.so, as nbx_batch.hpp
namespace nbx_detail {
// nbx_ensemble.hip: every member's partials -> ke_dev[slot * members + m], fixed order, on the ensemble's stream
int enqueue_ke_reduce(nbx_ensemble* e, int slot);
}  // namespace nbx_detail
#pragma GCC visibility pop
