// nbx_ragged_internal.hpp -- the ragged-ensemble object, shared by the translation units that serve it: nbx_ragged.hip (create,
// upload, step, download), nbx_ragged_diag.hip (diagnostics) nbx_batch_accel.hip (accelerations) and nbx_kick.hip (kicks).  Not part of the C-ABI (include/nbx_ragged.h is).  It names no
// kernel header, so that each of these units compiles exactly the kernels it includes itself.  What a ragged ensemble has in
// common with an ensemble -- most of its fields and all of its host plumbing -- is nbx_batch.hpp.
#pragma once
#include "../../include/nbx_ragged.h"
#include "nbx_batch.hpp"  // nbx_detail::Batch; error plumbing; nbx_plan.hpp: nbx::RaggedPlan, nbx::RaggedDiagPlan, nbx::RaggedAccelPlan

namespace nbx {
struct RaggedParts;  // nbx_ragged_kernels.hpp: the table ragged_ke_reduce_kernel reads
}

struct nbx_ragged : nbx_detail::Batch {
  static constexpr nbx_detail::BatchNames names{"nbx_ragged", "ragged ensemble"};
  nbx::RaggedPlan plan;  // per-member offsets (plan.member) and the work list as uploaded (plan.work)
  void (*launch_step)(nbx_ragged*, double dt) = nullptr;  // plan.step, resolved by nbx_ragged_create
  // ke_part is [plan.W], a member's partials together
  nbx::RaggedWork* work_dev = nullptr;    // [plan.W]
  nbx::RaggedParts* parts_dev = nullptr;  // [members]
  // diagnostics (nbx_ragged_diag.hip), all built or allocated on first use and of a size that is fixed for the object's life:
  // the work list of plan_ragged_diag and its copy on the device, the {row_off, rows} table of the reduce; diag_part is
  // [diag_plan.total_rows][9]
  nbx::RaggedDiagPlan diag_plan;
  bool have_diag_plan = false;
  nbx::RaggedDiagWork* diag_work_dev = nullptr;
  nbx::RaggedDiagRows* diag_rows_dev = nullptr;
  // accelerations (nbx_batch_accel.hip), built and uploaded on first use likewise: the member-order work list of plan_ragged_accel
  nbx::RaggedAccelPlan accel_plan;
  bool have_accel_plan = false;
  nbx::RaggedWork* accel_work_dev = nullptr;  // [plan.W]
  nbx_detail::MemberSpan layout(int k) const {
    const nbx::RaggedMember& m = plan.member[(size_t)k];
    return {m.pos_off, m.vel_off, m.n, m.n_alloc};
  }
};

#pragma GCC visibility push(hidden)  // internal to libnbx.so, as nbx_batch.hpp
namespace nbx_detail {
// nbx_ragged.hip: every member's partials -> ke_dev[slot * members + m], fixed order, on the object's stream
int enqueue_ke_reduce(nbx_ragged* r, int slot);
}  // namespace nbx_detail
#pragma GCC visibility pop
