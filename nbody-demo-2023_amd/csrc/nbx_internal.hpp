// nbx_internal.hpp -- the context object and what the translation units that serve it share (nbx_api.hip, nbx_group.hip,
// nbx_diag.hip, nbx_kick.hip).  What a context has in common with the batch objects -- error plumbing, most of its fields, device choice,
// profiling, the shared part of create and destroy -- is nbx_object.hpp.  Not part of the C-ABI (include/nbx.h is); nothing
// here is visible outside the library.
#pragma once
#include "../../include/nbx_diag.h"  // includes nbx.h
#include "nbx_object.hpp"            // nbx_detail::Object; error plumbing
#include "nbx_plan.hpp"              // ceil_div, round_up, nbx::Plan

struct nbx_ctx : nbx_detail::Object {
  static constexpr nbx_detail::BatchNames names{"nbx", "ctx"};
  int n = 0, n_alloc = 0, i_begin = 0, i_count = 0, own_pad = 0;
  nbx::Plan plan;  // launch shape and kernel instances (nbx_plan.hpp)
  void (*launch_step)(nbx_ctx*, double dt, int acc_only) = nullptr;  // plan.step and plan.accel, resolved by nbx_create
  void (*launch_accel)(nbx_ctx*, double dt, int acc_only) = nullptr;
  unsigned slice_bit = 0;  // LOOP_ASM_TS: clock bit of the priority slices
  void* accp = nullptr;
  void* mass_all = nullptr;        // NBX_KERNEL_EXACT only: m of every body (the records carry G*m)
  void* posm_pairs = nullptr;      // one body per lane + hand-scheduled loop only: pair-interleaved copy of posm[cur], rebuilt every step
  int ke_parts = 0;       // partials in ke_part written by the last step
  bool uploaded = false;
  bool pending_commit = false;
  // hipGraph replay of multi-step windows (launch-bound small n; plan.use_graph)
  struct GraphUnit { int steps; int parity; double dt; hipGraphExec_t exec; };
  std::vector<GraphUnit> graphs;
  long long graph_replays = 0;
};

namespace nbx_detail {
// shared by the context entry points (nbx_api.hip) and the groups (nbx_group.hip)
double model_force_cost(const nbx_ctx* c, int own);  // relative cost of one force launch if the context owned `own` bodies (the tuner's predictor)
int enqueue_ke_reduce(nbx_ctx* c, int slot);  // ke_part[0 .. ke_parts) -> ke_dev[slot], fixed order, on the context's stream
// nbx_api.hip, for nbx_kick.hip: nbx_accel's acc-only force launch on the context's stream, outside the profile of the force kernel;
// accp then holds plan.S slabs of own_pad records once the stream gets there.  The caller has checked the state and chosen the device.
int enqueue_accel_slabs(nbx_ctx* c);
// nbx_api.hip, for nbx_tracers.hip: one step of an unsliced context as nbx_step's plain loop enqueues it -- the step's launches on
// the context's stream (timed like nbx_step's), then cur flipped and steps_done counted.  The caller has checked the state and
// chosen the device.
int enqueue_one_step(nbx_ctx* c, double dt);
constexpr int kDiagFieldCount = 9;  // = nbx::kDiagFields (nbx_diag_kernels.hpp; checked in nbx_diag.hip)
// nbx_diag.hip: checks the context's state, then enqueues the diagnostics kernels on its stream; c->diag_dev then holds the
// kDiagFields raw sums (nbx_diag_kernels.hpp) once the stream gets there
int enqueue_diagnostics(nbx_ctx* c, const char* where);
// the raw sums of diag_kernel's field order -> the public struct (kenergy = sum m v^2 / 2, potential = -sum m phi / 2)
void diag_fill(const double* raw, int32_t i_count, int64_t steps_done, nbx_diag_t* out);
}  // namespace nbx_detail
