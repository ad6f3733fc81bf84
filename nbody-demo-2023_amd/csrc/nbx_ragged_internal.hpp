// nbx_ragged_internal.hpp -- the ragged-ensemble object, shared by the translation units that serve it: nbx_ragged.hip (create,
// upload, step, download) and nbx_ragged_diag.hip (diagnostics).  Not part of the C-ABI (include/nbx_ragged.h is).  It names no
// kernel header, so that each of the two units compiles exactly the kernels it includes itself.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/nbx_ragged.h"
#include "nbx_internal.hpp"  // error plumbing; nbx_plan.hpp: nbx::RaggedPlan, nbx::RaggedDiagPlan

namespace nbx {
struct RaggedParts;  // nbx_ragged_kernels.hpp: the table ragged_ke_reduce_kernel reads
}

struct nbx_ragged {
  int members = 0, precision = 32;
  nbx::RaggedPlan plan;  // per-member offsets (plan.member) and the work list as uploaded (plan.work)
  void (*launch_step)(nbx_ragged*, double dt) = nullptr;  // plan.step, resolved by nbx_ragged_create
  int device = 0;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop{};
  size_t rec = 16;  // bytes per {x,y,z,w} record
  void* posm[2] = {nullptr, nullptr};
  int cur = 0;
  void* velm = nullptr;
  double* ke_part = nullptr;           // [plan.W], a member's partials together
  nbx::RaggedWork* work_dev = nullptr;   // [plan.W]
  nbx::RaggedParts* parts_dev = nullptr; // [members]
  bool have_parts = false;             // a step has written ke_part since the last upload
  double* ke_dev = nullptr;            // [ke_cap] reduced sums (sum m v^2), slot s of member m at s * members + m
  size_t ke_cap = 0;
  std::vector<char> uploaded;          // per member
  int uploaded_count = 0;
  long long steps_done = 0;
  bool profiling = false;
  std::vector<hipEvent_t> ev;          // pairs start/stop
  size_t ev_used = 0;
  double step_ms_total = 0.0;
  long long launches_timed = 0;
  // diagnostics (nbx_ragged_diag.hip), all built or allocated on first use and of a size that is fixed for the object's life:
  // the work list of plan_ragged_diag and its copy on the device, the {row_off, rows} table of the reduce, the per-workgroup
  // partials [diag_plan.total_rows][9] and the reduced fields [members][9]
  nbx::RaggedDiagPlan diag_plan;
  bool have_diag_plan = false;
  nbx::RaggedDiagWork* diag_work_dev = nullptr;
  nbx::RaggedDiagRows* diag_rows_dev = nullptr;
  double* diag_part = nullptr;
  double* diag_dev = nullptr;
};
