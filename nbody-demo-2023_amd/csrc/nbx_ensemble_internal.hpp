// nbx_ensemble_internal.hpp -- the ensemble object, shared by the translation units that serve it: nbx_ensemble.hip (create,
// upload, step, download) and nbx_ensemble_diag.hip (diagnostics).  Not part of the C-ABI (include/nbx_ensemble.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/nbx_ensemble.h"
#include "nbx_internal.hpp"  // error plumbing; nbx_plan.hpp: nbx::EnsemblePlan

struct nbx_ensemble {
  int n = 0, members = 0, precision = 32, own_pad = 0;
  nbx::EnsemblePlan plan;
  void (*launch_step)(nbx_ensemble*, double dt) = nullptr;  // plan.step, resolved by nbx_ensemble_create
  int device = 0;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop{};
  size_t rec = 16;         // bytes per {x,y,z,w} record
  size_t pos_stride = 0;   // records between members in posm: n_alloc + kSgprOverread
  void* posm[2] = {nullptr, nullptr};
  int cur = 0;
  void* velm = nullptr;
  double* ke_part = nullptr;  // [members][grid_x]
  bool have_parts = false;    // a step has written ke_part since the last upload
  double* ke_dev = nullptr;   // [ke_cap] reduced sums (sum m v^2), slot s of member m at s * members + m
  size_t ke_cap = 0;
  std::vector<char> uploaded;  // per member
  int uploaded_count = 0;
  long long steps_done = 0;
  bool profiling = false;
  std::vector<hipEvent_t> ev;  // pairs start/stop
  size_t ev_used = 0;
  double step_ms_total = 0.0;
  long long launches_timed = 0;
  // diagnostics (nbx_ensemble_diag.hip): per-workgroup partials [members][parts][9] and the reduced fields [members][9],
  // allocated on first use
  double* diag_part = nullptr;
  double* diag_dev = nullptr;
};
