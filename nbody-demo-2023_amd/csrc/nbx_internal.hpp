// nbx_internal.hpp -- what the translation units of libnbx.so share: the context object, error plumbing, small helpers.
// Not part of the C-ABI (include/nbx.h is); nothing here is visible outside the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/nbx_diag.h"  // includes nbx.h
#include "nbx_plan.hpp"               // ceil_div, round_up, nbx::Plan

namespace nbx_detail {

std::string& last_error();  // thread-local text behind nbx_last_error() (defined in nbx_api.hip)

inline int fail(int code, const std::string& msg) {
  last_error() = msg;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(NBX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

// No C++ exception may cross the C boundary: every entry point that can allocate host memory runs inside this.
template <typename F>
inline int guarded(const char* where, F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    try { return fail(NBX_ERR_ALLOC, std::string(where) + ": out of host memory"); } catch (...) { return NBX_ERR_ALLOC; }
  } catch (const std::exception& e) {
    try { return fail(NBX_ERR_STATE, std::string(where) + ": " + e.what()); } catch (...) { return NBX_ERR_STATE; }
  } catch (...) {
    return NBX_ERR_STATE;
  }
}

}  // namespace nbx_detail

struct nbx_ctx {
  int n = 0, n_alloc = 0, i_begin = 0, i_count = 0, own_pad = 0, precision = 32;
  nbx::Plan plan;  // launch shape and kernel instances (nbx_plan.hpp)
  void (*launch_step)(nbx_ctx*, double dt, int acc_only) = nullptr;  // plan.step and plan.accel, resolved by nbx_create
  void (*launch_accel)(nbx_ctx*, double dt, int acc_only) = nullptr;
  unsigned slice_bit = 0;  // LOOP_ASM_TS: clock bit of the priority slices
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  size_t rec = 16;  // bytes per {x,y,z,w} record
  void* posm[2] = {nullptr, nullptr};
  int cur = 0;
  void* velm = nullptr;
  void* accp = nullptr;
  double* ke_part = nullptr;
  void* mass_all = nullptr;        // NBX_KERNEL_EXACT only: m of every body (the records carry G*m)
  void* posm_pairs = nullptr;      // one body per lane + hand-scheduled loop only: pair-interleaved copy of posm[cur], rebuilt every step
  int ke_parts = 0;       // partials written by the last step
  double* ke_dev = nullptr;  // [ke_cap] reduced sums (sum m v^2)
  int ke_cap = 0;
  bool uploaded = false;
  bool pending_commit = false;
  long long steps_done = 0;
  // profiling
  bool profiling = false;
  std::vector<hipEvent_t> ev;  // pairs start/stop
  size_t ev_used = 0;
  double force_ms_total = 0.0;
  long long force_timed = 0;
  hipDeviceProp_t prop{};
  // hipGraph replay of multi-step windows (launch-bound small n; plan.use_graph)
  struct GraphUnit { int steps; int parity; double dt; hipGraphExec_t exec; };
  std::vector<GraphUnit> graphs;
  long long graph_replays = 0;
  // diagnostics (nbx_diag.hip): per-workgroup partials and the reduced fields, allocated on first use
  double* diag_part = nullptr;
  double* diag_dev = nullptr;
};

namespace nbx_detail {
// shared by the context entry points (nbx_api.hip) and the groups (nbx_group.hip)
int use_device(nbx_ctx* c);
double model_force_cost(const nbx_ctx* c, int own);  // relative cost of one force launch if the context owned `own` bodies (the tuner's predictor)
int enqueue_ke_reduce(nbx_ctx* c, int slot);  // ke_part[0 .. ke_parts) -> ke_dev[slot], fixed order, on the context's stream
constexpr int kDiagFieldCount = 9;  // = nbx::kDiagFields (nbx_diag_kernels.hpp; checked in nbx_diag.hip)
// nbx_diag.hip: checks the context's state, then enqueues the diagnostics kernels on its stream; c->diag_dev then holds the
// kDiagFields raw sums (nbx_diag_kernels.hpp) once the stream gets there
int enqueue_diagnostics(nbx_ctx* c, const char* where);
// the raw sums of diag_kernel's field order -> the public struct (kenergy = sum m v^2 / 2, potential = -sum m phi / 2)
void diag_fill(const double* raw, int32_t i_count, int64_t steps_done, nbx_diag_t* out);
}  // namespace nbx_detail
