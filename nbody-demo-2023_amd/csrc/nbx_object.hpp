// nbx_object.hpp -- what the three kinds of device object -- the context (nbx_internal.hpp), the ensemble and the ragged ensemble
// (nbx_batch.hpp) -- have in common on the host: error plumbing, the fields every object has, device choice, the energy trace
// and its read-back, profiling and the event bracket around a launch, and the shared part of create and destroy.  Host-only: it
// defines no kernel and includes no kernel header, so every translation unit keeps compiling exactly the kernels it includes
// itself.  Not part of the C-ABI.
//
// A kind is a struct derived from Object that adds   static constexpr BatchNames names;   the words its error texts are made of.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/nbx.h"

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

// Nothing below is visible outside the library: libnbx.so exports what the public headers declare.
#pragma GCC visibility push(hidden)
namespace nbx_detail {

struct BatchNames {
  const char* prefix;  // "nbx_ensemble": the upload hint and the energy-trace text
  const char* noun;    // "ensemble", as in "ensemble is NULL"
};

struct Object {
  int precision = 32;
  int device = 0;
  hipStream_t stream = nullptr;  // a context may work on one the caller lent it (NULL = the default stream)
  bool own_stream = false;       // made by batch_open, destroyed by batch_release
  hipDeviceProp_t prop{};
  size_t rec = 16;  // bytes per {x,y,z,w} record
  void* posm[2] = {nullptr, nullptr};
  int cur = 0;
  void* velm = nullptr;
  double* ke_part = nullptr;  // the step's energy partials
  double* ke_dev = nullptr;   // [ke_cap] reduced sums (sum m v^2): S per step (S = the members of a batch, 1 for a context)
  size_t ke_cap = 0;
  long long steps_done = 0;
  bool profiling = false;
  std::vector<hipEvent_t> ev;  // pairs start/stop
  size_t ev_used = 0;
  double ms_total = 0.0;  // of the launches_timed launches whose events have been drained
  long long launches_timed = 0;
  // diagnostics (nbx_*diag.hip): per-workgroup partials and the reduced fields, allocated on first use
  double* diag_part = nullptr;
  double* diag_dev = nullptr;
  // time scales (nbx_timescale.hip): per-workgroup rows of 3 and the reduced values per system, allocated on first use
  double* ts_part = nullptr;
  double* ts_dev = nullptr;
  // field at caller-supplied points (nbx_field.hip): the packed points, the partial rows and the result records, allocated on
  // first use and grown -- never shrunk -- when a larger call arrives (sizes in bytes); field_tab: a ragged ensemble's
  // {pos_off, n} per member, built on first use and fixed for the object's life
  void* field_pts = nullptr;
  void* field_part = nullptr;
  void* field_out = nullptr;
  void* field_tab = nullptr;
  size_t field_pts_cap = 0, field_part_cap = 0, field_out_cap = 0;
  // nearest neighbours and radius counts (nbx_neighbours.hip): the partial records and the result records, allocated on first
  // use and grown likewise (sizes in bytes); nb_tab: a ragged ensemble's {pos_off, out_off, n} per member, built on first use
  void* nb_part = nullptr;
  void* nb_out = nullptr;
  void* nb_tab = nullptr;
  size_t nb_part_cap = 0, nb_out_cap = 0;
  // pair counts within a list of radii (nbx_paircount.hip): the workgroup records and the results, allocated on first use and
  // grown likewise (sizes in bytes); pc_tab: a ragged ensemble's {pos_off, n} per member, built on first use
  void* pc_part = nullptr;
  void* pc_out = nullptr;
  void* pc_tab = nullptr;
  size_t pc_part_cap = 0, pc_out_cap = 0;
  // k nearest neighbours (nbx_knn.hip): the partial rows and the result rows, allocated on first use and grown likewise (sizes
  // in bytes); knn_tab: a ragged ensemble's {pos_off, out_off, n} per member, built on first use
  void* knn_part = nullptr;
  void* knn_out = nullptr;
  void* knn_tab = nullptr;
  size_t knn_part_cap = 0, knn_out_cap = 0;
  // friends-of-friends groups (nbx_fof.hip): the staged {x, y, z, label} records, the split rows of a pass, the work arrays
  // (labels, their successors, where a body's record is, the histogram, the changed words) and the results, allocated on first
  // use and grown likewise (sizes in bytes); fof_tab: a ragged ensemble's {pos_off, out_off, rec_off, n} per member, built on
  // first use
  void* fof_rec = nullptr;
  void* fof_part = nullptr;
  void* fof_work = nullptr;
  void* fof_out = nullptr;
  void* fof_tab = nullptr;
  size_t fof_rec_cap = 0, fof_part_cap = 0, fof_work_cap = 0, fof_out_cap = 0;
  // most bound partners and bound counts (nbx_binaries.hip): the partial records and the result records, allocated on first
  // use and grown likewise (sizes in bytes); bin_tab: a ragged ensemble's {pos_off, vel_off, out_off, n} per member, built on
  // first use
  void* bin_part = nullptr;
  void* bin_out = nullptr;
  void* bin_tab = nullptr;
  size_t bin_part_cap = 0, bin_out_cap = 0;
  // tidal tensors at caller-supplied points and at the bodies (nbx_tidal.hip): the packed points, the partial rows (two records
  // per point and split) and the result records (two per point), allocated on first use and grown likewise (sizes in bytes);
  // tidal_tab: a ragged ensemble's {pos_off, out_off, n} per member, built on first use
  void* tidal_pts = nullptr;
  void* tidal_part = nullptr;
  void* tidal_out = nullptr;
  void* tidal_tab = nullptr;
  size_t tidal_pts_cap = 0, tidal_part_cap = 0, tidal_out_cap = 0;
  // clumps under a caller-supplied label (nbx_clumps.hip): the uploaded labels, the partial records followed by the count rows
  // and the result records followed by the members, allocated on first use and grown likewise (sizes in bytes); clump_tab: a
  // ragged ensemble's {pos_off, vel_off, out_off, n} per member, built on first use
  void* clump_lab = nullptr;
  void* clump_part = nullptr;
  void* clump_out = nullptr;
  void* clump_tab = nullptr;
  size_t clump_lab_cap = 0, clump_part_cap = 0, clump_out_cap = 0;
  // neighbour lists (nbx_nlist.hip): the (split, body) segments, the scan's arrays (within, offsets, block sums) and the two
  // lists, the lists sized by a call's total and never by the caller's capacity, allocated on first use and grown likewise
  // (sizes in bytes); nl_tab: a ragged ensemble's {pos_off, out_off, n} per member, built on first use
  void* nl_seg = nullptr;
  void* nl_scan = nullptr;
  void* nl_index = nullptr;
  void* nl_r2 = nullptr;
  void* nl_tab = nullptr;
  size_t nl_seg_cap = 0, nl_scan_cap = 0, nl_index_cap = 0, nl_r2_cap = 0;
  // accelerations and their time derivatives (nbx_jerk.hip): the partial rows (two records per body and split) and the result
  // records (two per body), allocated on first use and grown likewise (sizes in bytes); jerk_tab: a ragged ensemble's
  // {pos_off, vel_off, out_off, n} per member, built on first use
  void* jerk_part = nullptr;
  void* jerk_out = nullptr;
  void* jerk_tab = nullptr;
  size_t jerk_part_cap = 0, jerk_out_cap = 0;
  // resident Hermite stepper (nbx_hermite.hip): the partial rows (two records per body and split) and the kept {a, 0}, {j, 0}
  // records (two per velocity record), allocated on first use and of a size that is fixed for the object's life; herm_tab: a
  // ragged ensemble's {pos_off, vel_off, out_off, n} per member, built on first use, herm_tab_src the host bytes its copy reads
  // (no call of the stepper synchronises, so they live with the object); herm_have: a call has left kept records, made when
  // steps_done was herm_steps and the current position buffer herm_cur -- what `resume` is checked against
  void* herm_part = nullptr;
  void* herm_keep = nullptr;
  void* herm_tab = nullptr;
  std::vector<char> herm_tab_src;
  bool herm_have = false;
  long long herm_steps = 0;
  int herm_cur = 0;
  // adaptive power-of-two steps (nbx_advance.hip): it works in herm_part, herm_keep and herm_tab (the same sizes and layout) and
  // adds the candidates, one double per body, and the clock records, one per system, allocated on first use and of a size that
  // is fixed for the object's life; adv_have: an advance call has left clocks and kept records, made when steps_done was
  // adv_steps and the current position buffer adv_cur, with these dt_cap and levels -- what its `resume` is checked against --
  // and this t_end, which the clock calls report `done` against
  void* adv_cand = nullptr;
  void* adv_clock = nullptr;
  bool adv_have = false;
  long long adv_steps = 0;
  int adv_cur = 0;
  int adv_levels = 0;
  double adv_dt_cap = 0.0;
  double adv_t_end = 0.0;
  // resident tracers (nbx_tracers.hip): tr_m per system (0: none), every system's {x, y, z, 0} position and velocity records
  // one system after the other, and the partial rows of the pair work ([systems][tr_rows][tr_m] records, buffers of their own:
  // not the field's scratch), allocated by the first upload and grown likewise (sizes in bytes); tr_have: per system, its
  // tracers have been uploaded; tr_tab: a ragged ensemble's {pos_off, n} per member, built by the first upload
  void* tr_pos = nullptr;
  void* tr_vel = nullptr;
  void* tr_part = nullptr;
  void* tr_tab = nullptr;
  size_t tr_pos_cap = 0, tr_vel_cap = 0, tr_part_cap = 0;
  int tr_m = 0, tr_rows = 1;
  std::vector<char> tr_have;
};

constexpr int kMaxProfiledLaunches = 8192;

// ---------------------------------------------------------------------------------------------------------------------------
// device selection, buffers allocated after create, energy trace
// ---------------------------------------------------------------------------------------------------------------------------
inline int use_device(Object* o) {
  HIP_TRY(hipSetDevice(o->device));
  return NBX_OK;
}

// `where` is the entry point the text names
template <typename P>
int device_alloc(P** p, size_t count, const char* where, const char* what) {
  const hipError_t err = hipMalloc(p, sizeof(P) * count);
  if (err == hipSuccess) return NBX_OK;
  *p = nullptr;
  return fail(err == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE,
              std::string(where) + ": hipMalloc of " + what + ": " + hipGetErrorString(err));
}

inline int ensure_ke_cap(Object* o, const char* where, size_t need) {
  if (need <= o->ke_cap) return NBX_OK;
  if (o->ke_dev) HIP_TRY(hipFree(o->ke_dev));
  o->ke_dev = nullptr;
  o->ke_cap = 0;
  const int rc = device_alloc(&o->ke_dev, need, where, "the energy trace");
  if (rc == NBX_OK) o->ke_cap = need;
  return rc;
}

// The end of a *_step (ke_trace == nullptr) or *_step_trace (ke_last == nullptr): S reduced sums per step from ke_dev to the
// caller as energies.  A step call of no steps reads the partials the last step since an upload left behind -- `reduce()` puts
// their sums into slot 0 -- and gives 0 where there are none (`have_parts`).
template <typename Reduce>
int read_energies(Object* o, size_t S, int nsteps, bool have_parts, double* ke_last, double* ke_trace, Reduce reduce) {
  double* out = ke_last;
  size_t count = S;
  if (ke_trace && nsteps > 0) {
    out = ke_trace;
    count = S * (size_t)nsteps;
  } else if (ke_last && nsteps == 0) {
    if (!have_parts) {
      for (size_t m = 0; m < S; ++m) ke_last[m] = 0.0;
      return NBX_OK;
    }
    const int rc = reduce();
    if (rc) return rc;
  }
  if (!out) return NBX_OK;
  HIP_TRY(hipMemcpyAsync(out, o->ke_dev, sizeof(double) * count, hipMemcpyDeviceToHost, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  for (size_t k = 0; k < count; ++k) out[k] *= 0.5;  // ver7/GSimulation.cpp:200
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------------------------------------
// `launch()` between a pair of events while the object is profiling and has events left (timed: this launch is one to time)
template <typename Launch>
int timed_launch(Object* o, bool timed, Launch launch) {
  const bool prof = timed && o->profiling && o->ev_used + 2 <= o->ev.size();
  if (prof) HIP_TRY(hipEventRecord(o->ev[o->ev_used], o->stream));
  launch();
  if (prof) {
    HIP_TRY(hipEventRecord(o->ev[o->ev_used + 1], o->stream));
    o->ev_used += 2;
  }
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

inline int drain_profile(Object* o) {
  for (size_t k = 0; k + 1 < o->ev_used; k += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, o->ev[k], o->ev[k + 1]));
    o->ms_total += ms;
    o->launches_timed += 1;
  }
  o->ev_used = 0;
  return NBX_OK;
}

template <typename O>
int batch_sync(O* o, const char* where) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = use_device(o);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(o->stream));
  return NBX_OK;
  });
}

template <typename O>
int batch_profile(O* o, const char* where, int32_t enable) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = use_device(o);
  if (rc) return rc;
  if (enable && o->ev.empty()) {
    o->ev.assign(2 * kMaxProfiledLaunches, nullptr);
    for (auto& ev : o->ev) HIP_TRY(hipEventCreate(&ev));
  }
  if (!enable && o->profiling) {
    HIP_TRY(hipStreamSynchronize(o->stream));
    rc = drain_profile(o);
    if (rc) return rc;
  }
  if (enable && !o->profiling) {
    o->ms_total = 0.0;
    o->launches_timed = 0;
    o->ev_used = 0;
  }
  o->profiling = enable != 0;
  return NBX_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// create and destroy.  A *_create is: create_opts, the kind's argument checks and planning (all before the first HIP call),
// batch_open, planning with the CU count, the kind's own buffers under CREATE_TRY, owner.release().
// ---------------------------------------------------------------------------------------------------------------------------
#define CREATE_TRY(where, expr)                                                              \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      std::string m_ = std::string(where) + ": " #expr ": " + hipGetErrorString(e_);         \
      return fail(e_ == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE, m_);           \
    }                                                                                        \
  } while (0)

// frees the object on every failure path of *_create
template <typename O>
struct BatchOwner {
  void (*destroy)(O*);
  O* o = nullptr;
  ~BatchOwner() { if (o) destroy(o); }
  O* release() { O* p = o; o = nullptr; return p; }
};

// *out cleared, the caller's options or the defaults -> *o
template <typename O>
int create_opts(const char* where, O** out, const nbx_opts* opts, nbx_opts* o) {
  if (!out) return fail(NBX_ERR_ARG, std::string(where) + ": out is NULL");
  *out = nullptr;
  std::memset(o, 0, sizeof(*o));
  o->device = -1;
  if (opts) {
    if (opts->struct_size != 0 && opts->struct_size != (int32_t)sizeof(nbx_opts))
      return fail(NBX_ERR_ARG, std::string(where) + ": nbx_opts.struct_size does not match this library");
    *o = *opts;
  }
  return NBX_OK;
}

// the device, the object (owned by *owner from here on) and its stream -- the caller's if o.external_stream says so (only the
// context's planning lets that through), else one of its own; prop.multiProcessorCount is known afterwards
template <typename O>
int batch_open(const char* where, const nbx_opts& o, int precision, BatchOwner<O>* owner) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(NBX_ERR_DEVICE, std::string(where) + ": no HIP device available (libnbx has no CPU path)");
  int dev = o.device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return fail(NBX_ERR_DEVICE, std::string(where) + ": hipGetDevice failed");
  }
  if (dev >= ndev) return fail(NBX_ERR_ARG, std::string(where) + ": device ordinal out of range");

  O* b = new (std::nothrow) O();
  if (!b) return fail(NBX_ERR_ALLOC, std::string(where) + ": out of host memory");
  owner->o = b;
  b->device = dev;
  b->precision = precision;
  b->rec = precision == 32 ? sizeof(float4) : sizeof(double4);
  CREATE_TRY(where, hipSetDevice(dev));
  CREATE_TRY(where, hipGetDeviceProperties(&b->prop, dev));
  if (o.external_stream) {
    b->stream = (hipStream_t)o.stream;  // may be NULL: the default stream
  } else {
    CREATE_TRY(where, hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    b->own_stream = true;
  }
  return NBX_OK;
}

// A *_destroy is: batch_quiesce, free what the kind owns, batch_release, delete.  The stream is synchronised first -- also a
// lent one, NULL (the caller's default stream) included -- and, where the object made it, destroyed last.
inline void batch_quiesce(Object* o) {
  (void)hipSetDevice(o->device);
  (void)hipStreamSynchronize(o->stream);
}

inline void batch_release(Object* o) {
  for (hipEvent_t ev : o->ev)
    if (ev) (void)hipEventDestroy(ev);
  for (void* p : {o->posm[0], o->posm[1], o->velm, (void*)o->ke_part, (void*)o->ke_dev, (void*)o->diag_part, (void*)o->diag_dev, (void*)o->ts_part,
                  (void*)o->ts_dev, o->field_pts, o->field_part, o->field_out, o->field_tab, o->nb_part, o->nb_out, o->nb_tab, o->pc_part,
                  o->pc_out, o->pc_tab, o->knn_part, o->knn_out, o->knn_tab, o->fof_rec, o->fof_part,
                  o->fof_work, o->fof_out, o->fof_tab, o->bin_part, o->bin_out, o->bin_tab, o->tidal_pts, o->tidal_part,
                  o->tidal_out, o->tidal_tab, o->clump_lab, o->clump_part, o->clump_out, o->clump_tab, o->nl_seg, o->nl_scan, o->nl_index,
                  o->nl_r2, o->nl_tab, o->jerk_part, o->jerk_out, o->jerk_tab, o->herm_part, o->herm_keep, o->herm_tab, o->adv_cand, o->adv_clock, o->tr_pos, o->tr_vel, o->tr_part, o->tr_tab})
    if (p) (void)hipFree(p);
  if (o->own_stream) (void)hipStreamDestroy(o->stream);
}

}  // namespace nbx_detail
#pragma GCC visibility pop
