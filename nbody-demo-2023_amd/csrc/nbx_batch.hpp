// nbx_batch.hpp -- the host side that ensembles (nbx_ensemble.hip, nbx_ensemble_diag.hip) and ragged ensembles (nbx_ragged.hip,
// nbx_ragged_diag.hip) share on top of what every device object has (nbx_object.hpp: the fields, device choice, the energy
// trace, profiling, create / destroy -- the context, nbx_internal.hpp, stands on that base too): the member bookkeeping and
// checks, the step loop, the launcher tables, upload and download over a member-layout lookup, stats, and the diagnostics,
// accelerations and kick entry points.  Host-only: it defines no kernel and includes no kernel header, so every translation unit keeps compiling exactly the
// kernels it includes itself.
//
// A kind is a struct derived from Batch (nbx_ensemble, nbx_ragged) that adds
//   static constexpr BatchNames names;           the words its error texts are made of
//   MemberSpan layout(int k) const;              where member k lies on the device
//   void (*launch_step)(Kind*, double dt);       one time step of all members, resolved at create from kLaunchers
// and whose internal header declares the overload  int nbx_detail::enqueue_ke_reduce(Kind*, int slot)  (the step loop below
// finds it by argument-dependent lookup); the kind's main translation unit defines it: it launches that unit's own reduce kernel.
// The context's step path (nbx_api.hip) is tied to graph replay and the exchange protocol and is not served from here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "nbx_internal.hpp"  // nbx_object.hpp: Object, error plumbing; diag_fill; nbx_plan.hpp: kEnsembleInstances, kSgprOverread
#include "nbx_pair.hpp"      // the record types and the constants a record carries (inline code only, no kernel)

// Nothing of this layer is visible outside the library: libnbx.so exports what the public headers declare, as before.
#pragma GCC visibility push(hidden)
namespace nbx_detail {

// Member k on the device: its first record in posm / velm, its bodies, and its records (n rounded up to the tile; kSgprOverread
// spare records follow them in posm).
struct MemberSpan {
  size_t pos_off, vel_off;
  int n, n_alloc;
};

struct Batch : Object {
  int members = 0;
  bool have_parts = false;     // a step has written ke_part (a member's partials together) since the last upload
  std::vector<char> uploaded;  // per member
  int uploaded_count = 0;
  // ke_dev: slot s of member m at s * members + m; diag_part is [rows][9], diag_dev [members][9]
  void* accm = nullptr;  // *_accel (nbx_batch_accel.hip): {ax, ay, az, 0} records laid out as velm, allocated on first use; the kind's destroy frees it
};

// *_stats up to the fields of the kind: the checks, the pending events drained, *s cleared and the fields every kind reports
// filled in; `fill(s)` adds the rest.  S is the kind's public stats struct, named where + "_t".
template <typename O, typename S, typename Fill>
int batch_stats(O* o, S* s, const char* where, Fill fill) {
  return guarded(where, [&]() -> int {
  if (!o || !s) return fail(NBX_ERR_ARG, std::string(where) + ": NULL argument");
  if (s->struct_size != 0 && s->struct_size != (int32_t)sizeof(S))
    return fail(NBX_ERR_ARG, std::string(where) + ": " + where + "_t.struct_size does not match this library");
  int rc = use_device(o);
  if (rc) return rc;
  if (o->ev_used) {
    HIP_TRY(hipStreamSynchronize(o->stream));
    rc = drain_profile(o);
    if (rc) return rc;
  }
  std::memset(s, 0, sizeof(*s));
  s->struct_size = (int32_t)sizeof(S);
  s->members = o->members; s->precision = o->precision; s->block = nbx::kBlock; s->cu_count = o->prop.multiProcessorCount;
  s->steps_done = o->steps_done; s->launches_timed = o->launches_timed; s->step_ms_total = o->ms_total;
  fill(s);
  return NBX_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// member checks
// ---------------------------------------------------------------------------------------------------------------------------
inline int check_range(const Batch* b, const char* where, int first, int count) {
  if (first < 0 || count < 0 || (long long)first + count > b->members)
    return fail(NBX_ERR_ARG, std::string(where) + ": members [first, first + count) are outside [0, members)");
  return NBX_OK;
}

inline int check_uploaded(const Batch* b, const char* where, int first, int count) {
  for (int k = first; k < first + count; ++k)
    if (!b->uploaded[k]) return fail(NBX_ERR_STATE, std::string(where) + ": member " + std::to_string(k) + " has not been uploaded");
  return NBX_OK;
}

inline void mark_uploaded(Batch* b, int first, int count) {
  for (int k = first; k < first + count; ++k)
    if (!b->uploaded[k]) { b->uploaded[k] = 1; b->uploaded_count += 1; }
  b->have_parts = false;  // the partials on the device belong to the previous trajectories
}

// ---------------------------------------------------------------------------------------------------------------------------
// device tables made after create (the diagnostics'); `where` is the entry point the text names
// ---------------------------------------------------------------------------------------------------------------------------
// a host table (which lives as long as the object) -> a device copy, on the stream the launches follow on; *p is set only once
// the copy has been enqueued
template <typename P>
int device_table(Batch* b, P** p, const std::vector<P>& src, const char* where, const char* what) {
  P* dev = nullptr;
  const int rc = device_alloc(&dev, src.size(), where, what);
  if (rc) return rc;
  const hipError_t err = hipMemcpyAsync(dev, src.data(), sizeof(P) * src.size(), hipMemcpyHostToDevice, b->stream);
  if (err != hipSuccess) {
    (void)hipFree(dev);
    return fail(NBX_ERR_DEVICE, std::string(where) + ": copy of " + what + ": " + hipGetErrorString(err));
  }
  *p = dev;
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the step loop: one launch per step through o->launch_step, no allocation and no indirect call besides it
// ---------------------------------------------------------------------------------------------------------------------------
template <typename O>
int enqueue_step(O* o, double dt) {
  const int rc = timed_launch(o, true, [&] { o->launch_step(o, dt); });
  if (rc == NBX_OK) o->have_parts = true;
  return rc;
}

// *_step (ke_trace == nullptr) and, behind step_trace below, *_step_trace (ke_last == nullptr)
template <typename O>
int step_common(O* o, const char* where, double dt, int32_t nsteps, double* ke_last, double* ke_trace) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (nsteps < 0) return fail(NBX_ERR_ARG, std::string(where) + ": nsteps < 0");
  if (!std::isfinite(dt)) return fail(NBX_ERR_ARG, std::string(where) + ": dt is not finite");
  if (o->uploaded_count != o->members)
    return fail(NBX_ERR_STATE, std::string(where) + ": " + std::to_string(o->members - o->uploaded_count) + " of " + std::to_string(o->members) +
                                   " members have not been uploaded (" + O::names.prefix + "_upload)");
  int rc = use_device(o);
  if (rc) return rc;
  const size_t S = (size_t)o->members;
  if (ke_trace || ke_last) {
    rc = ensure_ke_cap(o, O::names.prefix, S * (size_t)(ke_trace ? std::max(nsteps, 1) : 1));
    if (rc) return rc;
  }
  for (int s = 0; s < nsteps; ++s) {
    rc = enqueue_step(o, dt);
    if (rc) return rc;
    o->cur ^= 1;
    o->steps_done += 1;
    if (ke_trace) rc = enqueue_ke_reduce(o, s);
    else if (ke_last && s == nsteps - 1) rc = enqueue_ke_reduce(o, 0);
    if (rc) return rc;
  }
  return read_energies(o, S, nsteps, o->have_parts, ke_last, ke_trace, [&] { return enqueue_ke_reduce(o, 0); });
  });
}

// a NULL ke_trace is reported before the handle is looked at
template <typename O>
int step_trace(O* o, const char* where, double dt, int32_t nsteps, double* ke_trace) {
  if (!ke_trace) return guarded(where, [&]() -> int { return fail(NBX_ERR_ARG, std::string(where) + ": ke_trace is NULL"); });
  return step_common(o, where, dt, nsteps, nullptr, ke_trace);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the launcher table: one launcher per entry of kEnsembleInstances -- the shapes a jlane context can run, and the only step-kernel
// instances a kind's translation unit compiles.  Launch::run<I>(o, dt) launches the kind's kernel for entry I.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename O, typename Launch, int I>
void launch_instance(O* o, double dt) {
  static_assert(nbx::kEnsembleInstances[I].kind == nbx::INST_JLANE, "a member steps with the one-launch kernel body");
  Launch::template run<I>(o, dt);
}
template <typename O, typename Launch, int... I>
constexpr std::array<void (*)(O*, double), sizeof...(I)> make_launchers(std::integer_sequence<int, I...>) {
  return {{&launch_instance<O, Launch, I>...}};
}
template <typename O, typename Launch>
constexpr auto kLaunchers = make_launchers<O, Launch>(std::make_integer_sequence<int, nbx::kEnsembleInstanceCount>{});

// ---------------------------------------------------------------------------------------------------------------------------
// *_kick (include/nbx_kick.h): v += a(x) * h for every body of every member -- ONE launch over the step's own grid through a
// third launcher table, one launcher per entry of kEnsembleInstances: Launch::run<I>(o, h) launches the kind's kick kernel
// (nbx_kick_kernels.hpp, instantiated by nbx_kick.hip alone) for entry I.  Beside step_common because it ends as a step does:
// the launch leaves ke_part describing the kicked velocities (have_parts), and an energy asked for takes the step's reduce and
// read-back.  It is not a step otherwise: cur, steps_done and the profile of the step kernel do not see it (the launch is not
// timed).  Every check comes before the first HIP call.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename O, typename Launch, int I>
void launch_kick_instance(O* o, double h) {
  static_assert(nbx::kEnsembleInstances[I].kind == nbx::INST_JLANE, "a member is kicked by the one-launch kernel body");
  Launch::template run<I>(o, h);
}
template <typename O, typename Launch, int... I>
constexpr std::array<void (*)(O*, double), sizeof...(I)> make_kick_launchers(std::integer_sequence<int, I...>) {
  return {{&launch_kick_instance<O, Launch, I>...}};
}
template <typename O, typename Launch>
constexpr auto kKickLaunchers = make_kick_launchers<O, Launch>(std::make_integer_sequence<int, nbx::kEnsembleInstanceCount>{});

template <typename O, typename Launch>
int kick_common(O* o, const char* where, double h, double* ke_out) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!std::isfinite(h)) return fail(NBX_ERR_ARG, std::string(where) + ": h is not finite");
  int rc = check_uploaded(o, where, 0, o->members);
  if (rc) return rc;
  const int k = nbx::ensemble_instance_index(o->plan.step);  // *_create has resolved the step's launcher from the same index
  if (k < 0) return fail(NBX_ERR_STATE, std::string(where) + ": no kernel instance for this bodies_per_lane / precision");
  rc = use_device(o);
  if (rc) return rc;
  const size_t S = (size_t)o->members;
  if (ke_out) {
    rc = ensure_ke_cap(o, where, S);
    if (rc) return rc;
  }
  kKickLaunchers<O, Launch>[(size_t)k](o, h);
  HIP_TRY(hipGetLastError());
  o->have_parts = true;  // of the kicked velocities: what a following step call of no steps reports
  if (ke_out) {
    rc = enqueue_ke_reduce(o, 0);
    if (rc) return rc;
  }
  return read_energies(o, S, 1, true, ke_out, nullptr, [] { return (int)NBX_OK; });  // without ke_out: no copy, no synchronisation
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// upload and download
// ---------------------------------------------------------------------------------------------------------------------------
// Members [first, first + count) lie one behind the other on the device: records [pos_begin, pos_begin + pos_count) of posm,
// [vel_begin, vel_begin + vel_count) of velm.  For an ensemble (member k at k * pos_stride and k * own_pad, pos_stride =
// n_alloc + kSgprOverread, own_pad = n_alloc) the counts are (count - 1) * stride + the last member's = count * pos_stride and
// count * own_pad.
struct Span { size_t pos_begin, pos_count, vel_begin, vel_count; };
template <typename O>
Span span_of(const O* o, int first, int count) {
  const MemberSpan a = o->layout(first), b = o->layout(first + count - 1);
  return {a.pos_off, b.pos_off + b.n_alloc + nbx::kSgprOverread - a.pos_off, a.vel_off, b.vel_off + b.n_alloc - a.vel_off};
}

// The host arrays hold the members one after the other, member `first` at element 0.
template <typename T, typename O>
int upload_t(O* o, int first, int count, const T* px, const T* py, const T* pz, const T* vx, const T* vy, const T* vz, const T* m) {
  using T4 = typename nbx::V4<T>::type;
  // the members' records as they lie on the device, padding and spare records included (zero): one copy per buffer
  const Span sp = span_of(o, first, count);
  T4 zero; zero.x = zero.y = zero.z = zero.w = (T)0;
  std::vector<T4> hp(sp.pos_count, zero), hv(sp.vel_count, zero);
  const T G = nbx::grav_const<T>();
  size_t h = 0;  // the member's first element in the host arrays
  for (int k = first; k < first + count; ++k) {
    const MemberSpan mem = o->layout(k);
    T4* p = hp.data() + (mem.pos_off - sp.pos_begin);
    T4* v = hv.data() + (mem.vel_off - sp.vel_begin);
    for (int i = 0; i < mem.n; ++i) {
      T4 q; q.x = px[h + i]; q.y = py[h + i]; q.z = pz[h + i]; q.w = (G * m[h + i]) * nbx::gm_prescale<T>();
      p[i] = q;
      T4 u; u.x = vx[h + i]; u.y = vy[h + i]; u.z = vz[h + i]; u.w = m[h + i];
      v[i] = u;
    }
    h += (size_t)mem.n;
  }
  const size_t pos_off = sizeof(T4) * sp.pos_begin, vel_off = sizeof(T4) * sp.vel_begin;
  HIP_TRY(hipMemcpyAsync((char*)o->posm[0] + pos_off, hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, o->stream));
  HIP_TRY(hipMemcpyAsync((char*)o->posm[1] + pos_off, hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, o->stream));
  HIP_TRY(hipMemcpyAsync((char*)o->velm + vel_off, hv.data(), sizeof(T4) * hv.size(), hipMemcpyHostToDevice, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  return NBX_OK;
}

// one buffer's records of members [first, first + count) -> up to three host arrays (a NULL one is skipped)
template <typename T, typename O>
int download_records(O* o, int first, int count, const void* dev, bool is_pos, T* x, T* y, T* z) {
  using T4 = typename nbx::V4<T>::type;
  if (!x && !y && !z) return NBX_OK;
  const Span sp = span_of(o, first, count);
  const size_t begin = is_pos ? sp.pos_begin : sp.vel_begin;
  std::vector<T4> hr(is_pos ? sp.pos_count : sp.vel_count);
  HIP_TRY(hipMemcpyAsync(hr.data(), (const char*)dev + sizeof(T4) * begin, sizeof(T4) * hr.size(), hipMemcpyDeviceToHost, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  size_t h = 0;
  for (int k = first; k < first + count; ++k) {
    const MemberSpan mem = o->layout(k);
    const T4* r = hr.data() + ((is_pos ? mem.pos_off : mem.vel_off) - begin);
    for (int i = 0; i < mem.n; ++i) {
      if (x) x[h + i] = r[i].x;
      if (y) y[h + i] = r[i].y;
      if (z) z[h + i] = r[i].z;
    }
    h += (size_t)mem.n;
  }
  return NBX_OK;
}

template <typename T, typename O>
int download_t(O* o, int first, int count, T* px, T* py, T* pz, T* vx, T* vy, T* vz) {
  const int rc = download_records(o, first, count, o->posm[o->cur], true, px, py, pz);
  return rc ? rc : download_records(o, first, count, o->velm, false, vx, vy, vz);
}

template <typename O>
int batch_upload(O* o, const char* where, int32_t first, int32_t count, const void* px, const void* py, const void* pz,
                 const void* vx, const void* vy, const void* vz, const void* m) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (!px || !py || !pz || !vx || !vy || !vz || !m) return fail(NBX_ERR_ARG, std::string(where) + ": NULL array");
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  rc = o->precision == 32
           ? upload_t<float>(o, first, count, (const float*)px, (const float*)py, (const float*)pz, (const float*)vx, (const float*)vy,
                             (const float*)vz, (const float*)m)
           : upload_t<double>(o, first, count, (const double*)px, (const double*)py, (const double*)pz, (const double*)vx,
                              (const double*)vy, (const double*)vz, (const double*)m);
  if (rc) return rc;
  mark_uploaded(o, first, count);
  return NBX_OK;
  });
}

template <typename O>
int batch_download(O* o, const char* where, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32
             ? download_t<float>(o, first, count, (float*)px, (float*)py, (float*)pz, (float*)vx, (float*)vy, (float*)vz)
             : download_t<double>(o, first, count, (double*)px, (double*)py, (double*)pz, (double*)vx, (double*)vy, (double*)vz);
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// create (after batch_open of nbx_object.hpp)
// ---------------------------------------------------------------------------------------------------------------------------
inline void set_members(Batch* b, int members) {
  b->members = members;
  b->uploaded.assign((size_t)members, 0);
}

// plan.step -> o->launch_step
template <typename O, typename Launch>
int resolve_launcher(O* o, const char* where) {
  const int k = nbx::ensemble_instance_index(o->plan.step);
  if (k < 0) return fail(NBX_ERR_ARG, std::string(where) + ": no kernel instance for this bodies_per_lane / precision");
  o->launch_step = kLaunchers<O, Launch>[k];
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// *_diagnostics: `enqueue(T{}, o, first, count)`, T the precision's type, enqueues the kind's kernels on o->stream; they leave
// Fields raw sums per member in o->diag_dev[k * Fields ...], k = 0 .. count - 1
// ---------------------------------------------------------------------------------------------------------------------------
template <int Fields, typename O, typename Enqueue>
int batch_diagnostics(O* o, const char* where, int32_t first, int32_t count, nbx_diag_t* out, Enqueue enqueue) {
  static_assert(Fields == kDiagFieldCount, "diag_fill reads kDiagFieldCount raw sums per member");
  return guarded(where, [&]() -> int {
  if (!o || !out) return fail(NBX_ERR_ARG, std::string(where) + ": NULL argument");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  for (int k = 0; k < count; ++k)
    if (out[k].struct_size != 0 && out[k].struct_size != (int32_t)sizeof(nbx_diag_t))
      return fail(NBX_ERR_ARG, std::string(where) + ": out[" + std::to_string(k) + "].struct_size does not match this library");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  rc = o->precision == 32 ? enqueue(float{}, o, first, count) : enqueue(double{}, o, first, count);
  if (rc) return rc;
  std::vector<double> raw((size_t)count * Fields);
  HIP_TRY(hipMemcpyAsync(raw.data(), o->diag_dev, sizeof(double) * raw.size(), hipMemcpyDeviceToHost, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  for (int k = 0; k < count; ++k) diag_fill(raw.data() + (size_t)k * Fields, o->layout(first + k).n, o->steps_done, out + k);
  return NBX_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------------
// *_accel (include/nbx_batch_accel.h): the accelerations of members [first, first + count) at posm[cur] -- one launch over the
// workgroups of those members, one copy of the range's span of the slab, one synchronisation.  The launcher table is the step's
// over again: one launcher per entry of kEnsembleInstances, Launch::run<I>(o, first, count) launches the kind's accel kernel
// for entry I.  `prepare(o)` is the kind's part of the first use (a ragged ensemble's work list).  The launch is not a step: it
// is not timed, and have_parts, steps_done and cur do not see it.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename O, typename Launch, int I>
void launch_accel_instance(O* o, int first, int count) {
  static_assert(nbx::kEnsembleInstances[I].kind == nbx::INST_JLANE, "a member's accelerations come from the one-launch kernel body");
  Launch::template run<I>(o, first, count);
}
template <typename O, typename Launch, int... I>
constexpr std::array<void (*)(O*, int, int), sizeof...(I)> make_accel_launchers(std::integer_sequence<int, I...>) {
  return {{&launch_accel_instance<O, Launch, I>...}};
}
template <typename O, typename Launch>
constexpr auto kAccelLaunchers = make_accel_launchers<O, Launch>(std::make_integer_sequence<int, nbx::kEnsembleInstanceCount>{});

// first use: the slab, member k's n_alloc_k records at its vel_off -- the size and layout of velm, fixed for the object's life.
// Not cleared: the kernel writes the records [0, n_k) of every member it is launched for, and download_records reads no other.
template <typename O>
int ensure_accel_slab(O* o, const char* where) {
  if (o->accm) return NBX_OK;
  char* dev = nullptr;
  const int rc = device_alloc(&dev, o->rec * span_of(o, 0, o->members).vel_count, where, "the accelerations");
  if (rc == NBX_OK) o->accm = dev;
  return rc;
}

template <typename O, typename Launch, typename Prepare>
int batch_accel(O* o, const char* where, int32_t first, int32_t count, void* ax, void* ay, void* az, Prepare prepare) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || (!ax && !ay && !az)) return NBX_OK;
  const int k = nbx::ensemble_instance_index(o->plan.step);  // *_create has resolved the step's launcher from the same index
  if (k < 0) return fail(NBX_ERR_STATE, std::string(where) + ": no kernel instance for this bodies_per_lane / precision");
  rc = use_device(o);
  if (rc) return rc;
  rc = ensure_accel_slab(o, where);
  if (rc) return rc;
  rc = prepare(o);
  if (rc) return rc;
  kAccelLaunchers<O, Launch>[(size_t)k](o, first, count);
  HIP_TRY(hipGetLastError());
  return o->precision == 32 ? download_records<float>(o, first, count, o->accm, false, (float*)ax, (float*)ay, (float*)az)
                            : download_records<double>(o, first, count, o->accm, false, (double*)ax, (double*)ay, (double*)az);
  });
}

}  // namespace nbx_detail
#pragma GCC visibility pop
