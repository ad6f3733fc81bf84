// nbx_ragged.hip -- include/nbx_ragged.h over the kernels of nbx_ragged_kernels.hpp: independent systems of different size, one
// launch per time step for all of them.  The layout, the work list and the kernel instance come from plan_ragged
// (nbx_plan.hpp); this file instantiates exactly kEnsembleInstances -- the shapes a jlane context can run -- as
// ragged_step_kernel and launches the one the plan names.
//
// Plain launches on the object's own non-blocking stream, no graph capture, as for an ensemble (nbx_ensemble.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "nbx_ragged_internal.hpp"  // struct nbx_ragged; error plumbing; nbx_plan.hpp: nbx::RaggedPlan
#include "nbx_ragged_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

constexpr int kMaxProfiledLaunches = 8192;

template <typename T>
RaggedArgs<T> ragged_args(const nbx_ragged* r, double dt) {
  using T4 = typename V4<T>::type;
  RaggedArgs<T> a{};
  a.posm = (const T4*)r->posm[r->cur]; a.posm_next = (T4*)r->posm[r->cur ^ 1];
  a.velm = (T4*)r->velm; a.ke_part = r->ke_part; a.work = r->work_dev; a.dt = (T)dt;
  return a;
}

// one launcher per entry of kEnsembleInstances -- the only ragged_step_kernel instances this library compiles
template <int I>
void launch_instance(nbx_ragged* r, double dt) {
  constexpr Instance k = kEnsembleInstances[I];
  static_assert(k.kind == INST_JLANE, "a member steps with the one-launch kernel body");
  const dim3 grid(r->plan.W);
  if constexpr (k.precision == 32)
    hipLaunchKernelGGL((ragged_step_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, r->stream, ragged_args<float>(r, dt));
  else
    hipLaunchKernelGGL((ragged_step_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, r->stream, ragged_args<double>(r, dt));
}
template <int... I>
constexpr std::array<void (*)(nbx_ragged*, double), sizeof...(I)> make_launchers(std::integer_sequence<int, I...>) {
  return {{&launch_instance<I>...}};
}
constexpr auto kLaunchers = make_launchers(std::make_integer_sequence<int, kEnsembleInstanceCount>{});

int use_device(nbx_ragged* r) {
  HIP_TRY(hipSetDevice(r->device));
  return NBX_OK;
}

int enqueue_step(nbx_ragged* r, double dt) {
  const bool prof = r->profiling && r->ev_used + 2 <= r->ev.size();
  if (prof) HIP_TRY(hipEventRecord(r->ev[r->ev_used], r->stream));
  r->launch_step(r, dt);
  if (prof) {
    HIP_TRY(hipEventRecord(r->ev[r->ev_used + 1], r->stream));
    r->ev_used += 2;
  }
  HIP_TRY(hipGetLastError());
  r->have_parts = true;
  return NBX_OK;
}

// every member's partials -> ke_dev[slot * members + m], fixed order
int enqueue_ke_reduce(nbx_ragged* r, int slot) {
  hipLaunchKernelGGL(ragged_ke_reduce_kernel, dim3(r->members), dim3(kBlock), 0, r->stream, (const double*)r->ke_part,
                     (const RaggedParts*)r->parts_dev, r->ke_dev + (size_t)slot * r->members);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

int ensure_ke_cap(nbx_ragged* r, size_t need) {
  if (need <= r->ke_cap) return NBX_OK;
  if (r->ke_dev) HIP_TRY(hipFree(r->ke_dev));
  r->ke_dev = nullptr;
  r->ke_cap = 0;
  hipError_t err = hipMalloc(&r->ke_dev, sizeof(double) * need);
  if (err != hipSuccess) return fail(err == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE, std::string("nbx_ragged: hipMalloc of the energy trace: ") + hipGetErrorString(err));
  r->ke_cap = need;
  return NBX_OK;
}

int drain_profile(nbx_ragged* r) {
  for (size_t k = 0; k + 1 < r->ev_used; k += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r->ev[k], r->ev[k + 1]));
    r->step_ms_total += ms;
    r->launches_timed += 1;
  }
  r->ev_used = 0;
  return NBX_OK;
}

// Members [first, first + count) lie one behind the other on the device: records [pos_begin, pos_end) of posm, [vel_begin, vel_end) of velm.
struct Span { size_t pos_begin, pos_count, vel_begin, vel_count; };
Span span_of(const nbx_ragged* r, int first, int count) {
  const RaggedMember &a = r->plan.member[(size_t)first], &b = r->plan.member[(size_t)(first + count - 1)];
  return {a.pos_off, (size_t)b.pos_off + b.n_alloc + kSgprOverread - a.pos_off, a.vel_off, (size_t)b.vel_off + b.n_alloc - a.vel_off};
}

template <typename T>
int upload_t(nbx_ragged* r, int first, int count, const T* px, const T* py, const T* pz, const T* vx, const T* vy, const T* vz, const T* m) {
  using T4 = typename V4<T>::type;
  // the members' records as they lie on the device, padding and spare records included (zero): one copy per buffer
  const Span sp = span_of(r, first, count);
  T4 zero; zero.x = zero.y = zero.z = zero.w = (T)0;
  std::vector<T4> hp(sp.pos_count, zero), hv(sp.vel_count, zero);
  const T G = grav_const<T>();
  size_t h = 0;  // the member's first element in the host arrays
  for (int k = first; k < first + count; ++k) {
    const RaggedMember& mem = r->plan.member[(size_t)k];
    T4* p = hp.data() + (mem.pos_off - sp.pos_begin);
    T4* v = hv.data() + (mem.vel_off - sp.vel_begin);
    for (int i = 0; i < mem.n; ++i) {
      T4 q; q.x = px[h + i]; q.y = py[h + i]; q.z = pz[h + i]; q.w = (G * m[h + i]) * gm_prescale<T>();
      p[i] = q;
      T4 u; u.x = vx[h + i]; u.y = vy[h + i]; u.z = vz[h + i]; u.w = m[h + i];
      v[i] = u;
    }
    h += (size_t)mem.n;
  }
  const size_t pos_off = sizeof(T4) * sp.pos_begin, vel_off = sizeof(T4) * sp.vel_begin;
  HIP_TRY(hipMemcpyAsync((char*)r->posm[0] + pos_off, hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, r->stream));
  HIP_TRY(hipMemcpyAsync((char*)r->posm[1] + pos_off, hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, r->stream));
  HIP_TRY(hipMemcpyAsync((char*)r->velm + vel_off, hv.data(), sizeof(T4) * hv.size(), hipMemcpyHostToDevice, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  return NBX_OK;
}

template <typename T>
int download_t(nbx_ragged* r, int first, int count, T* px, T* py, T* pz, T* vx, T* vy, T* vz) {
  using T4 = typename V4<T>::type;
  const Span sp = span_of(r, first, count);
  if (px || py || pz) {
    std::vector<T4> hp(sp.pos_count);
    HIP_TRY(hipMemcpyAsync(hp.data(), (const char*)r->posm[r->cur] + sizeof(T4) * sp.pos_begin, sizeof(T4) * hp.size(), hipMemcpyDeviceToHost,
                           r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    size_t h = 0;
    for (int k = first; k < first + count; ++k) {
      const RaggedMember& mem = r->plan.member[(size_t)k];
      const T4* p = hp.data() + (mem.pos_off - sp.pos_begin);
      for (int i = 0; i < mem.n; ++i) {
        if (px) px[h + i] = p[i].x;
        if (py) py[h + i] = p[i].y;
        if (pz) pz[h + i] = p[i].z;
      }
      h += (size_t)mem.n;
    }
  }
  if (vx || vy || vz) {
    std::vector<T4> hv(sp.vel_count);
    HIP_TRY(hipMemcpyAsync(hv.data(), (const char*)r->velm + sizeof(T4) * sp.vel_begin, sizeof(T4) * hv.size(), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    size_t h = 0;
    for (int k = first; k < first + count; ++k) {
      const RaggedMember& mem = r->plan.member[(size_t)k];
      const T4* v = hv.data() + (mem.vel_off - sp.vel_begin);
      for (int i = 0; i < mem.n; ++i) {
        if (vx) vx[h + i] = v[i].x;
        if (vy) vy[h + i] = v[i].y;
        if (vz) vz[h + i] = v[i].z;
      }
      h += (size_t)mem.n;
    }
  }
  return NBX_OK;
}

int step_common(nbx_ragged* r, const char* where, double dt, int32_t nsteps, double* ke_last, double* ke_trace) {
  return guarded(where, [&]() -> int {
  if (!r) return fail(NBX_ERR_ARG, std::string(where) + ": ragged ensemble is NULL");
  if (nsteps < 0) return fail(NBX_ERR_ARG, std::string(where) + ": nsteps < 0");
  if (r->uploaded_count != r->members)
    return fail(NBX_ERR_STATE, std::string(where) + ": " + std::to_string(r->members - r->uploaded_count) + " of " + std::to_string(r->members) +
                                   " members have not been uploaded (nbx_ragged_upload)");
  int rc = use_device(r);
  if (rc) return rc;
  const size_t S = (size_t)r->members;
  if (ke_trace || ke_last) {
    rc = ensure_ke_cap(r, S * (size_t)(ke_trace ? std::max(nsteps, 1) : 1));
    if (rc) return rc;
  }
  for (int s = 0; s < nsteps; ++s) {
    rc = enqueue_step(r, dt);
    if (rc) return rc;
    r->cur ^= 1;
    r->steps_done += 1;
    if (ke_trace) rc = enqueue_ke_reduce(r, s);
    else if (ke_last && s == nsteps - 1) rc = enqueue_ke_reduce(r, 0);
    if (rc) return rc;
  }
  if (ke_trace && nsteps > 0) {
    HIP_TRY(hipMemcpyAsync(ke_trace, r->ke_dev, sizeof(double) * S * (size_t)nsteps, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (size_t k = 0; k < S * (size_t)nsteps; ++k) ke_trace[k] *= 0.5;  // ver7/GSimulation.cpp:200
  } else if (ke_last) {
    if (nsteps > 0 || r->have_parts) {
      if (nsteps == 0) {
        rc = enqueue_ke_reduce(r, 0);
        if (rc) return rc;
      }
      HIP_TRY(hipMemcpyAsync(ke_last, r->ke_dev, sizeof(double) * S, hipMemcpyDeviceToHost, r->stream));
      HIP_TRY(hipStreamSynchronize(r->stream));
      for (size_t m = 0; m < S; ++m) ke_last[m] *= 0.5;
    } else {
      for (size_t m = 0; m < S; ++m) ke_last[m] = 0.0;
    }
  }
  return NBX_OK;
  });
}

}  // namespace

extern "C" {

int nbx_ragged_create(nbx_ragged** out, int32_t members, const int32_t* n, int32_t precision, const nbx_opts* opts) {
  return guarded("nbx_ragged_create", [&]() -> int {
  if (!out) return fail(NBX_ERR_ARG, "nbx_ragged_create: out is NULL");
  *out = nullptr;
  nbx_opts o;
  std::memset(&o, 0, sizeof(o));
  o.device = -1;
  if (opts) {
    if (opts->struct_size != 0 && opts->struct_size != (int32_t)sizeof(nbx_opts))
      return fail(NBX_ERR_ARG, "nbx_ragged_create: nbx_opts.struct_size does not match this library");
    o = *opts;
  }
  // every argument check before the first HIP call: whether a plan exists does not depend on the device (its CU count only
  // moves the choice of bodies per wave, and auto never picks a shape without an instance)
  static_assert(std::is_same<int32_t, int>::value, "plan_ragged reads the sizes as int");
  const char* msg = nullptr;
  {
    RaggedPlan plan;
    if (plan_ragged(n, members, precision, 0, o, &plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);
  }

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(NBX_ERR_DEVICE, "nbx_ragged_create: no HIP device available (libnbx has no CPU path)");
  int dev = o.device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return fail(NBX_ERR_DEVICE, "nbx_ragged_create: hipGetDevice failed");
  }
  if (dev >= ndev) return fail(NBX_ERR_ARG, "nbx_ragged_create: device ordinal out of range");

  nbx_ragged* r = new (std::nothrow) nbx_ragged();
  if (!r) return fail(NBX_ERR_ALLOC, "nbx_ragged_create: out of host memory");
  struct Owner { nbx_ragged* r; ~Owner() { nbx_ragged_destroy(r); } } owner{r};  // every failure path below frees the object
  r->device = dev;
  r->members = members;
  r->precision = precision;
  r->rec = precision == 32 ? sizeof(float4) : sizeof(double4);
  r->uploaded.assign((size_t)members, 0);

#define CREATE_TRY(expr)                                                                          \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      std::string m_ = std::string("nbx_ragged_create: " #expr ": ") + hipGetErrorString(e_);     \
      return fail(e_ == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE, m_);                \
    }                                                                                             \
  } while (0)

  CREATE_TRY(hipSetDevice(dev));
  CREATE_TRY(hipGetDeviceProperties(&r->prop, dev));
  CREATE_TRY(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  if (plan_ragged(n, members, precision, r->prop.multiProcessorCount, o, &r->plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);
  const int k = ensemble_instance_index(r->plan.step);
  if (k < 0) return fail(NBX_ERR_ARG, "nbx_ragged_create: no kernel instance for this bodies_per_lane / precision");
  r->launch_step = kLaunchers[k];

  const RaggedPlan& p = r->plan;
  std::vector<RaggedParts> parts((size_t)members);
  for (int m = 0; m < members; ++m) parts[(size_t)m] = {p.member[(size_t)m].ke_off, p.member[(size_t)m].grid};
  const size_t pos_bytes = r->rec * (size_t)p.pos_records, vel_bytes = r->rec * (size_t)p.vel_records;
  const size_t part_bytes = sizeof(double) * (size_t)p.ke_parts, work_bytes = sizeof(RaggedWork) * p.work.size();
  CREATE_TRY(hipMalloc(&r->posm[0], pos_bytes));
  CREATE_TRY(hipMalloc(&r->posm[1], pos_bytes));
  CREATE_TRY(hipMalloc(&r->velm, vel_bytes));
  CREATE_TRY(hipMalloc(&r->ke_part, part_bytes));
  CREATE_TRY(hipMalloc(&r->work_dev, work_bytes));
  CREATE_TRY(hipMalloc(&r->parts_dev, sizeof(RaggedParts) * parts.size()));
  CREATE_TRY(hipMemsetAsync(r->posm[0], 0, pos_bytes, r->stream));
  CREATE_TRY(hipMemsetAsync(r->posm[1], 0, pos_bytes, r->stream));
  CREATE_TRY(hipMemsetAsync(r->velm, 0, vel_bytes, r->stream));
  CREATE_TRY(hipMemsetAsync(r->ke_part, 0, part_bytes, r->stream));
  CREATE_TRY(hipMemcpyAsync(r->work_dev, p.work.data(), work_bytes, hipMemcpyHostToDevice, r->stream));
  CREATE_TRY(hipMemcpyAsync(r->parts_dev, parts.data(), sizeof(RaggedParts) * parts.size(), hipMemcpyHostToDevice, r->stream));
  CREATE_TRY(hipStreamSynchronize(r->stream));
#undef CREATE_TRY
  owner.r = nullptr;
  *out = r;
  last_error().clear();
  return NBX_OK;
  });
}

void nbx_ragged_destroy(nbx_ragged* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  for (hipEvent_t ev : r->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (r->posm[0]) (void)hipFree(r->posm[0]);
  if (r->posm[1]) (void)hipFree(r->posm[1]);
  if (r->velm) (void)hipFree(r->velm);
  if (r->ke_part) (void)hipFree(r->ke_part);
  if (r->work_dev) (void)hipFree(r->work_dev);
  if (r->parts_dev) (void)hipFree(r->parts_dev);
  if (r->ke_dev) (void)hipFree(r->ke_dev);
  if (r->diag_work_dev) (void)hipFree(r->diag_work_dev);  // the buffers of nbx_ragged_diag.hip
  if (r->diag_rows_dev) (void)hipFree(r->diag_rows_dev);
  if (r->diag_part) (void)hipFree(r->diag_part);
  if (r->diag_dev) (void)hipFree(r->diag_dev);
  if (r->stream) (void)hipStreamDestroy(r->stream);
  delete r;
}

int nbx_ragged_upload(nbx_ragged* r, int32_t first, int32_t count, const void* px, const void* py, const void* pz, const void* vx,
                      const void* vy, const void* vz, const void* m) {
  return guarded("nbx_ragged_upload", [&]() -> int {
  if (!r) return fail(NBX_ERR_ARG, "nbx_ragged_upload: ragged ensemble is NULL");
  if (first < 0 || count < 0 || (long long)first + count > r->members)
    return fail(NBX_ERR_ARG, "nbx_ragged_upload: members [first, first + count) are outside [0, members)");
  if (!px || !py || !pz || !vx || !vy || !vz || !m) return fail(NBX_ERR_ARG, "nbx_ragged_upload: NULL array");
  if (count == 0) return NBX_OK;
  int rc = use_device(r);
  if (rc) return rc;
  rc = r->precision == 32
           ? upload_t<float>(r, first, count, (const float*)px, (const float*)py, (const float*)pz, (const float*)vx, (const float*)vy,
                             (const float*)vz, (const float*)m)
           : upload_t<double>(r, first, count, (const double*)px, (const double*)py, (const double*)pz, (const double*)vx,
                              (const double*)vy, (const double*)vz, (const double*)m);
  if (rc) return rc;
  for (int k = first; k < first + count; ++k)
    if (!r->uploaded[k]) { r->uploaded[k] = 1; r->uploaded_count += 1; }
  r->have_parts = false;  // the partials on the device belong to the previous trajectories
  return NBX_OK;
  });
}

int nbx_ragged_step(nbx_ragged* r, double dt, int32_t nsteps, double* kenergy_out) {
  return step_common(r, "nbx_ragged_step", dt, nsteps, kenergy_out, nullptr);
}

int nbx_ragged_step_trace(nbx_ragged* r, double dt, int32_t nsteps, double* ke_trace) {
  if (!ke_trace) return guarded("nbx_ragged_step_trace", [&]() -> int { return fail(NBX_ERR_ARG, "nbx_ragged_step_trace: ke_trace is NULL"); });
  return step_common(r, "nbx_ragged_step_trace", dt, nsteps, nullptr, ke_trace);
}

int nbx_ragged_download(nbx_ragged* r, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return guarded("nbx_ragged_download", [&]() -> int {
  if (!r) return fail(NBX_ERR_ARG, "nbx_ragged_download: ragged ensemble is NULL");
  if (first < 0 || count < 0 || (long long)first + count > r->members)
    return fail(NBX_ERR_ARG, "nbx_ragged_download: members [first, first + count) are outside [0, members)");
  for (int k = first; k < first + count; ++k)
    if (!r->uploaded[k]) return fail(NBX_ERR_STATE, "nbx_ragged_download: member " + std::to_string(k) + " has not been uploaded");
  if (count == 0) return NBX_OK;
  int rc = use_device(r);
  if (rc) return rc;
  return r->precision == 32
             ? download_t<float>(r, first, count, (float*)px, (float*)py, (float*)pz, (float*)vx, (float*)vy, (float*)vz)
             : download_t<double>(r, first, count, (double*)px, (double*)py, (double*)pz, (double*)vx, (double*)vy, (double*)vz);
  });
}

int nbx_ragged_sync(nbx_ragged* r) {
  return guarded("nbx_ragged_sync", [&]() -> int {
  if (!r) return fail(NBX_ERR_ARG, "nbx_ragged_sync: ragged ensemble is NULL");
  int rc = use_device(r);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(r->stream));
  return NBX_OK;
  });
}

int nbx_ragged_profile(nbx_ragged* r, int32_t enable) {
  return guarded("nbx_ragged_profile", [&]() -> int {
  if (!r) return fail(NBX_ERR_ARG, "nbx_ragged_profile: ragged ensemble is NULL");
  int rc = use_device(r);
  if (rc) return rc;
  if (enable && r->ev.empty()) {
    r->ev.assign(2 * kMaxProfiledLaunches, nullptr);
    for (auto& ev : r->ev) HIP_TRY(hipEventCreate(&ev));
  }
  if (!enable && r->profiling) {
    HIP_TRY(hipStreamSynchronize(r->stream));
    rc = drain_profile(r);
    if (rc) return rc;
  }
  if (enable && !r->profiling) {
    r->step_ms_total = 0.0;
    r->launches_timed = 0;
    r->ev_used = 0;
  }
  r->profiling = enable != 0;
  return NBX_OK;
  });
}

int nbx_ragged_stats(nbx_ragged* r, nbx_ragged_stats_t* s) {
  return guarded("nbx_ragged_stats", [&]() -> int {
  if (!r || !s) return fail(NBX_ERR_ARG, "nbx_ragged_stats: NULL argument");
  if (s->struct_size != 0 && s->struct_size != (int32_t)sizeof(nbx_ragged_stats_t))
    return fail(NBX_ERR_ARG, "nbx_ragged_stats: nbx_ragged_stats_t.struct_size does not match this library");
  int rc = use_device(r);
  if (rc) return rc;
  if (r->ev_used) {
    HIP_TRY(hipStreamSynchronize(r->stream));
    rc = drain_profile(r);
    if (rc) return rc;
  }
  std::memset(s, 0, sizeof(*s));
  s->struct_size = (int32_t)sizeof(nbx_ragged_stats_t);
  s->members = r->members; s->precision = r->precision;
  s->n_min = r->plan.n_min; s->n_max = r->plan.n_max; s->bodies_total = (int32_t)r->plan.bodies_total;
  s->bodies_per_lane = r->plan.NB; s->inner_loop = r->plan.loop == LOOP_ASM ? NBX_LOOP_ASM : NBX_LOOP_CXX;
  s->grid_x = r->plan.W; s->block = kBlock; s->cu_count = r->prop.multiProcessorCount;
  s->pairs_per_step = r->plan.pairs_per_step;
  s->steps_done = r->steps_done; s->launches_timed = r->launches_timed; s->step_ms_total = r->step_ms_total;
  return NBX_OK;
  });
}

}  // extern "C"
