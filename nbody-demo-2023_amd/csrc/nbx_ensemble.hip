// nbx_ensemble.hip -- include/nbx_ensemble.h over the kernels of nbx_ensemble_kernels.hpp: S independent systems of n bodies,
// one launch per time step for all of them.  The launch shape and the kernel instance come from plan_ensemble (nbx_plan.hpp);
// this file instantiates exactly kEnsembleInstances and launches the one the plan names.
//
// Plain launches on the ensemble's own non-blocking stream, no graph capture: one launch per step costs the host 3-4 us, and
// an ensemble worth creating has more pair work per step than that (64 members of 2048 bodies: 2.7e8 pairs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "nbx_ensemble_internal.hpp"
#include "nbx_ensemble_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

constexpr int kMaxProfiledLaunches = 8192;

template <typename T>
EnsembleArgs<T> ensemble_args(const nbx_ensemble* e, double dt) {
  using T4 = typename V4<T>::type;
  EnsembleArgs<T> a{};
  a.member0.posm = (const T4*)e->posm[e->cur]; a.member0.posm_next = (T4*)e->posm[e->cur ^ 1];
  a.member0.velm = (T4*)e->velm; a.member0.ke_part = e->ke_part;
  a.member0.i_begin = 0; a.member0.i_count = e->n; a.member0.own_pad = e->own_pad; a.member0.j_per_split = e->plan.n_alloc;
  a.member0.n_alloc = e->plan.n_alloc; a.member0.dt = (T)dt;
  a.pos_stride = (unsigned)e->pos_stride; a.vel_stride = (unsigned)e->own_pad; a.ke_stride = (unsigned)e->plan.grid_x;
  return a;
}

// one launcher per entry of kEnsembleInstances -- the only ensemble_step_kernel instances this library compiles
template <int I>
void launch_instance(nbx_ensemble* e, double dt) {
  constexpr Instance k = kEnsembleInstances[I];
  static_assert(k.kind == INST_JLANE, "an ensemble steps with the one-launch kernel body");
  const dim3 grid(e->plan.grid_x, e->plan.grid_y);
  if constexpr (k.precision == 32)
    hipLaunchKernelGGL((ensemble_step_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, e->stream, ensemble_args<float>(e, dt));
  else
    hipLaunchKernelGGL((ensemble_step_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, e->stream, ensemble_args<double>(e, dt));
}
template <int... I>
constexpr std::array<void (*)(nbx_ensemble*, double), sizeof...(I)> make_launchers(std::integer_sequence<int, I...>) {
  return {{&launch_instance<I>...}};
}
constexpr auto kLaunchers = make_launchers(std::make_integer_sequence<int, kEnsembleInstanceCount>{});

int use_device(nbx_ensemble* e) {
  HIP_TRY(hipSetDevice(e->device));
  return NBX_OK;
}

int enqueue_step(nbx_ensemble* e, double dt) {
  const bool prof = e->profiling && e->ev_used + 2 <= e->ev.size();
  if (prof) HIP_TRY(hipEventRecord(e->ev[e->ev_used], e->stream));
  e->launch_step(e, dt);
  if (prof) {
    HIP_TRY(hipEventRecord(e->ev[e->ev_used + 1], e->stream));
    e->ev_used += 2;
  }
  HIP_TRY(hipGetLastError());
  e->have_parts = true;
  return NBX_OK;
}

// every member's partials -> ke_dev[slot * members + m], fixed order
int enqueue_ke_reduce(nbx_ensemble* e, int slot) {
  hipLaunchKernelGGL(ensemble_ke_reduce_kernel, dim3(e->members), dim3(kBlock), 0, e->stream, (const double*)e->ke_part, e->plan.grid_x,
                     e->ke_dev + (size_t)slot * e->members);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

int ensure_ke_cap(nbx_ensemble* e, size_t need) {
  if (need <= e->ke_cap) return NBX_OK;
  if (e->ke_dev) HIP_TRY(hipFree(e->ke_dev));
  e->ke_dev = nullptr;
  e->ke_cap = 0;
  hipError_t err = hipMalloc(&e->ke_dev, sizeof(double) * need);
  if (err != hipSuccess) return fail(err == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE, std::string("nbx_ensemble: hipMalloc of the energy trace: ") + hipGetErrorString(err));
  e->ke_cap = need;
  return NBX_OK;
}

int drain_profile(nbx_ensemble* e) {
  for (size_t k = 0; k + 1 < e->ev_used; k += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev[k], e->ev[k + 1]));
    e->step_ms_total += ms;
    e->launches_timed += 1;
  }
  e->ev_used = 0;
  return NBX_OK;
}

template <typename T>
int upload_t(nbx_ensemble* e, int first, int count, const T* px, const T* py, const T* pz, const T* vx, const T* vy, const T* vz, const T* m) {
  using T4 = typename V4<T>::type;
  // the members' records as they lie on the device, spare records included (zero): one copy per buffer
  T4 zero; zero.x = zero.y = zero.z = zero.w = (T)0;
  std::vector<T4> hp((size_t)count * e->pos_stride, zero), hv((size_t)count * e->own_pad, zero);
  const T G = grav_const<T>();
  for (int k = 0; k < count; ++k) {
    T4* p = hp.data() + (size_t)k * e->pos_stride;
    T4* v = hv.data() + (size_t)k * e->own_pad;
    const size_t h = (size_t)k * e->n;
    for (int i = 0; i < e->n; ++i) {
      T4 r; r.x = px[h + i]; r.y = py[h + i]; r.z = pz[h + i]; r.w = (G * m[h + i]) * gm_prescale<T>();
      p[i] = r;
      T4 q; q.x = vx[h + i]; q.y = vy[h + i]; q.z = vz[h + i]; q.w = m[h + i];
      v[i] = q;
    }
  }
  const size_t pos_off = sizeof(T4) * (size_t)first * e->pos_stride, vel_off = sizeof(T4) * (size_t)first * e->own_pad;
  HIP_TRY(hipMemcpyAsync((char*)e->posm[0] + pos_off, hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync((char*)e->posm[1] + pos_off, hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync((char*)e->velm + vel_off, hv.data(), sizeof(T4) * hv.size(), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return NBX_OK;
}

template <typename T>
int download_t(nbx_ensemble* e, int first, int count, T* px, T* py, T* pz, T* vx, T* vy, T* vz) {
  using T4 = typename V4<T>::type;
  if (px || py || pz) {
    std::vector<T4> hp((size_t)count * e->pos_stride);
    HIP_TRY(hipMemcpyAsync(hp.data(), (const char*)e->posm[e->cur] + sizeof(T4) * (size_t)first * e->pos_stride, sizeof(T4) * hp.size(),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int k = 0; k < count; ++k) {
      const T4* p = hp.data() + (size_t)k * e->pos_stride;
      const size_t h = (size_t)k * e->n;
      for (int i = 0; i < e->n; ++i) {
        if (px) px[h + i] = p[i].x;
        if (py) py[h + i] = p[i].y;
        if (pz) pz[h + i] = p[i].z;
      }
    }
  }
  if (vx || vy || vz) {
    std::vector<T4> hv((size_t)count * e->own_pad);
    HIP_TRY(hipMemcpyAsync(hv.data(), (const char*)e->velm + sizeof(T4) * (size_t)first * e->own_pad, sizeof(T4) * hv.size(),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int k = 0; k < count; ++k) {
      const T4* v = hv.data() + (size_t)k * e->own_pad;
      const size_t h = (size_t)k * e->n;
      for (int i = 0; i < e->n; ++i) {
        if (vx) vx[h + i] = v[i].x;
        if (vy) vy[h + i] = v[i].y;
        if (vz) vz[h + i] = v[i].z;
      }
    }
  }
  return NBX_OK;
}

int step_common(nbx_ensemble* e, const char* where, double dt, int32_t nsteps, double* ke_last, double* ke_trace) {
  return guarded(where, [&]() -> int {
  if (!e) return fail(NBX_ERR_ARG, std::string(where) + ": ensemble is NULL");
  if (nsteps < 0) return fail(NBX_ERR_ARG, std::string(where) + ": nsteps < 0");
  if (e->uploaded_count != e->members)
    return fail(NBX_ERR_STATE, std::string(where) + ": " + std::to_string(e->members - e->uploaded_count) + " of " + std::to_string(e->members) +
                                   " members have not been uploaded (nbx_ensemble_upload)");
  int rc = use_device(e);
  if (rc) return rc;
  const size_t S = (size_t)e->members;
  if (ke_trace || ke_last) {
    rc = ensure_ke_cap(e, S * (size_t)(ke_trace ? std::max(nsteps, 1) : 1));
    if (rc) return rc;
  }
  for (int s = 0; s < nsteps; ++s) {
    rc = enqueue_step(e, dt);
    if (rc) return rc;
    e->cur ^= 1;
    e->steps_done += 1;
    if (ke_trace) rc = enqueue_ke_reduce(e, s);
    else if (ke_last && s == nsteps - 1) rc = enqueue_ke_reduce(e, 0);
    if (rc) return rc;
  }
  if (ke_trace && nsteps > 0) {
    HIP_TRY(hipMemcpyAsync(ke_trace, e->ke_dev, sizeof(double) * S * (size_t)nsteps, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < S * (size_t)nsteps; ++k) ke_trace[k] *= 0.5;  // ver7/GSimulation.cpp:200
  } else if (ke_last) {
    if (nsteps > 0 || e->have_parts) {
      if (nsteps == 0) {
        rc = enqueue_ke_reduce(e, 0);
        if (rc) return rc;
      }
      HIP_TRY(hipMemcpyAsync(ke_last, e->ke_dev, sizeof(double) * S, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
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

int nbx_ensemble_create(nbx_ensemble** out, int32_t n, int32_t precision, int32_t members, const nbx_opts* opts) {
  return guarded("nbx_ensemble_create", [&]() -> int {
  if (!out) return fail(NBX_ERR_ARG, "nbx_ensemble_create: out is NULL");
  *out = nullptr;
  nbx_opts o;
  std::memset(&o, 0, sizeof(o));
  o.device = -1;
  if (opts) {
    if (opts->struct_size != 0 && opts->struct_size != (int32_t)sizeof(nbx_opts))
      return fail(NBX_ERR_ARG, "nbx_ensemble_create: nbx_opts.struct_size does not match this library");
    o = *opts;
  }
  // every argument check before the first HIP call: whether a plan exists does not depend on the device (its CU count only
  // moves the choice of bodies per wave, and auto never picks a shape without an instance)
  EnsemblePlan plan;
  const char* msg = nullptr;
  if (plan_ensemble(n, precision, members, 0, o, &plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(NBX_ERR_DEVICE, "nbx_ensemble_create: no HIP device available (libnbx has no CPU path)");
  int dev = o.device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return fail(NBX_ERR_DEVICE, "nbx_ensemble_create: hipGetDevice failed");
  }
  if (dev >= ndev) return fail(NBX_ERR_ARG, "nbx_ensemble_create: device ordinal out of range");

  nbx_ensemble* e = new (std::nothrow) nbx_ensemble();
  if (!e) return fail(NBX_ERR_ALLOC, "nbx_ensemble_create: out of host memory");
  struct Owner { nbx_ensemble* e; ~Owner() { nbx_ensemble_destroy(e); } } owner{e};  // every failure path below frees the ensemble
  e->device = dev;
  e->n = n;
  e->members = members;
  e->precision = precision;
  e->rec = precision == 32 ? sizeof(float4) : sizeof(double4);
  e->own_pad = round_up(n, kBlock);
  e->uploaded.assign((size_t)members, 0);

#define CREATE_TRY(expr)                                                                          \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      std::string m_ = std::string("nbx_ensemble_create: " #expr ": ") + hipGetErrorString(e_);   \
      return fail(e_ == hipErrorOutOfMemory ? NBX_ERR_ALLOC : NBX_ERR_DEVICE, m_);                \
    }                                                                                             \
  } while (0)

  CREATE_TRY(hipSetDevice(dev));
  CREATE_TRY(hipGetDeviceProperties(&e->prop, dev));
  CREATE_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  if (plan_ensemble(n, precision, members, e->prop.multiProcessorCount, o, &e->plan, &msg) != NBX_OK) return fail(NBX_ERR_ARG, msg);
  const int k = ensemble_instance_index(e->plan.step);
  if (k < 0) return fail(NBX_ERR_ARG, "nbx_ensemble_create: no kernel instance for this bodies_per_lane / precision");
  e->launch_step = kLaunchers[k];

  e->pos_stride = (size_t)e->plan.n_alloc + kSgprOverread;
  const size_t pos_bytes = e->rec * e->pos_stride * (size_t)members, vel_bytes = e->rec * (size_t)e->own_pad * (size_t)members;
  const size_t part_bytes = sizeof(double) * (size_t)e->plan.grid_x * (size_t)members;
  CREATE_TRY(hipMalloc(&e->posm[0], pos_bytes));
  CREATE_TRY(hipMalloc(&e->posm[1], pos_bytes));
  CREATE_TRY(hipMalloc(&e->velm, vel_bytes));
  CREATE_TRY(hipMalloc(&e->ke_part, part_bytes));
  CREATE_TRY(hipMemsetAsync(e->posm[0], 0, pos_bytes, e->stream));
  CREATE_TRY(hipMemsetAsync(e->posm[1], 0, pos_bytes, e->stream));
  CREATE_TRY(hipMemsetAsync(e->velm, 0, vel_bytes, e->stream));
  CREATE_TRY(hipMemsetAsync(e->ke_part, 0, part_bytes, e->stream));
  CREATE_TRY(hipStreamSynchronize(e->stream));
#undef CREATE_TRY
  owner.e = nullptr;
  *out = e;
  last_error().clear();
  return NBX_OK;
  });
}

void nbx_ensemble_destroy(nbx_ensemble* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (hipEvent_t ev : e->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (e->posm[0]) (void)hipFree(e->posm[0]);
  if (e->posm[1]) (void)hipFree(e->posm[1]);
  if (e->velm) (void)hipFree(e->velm);
  if (e->ke_part) (void)hipFree(e->ke_part);
  if (e->ke_dev) (void)hipFree(e->ke_dev);
  if (e->diag_part) (void)hipFree(e->diag_part);
  if (e->diag_dev) (void)hipFree(e->diag_dev);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int nbx_ensemble_upload(nbx_ensemble* e, int32_t first, int32_t count, const void* px, const void* py, const void* pz, const void* vx,
                        const void* vy, const void* vz, const void* m) {
  return guarded("nbx_ensemble_upload", [&]() -> int {
  if (!e) return fail(NBX_ERR_ARG, "nbx_ensemble_upload: ensemble is NULL");
  if (first < 0 || count < 0 || (long long)first + count > e->members)
    return fail(NBX_ERR_ARG, "nbx_ensemble_upload: members [first, first + count) are outside [0, members)");
  if (!px || !py || !pz || !vx || !vy || !vz || !m) return fail(NBX_ERR_ARG, "nbx_ensemble_upload: NULL array");
  if (count == 0) return NBX_OK;
  int rc = use_device(e);
  if (rc) return rc;
  rc = e->precision == 32
           ? upload_t<float>(e, first, count, (const float*)px, (const float*)py, (const float*)pz, (const float*)vx, (const float*)vy,
                             (const float*)vz, (const float*)m)
           : upload_t<double>(e, first, count, (const double*)px, (const double*)py, (const double*)pz, (const double*)vx,
                              (const double*)vy, (const double*)vz, (const double*)m);
  if (rc) return rc;
  for (int k = first; k < first + count; ++k)
    if (!e->uploaded[k]) { e->uploaded[k] = 1; e->uploaded_count += 1; }
  e->have_parts = false;  // the partials on the device belong to the previous trajectories
  return NBX_OK;
  });
}

int nbx_ensemble_step(nbx_ensemble* e, double dt, int32_t nsteps, double* kenergy_out) {
  return step_common(e, "nbx_ensemble_step", dt, nsteps, kenergy_out, nullptr);
}

int nbx_ensemble_step_trace(nbx_ensemble* e, double dt, int32_t nsteps, double* ke_trace) {
  if (!ke_trace) return guarded("nbx_ensemble_step_trace", [&]() -> int { return fail(NBX_ERR_ARG, "nbx_ensemble_step_trace: ke_trace is NULL"); });
  return step_common(e, "nbx_ensemble_step_trace", dt, nsteps, nullptr, ke_trace);
}

int nbx_ensemble_download(nbx_ensemble* e, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return guarded("nbx_ensemble_download", [&]() -> int {
  if (!e) return fail(NBX_ERR_ARG, "nbx_ensemble_download: ensemble is NULL");
  if (first < 0 || count < 0 || (long long)first + count > e->members)
    return fail(NBX_ERR_ARG, "nbx_ensemble_download: members [first, first + count) are outside [0, members)");
  for (int k = first; k < first + count; ++k)
    if (!e->uploaded[k]) return fail(NBX_ERR_STATE, "nbx_ensemble_download: member " + std::to_string(k) + " has not been uploaded");
  if (count == 0) return NBX_OK;
  int rc = use_device(e);
  if (rc) return rc;
  return e->precision == 32
             ? download_t<float>(e, first, count, (float*)px, (float*)py, (float*)pz, (float*)vx, (float*)vy, (float*)vz)
             : download_t<double>(e, first, count, (double*)px, (double*)py, (double*)pz, (double*)vx, (double*)vy, (double*)vz);
  });
}

int nbx_ensemble_sync(nbx_ensemble* e) {
  return guarded("nbx_ensemble_sync", [&]() -> int {
  if (!e) return fail(NBX_ERR_ARG, "nbx_ensemble_sync: ensemble is NULL");
  int rc = use_device(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return NBX_OK;
  });
}

int nbx_ensemble_profile(nbx_ensemble* e, int32_t enable) {
  return guarded("nbx_ensemble_profile", [&]() -> int {
  if (!e) return fail(NBX_ERR_ARG, "nbx_ensemble_profile: ensemble is NULL");
  int rc = use_device(e);
  if (rc) return rc;
  if (enable && e->ev.empty()) {
    e->ev.assign(2 * kMaxProfiledLaunches, nullptr);
    for (auto& ev : e->ev) HIP_TRY(hipEventCreate(&ev));
  }
  if (!enable && e->profiling) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = drain_profile(e);
    if (rc) return rc;
  }
  if (enable && !e->profiling) {
    e->step_ms_total = 0.0;
    e->launches_timed = 0;
    e->ev_used = 0;
  }
  e->profiling = enable != 0;
  return NBX_OK;
  });
}

int nbx_ensemble_stats(nbx_ensemble* e, nbx_ensemble_stats_t* s) {
  return guarded("nbx_ensemble_stats", [&]() -> int {
  if (!e || !s) return fail(NBX_ERR_ARG, "nbx_ensemble_stats: NULL argument");
  if (s->struct_size != 0 && s->struct_size != (int32_t)sizeof(nbx_ensemble_stats_t))
    return fail(NBX_ERR_ARG, "nbx_ensemble_stats: nbx_ensemble_stats_t.struct_size does not match this library");
  int rc = use_device(e);
  if (rc) return rc;
  if (e->ev_used) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    rc = drain_profile(e);
    if (rc) return rc;
  }
  std::memset(s, 0, sizeof(*s));
  s->struct_size = (int32_t)sizeof(nbx_ensemble_stats_t);
  s->n = e->n; s->n_alloc = e->plan.n_alloc; s->members = e->members; s->precision = e->precision;
  s->bodies_per_lane = e->plan.NB; s->inner_loop = e->plan.loop == LOOP_ASM ? NBX_LOOP_ASM : NBX_LOOP_CXX;
  s->grid_x = e->plan.grid_x; s->grid_y = e->plan.grid_y; s->block = kBlock; s->cu_count = e->prop.multiProcessorCount;
  s->steps_done = e->steps_done; s->launches_timed = e->launches_timed; s->step_ms_total = e->step_ms_total;
  return NBX_OK;
  });
}

}  // extern "C"
