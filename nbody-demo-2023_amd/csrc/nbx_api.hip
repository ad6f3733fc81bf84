// nbx_api.hip -- the C-ABI of include/nbx.h over the gfx950 kernels of nbx_kernels.hpp.
//
// One context = one GPU's share of the reference's GSimulation::start() loop
// (ver7/GSimulation.cpp:138-200): it owns bodies [i_begin, i_begin+i_count), keeps
// {x,y,z,G*m} of ALL bodies resident (double buffered) and {vx,vy,vz,m} of its own.
// No CPU fallback exists: without a HIP device every entry point fails with NBX_ERR_DEVICE.
// What a context shares with the batch objects on the host -- device choice, the energy trace and its read-back, profiling and
// the event bracket, the shared part of create and destroy -- is nbx_object.hpp's; here are the kernel dispatch, graph replay,
// the slice and exchange protocol, and upload / download over a slice.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "nbx_internal.hpp"
#include "nbx_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace nbx_detail {
std::string& last_error() {
  thread_local std::string err;
  return err;
}
}  // namespace nbx_detail

namespace {

// ------------------------------------------------------------------------------------------
// kernel dispatch: one launcher per entry of kInstances (nbx_plan.hpp) -- the only kernel instances this library compiles
// ------------------------------------------------------------------------------------------
static_assert(kSgprGran == (kSgprAsmTrip<1> > 64 ? kSgprAsmTrip<1> : 64) && kSgprGran % kSgprAsmTrip<2> == 0 &&
                  kSgprGran % kSgprAsmTrip<4> == 0 && kTile % kSgprGran == 0,
              "j ranges are whole trips of the asm loop");

template <typename T>
ForceArgs<T> force_args(const nbx_ctx* c, double dt) {
  using T4 = typename V4<T>::type;
  ForceArgs<T> a{};
  a.posm = (const T4*)c->posm[c->cur]; a.posm_next = (T4*)c->posm[c->cur ^ 1]; a.posm_pairs = (const T4*)c->posm_pairs;
  a.accp = (T4*)c->accp; a.velm = (T4*)c->velm; a.ke_part = c->ke_part;
  a.i_begin = c->i_begin; a.i_count = c->i_count; a.own_pad = c->own_pad; a.j_per_split = c->plan.jps; a.n_alloc = c->n_alloc;
  a.dt = (T)dt; a.slice_bit = c->slice_bit;
  return a;
}

// acc_only: the jlane kernels store the accelerations instead of integrating (nbx_accel)
template <int I>
void launch_instance(nbx_ctx* c, double dt, int acc_only) {
  constexpr Instance k = kInstances[I];
  using T = std::conditional_t<k.precision == 32, float, double>;
  using T4 = typename V4<T>::type;
  const dim3 grid(c->plan.grid_x, c->plan.grid_y);
  if constexpr (k.kind == INST_EXACT)
    hipLaunchKernelGGL((force_exact_kernel<T, k.B == 1>), grid, dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur],
                       (const T*)c->mass_all, (T4*)c->accp, c->i_begin, c->i_count, c->n);
  else if constexpr (k.kind == INST_FORCE)
    hipLaunchKernelGGL((force_kernel<T, k.B, k.jsrc, k.epi, 1, k.math, k.ws, k.loop>), grid, dim3(kBlock), 0, c->stream, force_args<T>(c, dt));
  else if constexpr (k.precision == 32)  // jlane_depth: prefetch depth of the compiled loop / tail (nbx_plan.hpp)
    hipLaunchKernelGGL((force_jlane_kernel<k.B, jlane_depth(32, k.B), k.loop>), grid, dim3(kBlock), 0, c->stream, force_args<T>(c, dt), acc_only);
  else
    hipLaunchKernelGGL((force_jlane_kernel_f64<k.B, jlane_depth(64, k.B)>), grid, dim3(kBlock), 0, c->stream, force_args<T>(c, dt), acc_only);
}

template <int... I>
constexpr std::array<void (*)(nbx_ctx*, double, int), sizeof...(I)> make_launchers(std::integer_sequence<int, I...>) {
  return {{&launch_instance<I>...}};
}
constexpr auto kLaunchers = make_launchers(std::make_integer_sequence<int, kInstanceCount>{});

// the step kernel, or (accel) nbx_accel's slab form of it; timed = false: a launch the profile of the force kernel does not see
int enqueue_force(nbx_ctx* c, bool accel, double dt, bool timed = true) {
  if (c->plan.pairs) {  // this step's pair-interleaved copy of the records (all n_alloc of them: other ranks' blocks arrived by all-gather)
    const int npairs = c->n_alloc / 2;
    hipLaunchKernelGGL(pair_transpose_kernel, dim3(ceil_div(npairs, kBlock)), dim3(kBlock), 0, c->stream, (const float4*)c->posm[c->cur],
                       (float4*)c->posm_pairs, npairs);
  }
  // the force launch alone is timed, and the exact kernel (validation) is not
  return timed_launch(c, timed && c->plan.step.kind != INST_EXACT, [&] { (accel ? c->launch_accel : c->launch_step)(c, dt, accel ? 1 : 0); });
}

// energy partials one step of this context's shape writes: one per workgroup of the kernel that integrates
int step_ke_parts(const nbx_ctx* c) { return c->plan.epi != EPI_SLAB ? c->plan.grid_x : ceil_div(c->i_count, kBlock); }

// one local step: force (+ integrate) into the next buffer; does not swap
template <typename T>
int enqueue_step(nbx_ctx* c, double dt) {
  using T4 = typename V4<T>::type;
  int rc = enqueue_force(c, false, dt);
  if (rc) return rc;
  if (c->plan.epi != EPI_SLAB) {
    c->ke_parts = step_ke_parts(c);
  } else {
    const int blocks = step_ke_parts(c);
    hipLaunchKernelGGL((integrate_kernel<T>), dim3(blocks), dim3(kBlock), 0, c->stream,
                       (const T4*)c->posm[c->cur], (T4*)c->posm[c->cur ^ 1], (T4*)c->velm,
                       (const T4*)c->accp, c->plan.S, c->own_pad, c->i_begin, c->i_count, (T)dt, c->ke_part);
    HIP_TRY(hipGetLastError());
    c->ke_parts = blocks;
  }
  return NBX_OK;
}

int enqueue_step_any(nbx_ctx* c, double dt) {
  return c->precision == 32 ? enqueue_step<float>(c, dt) : enqueue_step<double>(c, dt);
}

// A window of `unit` (even) steps captured once per buffer parity and replayed: the two launches of a
// step cost ~3.5 us each from the host but ~1.5 us as graph nodes (MI355X_MICROARCH.md, rows
// 'boundary' / 'graph-replay-floor'), which is what bounds n <= 16k.
int graph_unit_exec(nbx_ctx* c, int unit, double dt, hipGraphExec_t* out) {
  for (auto& g : c->graphs)
    if (g.steps == unit && g.parity == c->cur && g.dt == dt) { *out = g.exec; return NBX_OK; }
  const int cur0 = c->cur;
  hipGraph_t graph = nullptr;
  HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  int rc = NBX_OK;
  for (int s = 0; s < unit && rc == NBX_OK; ++s) {
    rc = enqueue_step_any(c, dt);
    c->cur ^= 1;
  }
  c->cur = cur0;
  hipError_t e = hipStreamEndCapture(c->stream, &graph);
  if (rc != NBX_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (e != hipSuccess) return fail(NBX_ERR_DEVICE, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) return fail(NBX_ERR_DEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  c->graphs.push_back({unit, cur0, dt, exec});
  *out = exec;
  return NBX_OK;
}

}  // namespace

int nbx_detail::enqueue_ke_reduce(nbx_ctx* c, int slot) {
  hipLaunchKernelGGL(ke_reduce_kernel, dim3(1), dim3(kBlock), 0, c->stream, (const double*)c->ke_part,
                     c->ke_parts, c->ke_dev + slot);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}
// nbx_kick (nbx_kick.hip): the launch nbx_accel reads back -- the accelerations at posm[cur] into the S slabs of accp -- not timed
int nbx_detail::enqueue_accel_slabs(nbx_ctx* c) { return enqueue_force(c, true, 0.0, false); }
// nbx_tracers_step (nbx_tracers.hip): one turn of nbx_step's plain loop -- the step's own launches, then the buffer flip
int nbx_detail::enqueue_one_step(nbx_ctx* c, double dt) {
  const int rc = enqueue_step_any(c, dt);
  if (rc) return rc;
  c->cur ^= 1;
  c->steps_done += 1;
  return NBX_OK;
}
// the tuner's predictor: nbx_plan.hpp, force_cost
double nbx_detail::model_force_cost(const nbx_ctx* c, int own) { return force_cost(c->plan, c->precision, c->prop.multiProcessorCount, own); }

namespace {

template <typename T>
int upload_t(nbx_ctx* c, const T* px, const T* py, const T* pz, const T* vx, const T* vy, const T* vz,
             const T* m) {
  using T4 = typename V4<T>::type;
  std::vector<T4> hp((size_t)c->n_alloc);
  const T G = grav_const<T>();
  for (int i = 0; i < c->n; ++i) {
    T4 r; r.x = px[i]; r.y = py[i]; r.z = pz[i]; r.w = (G * m[i]) * gm_prescale<T>();
    hp[i] = r;
  }
  for (int i = c->n; i < c->n_alloc; ++i) { T4 z; z.x = z.y = z.z = z.w = (T)0; hp[i] = z; }
  std::vector<T4> hv((size_t)c->own_pad);
  for (int k = 0; k < c->own_pad; ++k) {
    T4 r; r.x = r.y = r.z = r.w = (T)0;
    if (k < c->i_count) { const int i = c->i_begin + k; r.x = vx[i]; r.y = vy[i]; r.z = vz[i]; r.w = m[i]; }
    hv[k] = r;
  }
  HIP_TRY(hipMemcpyAsync(c->posm[0], hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->posm[1], hp.data(), sizeof(T4) * hp.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->velm, hv.data(), sizeof(T4) * hv.size(), hipMemcpyHostToDevice, c->stream));
  if (c->mass_all) HIP_TRY(hipMemcpyAsync(c->mass_all, m, sizeof(T) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return NBX_OK;
}

template <typename T>
int download_t(nbx_ctx* c, T* px, T* py, T* pz, T* vx, T* vy, T* vz) {
  using T4 = typename V4<T>::type;
  if (px || py || pz) {
    std::vector<T4> hp((size_t)c->n);
    HIP_TRY(hipMemcpyAsync(hp.data(), c->posm[c->cur], sizeof(T4) * hp.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->n; ++i) {
      if (px) px[i] = hp[i].x;
      if (py) py[i] = hp[i].y;
      if (pz) pz[i] = hp[i].z;
    }
  }
  if (vx || vy || vz) {
    std::vector<T4> hv((size_t)c->i_count);
    HIP_TRY(hipMemcpyAsync(hv.data(), c->velm, sizeof(T4) * hv.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < c->i_count; ++k) {
      const int i = c->i_begin + k;
      if (vx) vx[i] = hv[k].x;
      if (vy) vy[i] = hv[k].y;
      if (vz) vz[i] = hv[k].z;
    }
  }
  return NBX_OK;
}

template <typename T>
int accel_t(nbx_ctx* c, T* ax, T* ay, T* az) {
  using T4 = typename V4<T>::type;
  int rc = enqueue_force(c, true, 0.0);
  if (rc) return rc;
  std::vector<T4> h((size_t)c->plan.S * c->own_pad);
  HIP_TRY(hipMemcpyAsync(h.data(), c->accp, sizeof(T4) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int k = 0; k < c->i_count; ++k) {
    T sx = (T)0, sy = (T)0, sz = (T)0;
    for (int s = 0; s < c->plan.S; ++s) {  // same order as integrate_kernel
      const T4& q = h[(size_t)s * c->own_pad + k];
      sx += q.x; sy += q.y; sz += q.z;
    }
    const int i = c->i_begin + k;
    if (ax) ax[i] = sx;
    if (ay) ay[i] = sy;
    if (az) az[i] = sz;
  }
  return NBX_OK;
}

}  // namespace

extern "C" {

const char* nbx_last_error(void) { return last_error().c_str(); }
int32_t nbx_abi_version(void) { return NBX_ABI_VERSION; }

int nbx_create(nbx_ctx** out, int32_t n, int32_t precision, const nbx_opts* opts) {
  constexpr const char* where = "nbx_create";
  return guarded(where, [&]() -> int {
  // n and precision are looked at before the options: the order the errors of a call that has several are reported in
  if (!out) return fail(NBX_ERR_ARG, "nbx_create: out is NULL");
  *out = nullptr;
  if (n <= 0) return fail(NBX_ERR_ARG, "nbx_create: n must be > 0");
  if (precision != 32 && precision != 64) return fail(NBX_ERR_ARG, "nbx_create: precision must be 32 or 64");
  nbx_opts o;
  int rc = create_opts(where, out, opts, &o);
  if (rc) return rc;
  if (o.i_begin < 0 || o.i_count < 0 || o.i_begin >= n || (long long)o.i_begin + o.i_count > n)
    return fail(NBX_ERR_ARG, "nbx_create: slice [i_begin, i_begin+i_count) is outside [0, n)");
  if (o.n_alloc != 0 && o.n_alloc < n) return fail(NBX_ERR_ARG, "nbx_create: n_alloc < n");

  BatchOwner<nbx_ctx> owner{nbx_destroy};  // every failure path below frees the context
  rc = batch_open(where, o, precision, &owner);
  if (rc) return rc;
  nbx_ctx* c = owner.o;
  c->n = n;
  c->i_begin = o.i_begin;
  c->i_count = o.i_count == 0 ? n - o.i_begin : o.i_count;
  c->n_alloc = round_up(std::max(n, o.n_alloc), kTile);
  c->own_pad = round_up(c->i_count, kBlock);
  const char* msg = nullptr;
  if (plan_launch({n, c->n_alloc, c->i_count, precision, c->prop.multiProcessorCount, c->own_stream}, o, &c->plan, &msg) != NBX_OK)
    return fail(NBX_ERR_ARG, msg);
  const int step_k = instance_index(c->plan.step), accel_k = instance_index(c->plan.accel);
  if (step_k < 0 || accel_k < 0) return fail(NBX_ERR_ARG, "no kernel instance for this bodies_per_lane / precision");
  c->launch_step = kLaunchers[step_k];
  c->launch_accel = kLaunchers[accel_k];
  c->slice_bit = kSliceBit;
  if (const char* e = getenv("NBX_SLICE_BIT")) {  // experiments: log2 of the slice length in 10 ns units
    const int k = atoi(e);
    if (k >= 4 && k <= 30) c->slice_bit = 1u << k;
  }

  // + spare records: the pipelined SGPR loop requests one batch past the last split (never used)
  const size_t pos_bytes = c->rec * (size_t)(c->n_alloc + kSgprOverread);
  CREATE_TRY(where, hipMalloc(&c->posm[0], pos_bytes));
  CREATE_TRY(where, hipMalloc(&c->posm[1], pos_bytes));
  CREATE_TRY(where, hipMalloc(&c->velm, c->rec * (size_t)c->own_pad));
  CREATE_TRY(where, hipMalloc(&c->accp, c->rec * (size_t)c->own_pad * c->plan.S));
  const int max_parts = std::max(ceil_div(c->i_count, kBlock), c->plan.grid_x);
  CREATE_TRY(where, hipMalloc(&c->ke_part, sizeof(double) * (size_t)max_parts));
  if (c->plan.variant == NBX_KERNEL_EXACT || c->plan.variant == NBX_KERNEL_EXACT_FMA) CREATE_TRY(where, hipMalloc(&c->mass_all, (c->rec / 4) * (size_t)c->n_alloc));
  if (c->plan.pairs) {  // same size and the same zero-filled spare records as posm
    CREATE_TRY(where, hipMalloc(&c->posm_pairs, pos_bytes));
    CREATE_TRY(where, hipMemsetAsync(c->posm_pairs, 0, pos_bytes, c->stream));
  }
  CREATE_TRY(where, hipMemsetAsync(c->posm[0], 0, pos_bytes, c->stream));
  CREATE_TRY(where, hipMemsetAsync(c->posm[1], 0, pos_bytes, c->stream));
  CREATE_TRY(where, hipMemsetAsync(c->ke_part, 0, sizeof(double) * (size_t)max_parts, c->stream));
  CREATE_TRY(where, hipStreamSynchronize(c->stream));
  rc = ensure_ke_cap(c, where, 64);
  if (rc) return rc;
  *out = owner.release();
  last_error().clear();
  return NBX_OK;
  });
}

void nbx_destroy(nbx_ctx* c) {
  if (!c) return;
  batch_quiesce(c);
  for (auto& g : c->graphs) (void)hipGraphExecDestroy(g.exec);
  for (void* p : {c->accp, c->mass_all, c->posm_pairs})
    if (p) (void)hipFree(p);
  batch_release(c);
  delete c;
}

int nbx_upload(nbx_ctx* c, const void* px, const void* py, const void* pz, const void* vx, const void* vy,
               const void* vz, const void* m) {
  return guarded("nbx_upload", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_upload: ctx is NULL");
  if (!px || !py || !pz || !vx || !vy || !vz || !m) return fail(NBX_ERR_ARG, "nbx_upload: NULL array");
  int rc = use_device(c);
  if (rc) return rc;
  rc = c->precision == 32
           ? upload_t<float>(c, (const float*)px, (const float*)py, (const float*)pz, (const float*)vx,
                             (const float*)vy, (const float*)vz, (const float*)m)
           : upload_t<double>(c, (const double*)px, (const double*)py, (const double*)pz, (const double*)vx,
                              (const double*)vy, (const double*)vz, (const double*)m);
  if (rc) return rc;
  c->cur = 0;
  c->uploaded = true;
  c->pending_commit = false;
  c->ke_parts = 0;  // the partials on the device belong to the previous trajectory
  return NBX_OK;
  });
}

static int step_common(nbx_ctx* c, double dt, int32_t nsteps, double* ke_last, double* ke_trace) {
  return guarded("nbx_step", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_step: ctx is NULL");
  if (nsteps < 0) return fail(NBX_ERR_ARG, "nbx_step: nsteps < 0");
  if (!std::isfinite(dt)) return fail(NBX_ERR_ARG, "nbx_step: dt is not finite");  // a NaN equals no cached graph's dt, itself included
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_step: nbx_upload has not been called");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_step: context owns a slice; use nbx_step_local + exchange + nbx_commit");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_step: a local step awaits nbx_commit");
  int rc = use_device(c);
  if (rc) return rc;
  if (ke_trace) {
    rc = ensure_ke_cap(c, "nbx_step", (size_t)std::max(nsteps, 1));
    if (rc) return rc;
  }
  int first = 0;
  if (c->plan.use_graph && !ke_trace && !c->profiling && nsteps >= 4) {
    const int unit = std::min(nsteps & ~1, 50);  // one replay costs the host 10-16 us: 50 steps per replay keeps that under 0.3 us per step
    hipGraphExec_t exec = nullptr;
    rc = graph_unit_exec(c, unit, dt, &exec);
    if (rc) return rc;
    while (nsteps - first >= unit) {  // an even unit leaves the buffer parity unchanged
      HIP_TRY(hipGraphLaunch(exec, c->stream));
      first += unit;
      c->steps_done += unit;
      c->graph_replays += 1;
      // a replay enqueues through the captured nodes, not through enqueue_step: say here how many energy partials its
      // last step leaves behind (nbx_upload zeroes the count; a cached graph must not leave it at zero)
      c->ke_parts = step_ke_parts(c);
    }
    if (first == nsteps && ke_last) {  // the partials of the last captured step are in ke_part
      rc = enqueue_ke_reduce(c, 0);
      if (rc) return rc;
    }
  }
  for (int s = first; s < nsteps; ++s) {
    rc = enqueue_step_any(c, dt);
    if (rc) return rc;
    c->cur ^= 1;
    c->steps_done += 1;
    if (ke_trace) {
      rc = enqueue_ke_reduce(c, s);
      if (rc) return rc;
    } else if (ke_last && s == nsteps - 1) {
      rc = enqueue_ke_reduce(c, 0);
      if (rc) return rc;
    }
  }
  return read_energies(c, 1, nsteps, c->ke_parts > 0, ke_last, ke_trace, [&] { return enqueue_ke_reduce(c, 0); });
  });
}

int nbx_step(nbx_ctx* c, double dt, int32_t nsteps, double* kenergy_out) {
  return step_common(c, dt, nsteps, kenergy_out, nullptr);
}

int nbx_step_trace(nbx_ctx* c, double dt, int32_t nsteps, double* ke_trace) {
  if (!ke_trace) return guarded("nbx_step_trace", [&]() -> int { return fail(NBX_ERR_ARG, "nbx_step_trace: ke_trace is NULL"); });
  return step_common(c, dt, nsteps, nullptr, ke_trace);
}

int nbx_step_local(nbx_ctx* c, double dt) {
  return guarded("nbx_step_local", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_step_local: ctx is NULL");
  if (!std::isfinite(dt)) return fail(NBX_ERR_ARG, "nbx_step_local: dt is not finite");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_step_local: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_step_local: previous step not committed");
  int rc = use_device(c);
  if (rc) return rc;
  rc = enqueue_step_any(c, dt);
  if (rc) return rc;
  c->pending_commit = true;
  return NBX_OK;
  });
}

int nbx_exchange_buffer(nbx_ctx* c, void** dev_ptr, size_t* total_bytes, size_t* own_offset_bytes, size_t* own_bytes) {
  return guarded("nbx_exchange_buffer", [&]() -> int {
  if (!c || !dev_ptr) return fail(NBX_ERR_ARG, "nbx_exchange_buffer: NULL argument");
  // the buffer the last local step wrote (NEXT while a commit is pending, else current)
  *dev_ptr = c->posm[c->pending_commit ? (c->cur ^ 1) : c->cur];
  if (total_bytes) *total_bytes = c->rec * (size_t)c->n_alloc;
  if (own_offset_bytes) *own_offset_bytes = c->rec * (size_t)c->i_begin;
  if (own_bytes) *own_bytes = c->rec * (size_t)c->i_count;
  return NBX_OK;
  });
}

int nbx_commit(nbx_ctx* c) {
  return guarded("nbx_commit", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_commit: ctx is NULL");
  if (!c->pending_commit) return fail(NBX_ERR_STATE, "nbx_commit: no local step pending");
  c->cur ^= 1;
  c->pending_commit = false;
  c->steps_done += 1;
  return NBX_OK;
  });
}

int nbx_kenergy_partial(nbx_ctx* c, double* sum_mv2) {
  return guarded("nbx_kenergy_partial", [&]() -> int {
  if (!c || !sum_mv2) return fail(NBX_ERR_ARG, "nbx_kenergy_partial: NULL argument");
  int rc = use_device(c);
  if (rc) return rc;
  if (c->ke_parts <= 0) {
    *sum_mv2 = 0.0;
    return NBX_OK;
  }
  rc = enqueue_ke_reduce(c, 0);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(sum_mv2, c->ke_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return NBX_OK;
  });
}

int nbx_accel(nbx_ctx* c, void* ax, void* ay, void* az) {
  return guarded("nbx_accel", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_accel: ctx is NULL");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_accel: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_accel: a local step awaits nbx_commit");
  int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? accel_t<float>(c, (float*)ax, (float*)ay, (float*)az)
                            : accel_t<double>(c, (double*)ax, (double*)ay, (double*)az);
  });
}

int nbx_sync(nbx_ctx* c) { return batch_sync(c, "nbx_sync"); }

int nbx_download(nbx_ctx* c, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return guarded("nbx_download", [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_download: ctx is NULL");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_download: nbx_upload has not been called");
  int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32
             ? download_t<float>(c, (float*)px, (float*)py, (float*)pz, (float*)vx, (float*)vy, (float*)vz)
             : download_t<double>(c, (double*)px, (double*)py, (double*)pz, (double*)vx, (double*)vy, (double*)vz);
  });
}

int nbx_profile(nbx_ctx* c, int32_t enable) { return batch_profile(c, "nbx_profile", enable); }

int nbx_stats(nbx_ctx* c, nbx_stats_t* s) {
  return guarded("nbx_stats", [&]() -> int {
  if (!c || !s) return fail(NBX_ERR_ARG, "nbx_stats: NULL argument");
  int rc = use_device(c);
  if (rc) return rc;
  if (c->ev_used) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = drain_profile(c);
    if (rc) return rc;
  }
  std::memset(s, 0, sizeof(*s));
  s->n = c->n; s->n_alloc = c->n_alloc; s->i_begin = c->i_begin; s->i_count = c->i_count;
  const nbx::Plan& p = c->plan;
  s->precision = c->precision; s->bodies_per_lane = p.B; s->j_split = p.S; s->j_tile = kTile;
  s->kernel_variant = p.variant; s->fused_epilogue = p.epi; s->summation_order = p.order;
  s->force_grid_x = p.grid_x; s->force_grid_y = p.grid_y; s->force_block = kBlock;
  s->cu_count = c->prop.multiProcessorCount; s->clock_mhz = c->prop.clockRate / 1000;
  s->steps_done = c->steps_done;
  s->force_launches_timed = c->launches_timed;
  s->force_ms_total = c->ms_total;
  s->pairs_per_launch = (double)c->i_count * (double)c->n;
  s->graph_replays = c->graph_replays;
  s->use_graph = p.use_graph ? 1 : 0;
  s->inner_loop = p.loop == LOOP_ASM_TS ? NBX_LOOP_ASM_TS : p.loop == LOOP_ASM_PF ? NBX_LOOP_ASM_PF : p.loop == LOOP_ASM ? NBX_LOOP_ASM : NBX_LOOP_CXX;
  // some boxes report an empty marketing name; fall back to / append the ISA name
  std::snprintf(s->device_name, sizeof(s->device_name), "%s%s%s", c->prop.name, c->prop.name[0] ? " " : "",
                c->prop.gcnArchName);
  return NBX_OK;
  });
}

}  // extern "C"

