// nbx_tracers.hip -- include/nbx_tracers.h over the kernels of nbx_tracers_kernels.hpp: m massless tracers per system, resident on
// the device, advanced with the bodies of a context, of every member of an ensemble or of every member of a ragged ensemble.
//
// A translation unit of its own: every other unit keeps its pinned kernel set.  One step is three things on the object's
// stream: the tracers' pair work at posm[cur] (launch shape field_shape(m, n), nbx_field_shape.hpp, the field's rule and nothing
// else), the tracers' update in place, and then the bodies' step through the hook its unit exposes -- enqueue_one_step
// (nbx_api.hip: enqueue_step_any and the cur flip) for a context, enqueue_step (nbx_batch.hpp) for the batch kinds -- so the
// body launches are the step's own and the tracers read the positions the bodies' force launch of that step reads.
//
// The buffers hang off Object (nbx_object.hpp): tr_pos and tr_vel, [systems][m] records {x, y, z, 0}; tr_part, the partial rows
// [systems][tr_rows][m] -- buffers of their own, NOT the field's scratch, so nbx_field between two steps disturbs nothing; tr_tab,
// a ragged ensemble's {pos_off, n} per member.  All are sized by the upload that fixes m: a step or a kick allocates nothing.
// The calls read posm[cur] and write the tr_* buffers: ke_part, have_parts, the profile and the cached graphs see only what the
// bodies' own step does to them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nbx_tracers.h"
#include "nbx_analysis.hpp"           // ensure_bytes, ragged_member_table
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, enqueue_step
#include "nbx_internal.hpp"           // struct nbx_ctx; enqueue_one_step, enqueue_ke_reduce
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged
#include "nbx_tracers_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// what the three kinds differ in
// ---------------------------------------------------------------------------------------------------------------------------
int systems(const nbx_ctx*) { return 1; }
int systems(const Batch* b) { return b->members; }
int bodies(const nbx_ctx* c, int) { return c->n; }
int bodies(const nbx_ensemble* e, int) { return e->n; }
int bodies(const nbx_ragged* r, int k) { return r->layout(k).n; }

int check_bodies(const nbx_ctx* c, const char* where) {
  if (!c->uploaded) return fail(NBX_ERR_STATE, std::string(where) + ": nbx_upload has not been called");
  return NBX_OK;
}
int check_bodies(const Batch* b, const char* where) { return check_uploaded(b, where, 0, b->members); }

// as nbx_step refuses them
int check_whole(const nbx_ctx* c, const char* where) {
  if (c->i_begin != 0 || c->i_count != c->n) return fail(NBX_ERR_STATE, std::string(where) + ": context owns a slice");
  if (c->pending_commit) return fail(NBX_ERR_STATE, std::string(where) + ": a local step awaits nbx_commit");
  return NBX_OK;
}
int check_whole(const Batch*, const char*) { return NBX_OK; }

// tracers of systems [first, first + count)
int check_tracers(const Object* o, const char* where, int first, int count, bool batch) {
  if (o->tr_m == 0) return fail(NBX_ERR_STATE, std::string(where) + ": no tracers have been uploaded");
  for (int k = first; k < first + count; ++k)
    if (!o->tr_have[(size_t)k])
      return fail(NBX_ERR_STATE, batch ? std::string(where) + ": member " + std::to_string(k) + " has no tracers"
                                       : std::string(where) + ": no tracers have been uploaded");
  return NBX_OK;
}

// the bodies' step, one turn of the kind's own loop
int body_step(nbx_ctx* c, double dt) { return enqueue_one_step(c, dt); }
template <typename O>
int body_step(O* o, double dt) {
  const int rc = enqueue_step(o, dt);
  if (rc) return rc;
  o->cur ^= 1;
  o->steps_done += 1;
  return NBX_OK;
}

bool have_parts(const nbx_ctx* c) { return c->ke_parts > 0; }
bool have_parts(const Batch* b) { return b->have_parts; }

int ensure_energy(nbx_ctx*, const char*) { return NBX_OK; }  // ke_dev holds at least one sum from nbx_create on
template <typename O>
int ensure_energy(O* o, const char* where) { return ensure_ke_cap(o, where, (size_t)o->members); }

// ---------------------------------------------------------------------------------------------------------------------------
// the pair work of all systems: one launch
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
void launch_pairs(nbx_ctx* c) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->tr_m, c->n);
  hipLaunchKernelGGL(tracer_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], c->n,
                     (const T4*)c->tr_pos, c->tr_m, s.tiles_per_split, (T4*)c->tr_part);
}

template <typename T>
void launch_pairs(nbx_ensemble* e) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->tr_m, e->n);
  EnsembleTracerArgs<T> k{};
  k.posm = (const T4*)e->posm[e->cur];
  k.trp = (const T4*)e->tr_pos;
  k.parts = (T4*)e->tr_part;
  k.pos_stride = (unsigned)e->pos_stride;
  k.n = e->n;
  k.m = e->tr_m;
  k.tiles_per_split = s.tiles_per_split;
  hipLaunchKernelGGL(ensemble_tracer_kernel<T>, dim3(s.columns, s.splits, e->members), dim3(kBlock), 0, e->stream, k);
}

// the grid's y extent is the largest number of splits any member has (tr_rows); a member's workgroups beyond its own return at once
template <typename T>
void launch_pairs(nbx_ragged* r) {
  using T4 = typename V4<T>::type;
  RaggedTracerArgs<T> k{};
  k.posm = (const T4*)r->posm[r->cur];
  k.table = (const TracerMember*)r->tr_tab;
  k.trp = (const T4*)r->tr_pos;
  k.parts = (T4*)r->tr_part;
  k.m = r->tr_m;
  hipLaunchKernelGGL(ragged_tracer_kernel<T>, dim3(field_shape(r->tr_m, 1).columns, r->tr_rows, r->members), dim3(kBlock), 0, r->stream, k);
}

// pair work and update of every tracer of the object: two launches, no allocation, outside the profile
template <typename T, bool KICK, typename O>
int enqueue_tracers(O* o, double h) {
  using T4 = typename V4<T>::type;
  launch_pairs<T>(o);
  HIP_TRY(hipGetLastError());
  const unsigned total = (unsigned)((size_t)systems(o) * (size_t)o->tr_m);
  hipLaunchKernelGGL((tracer_update_kernel<T, KICK>), dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, o->stream,
                     (const T4*)o->tr_part, (const TracerMember*)o->tr_tab, bodies(o, 0), o->tr_m, o->tr_rows, total, (T)h,
                     (T4*)o->tr_pos, (T4*)o->tr_vel);
  HIP_TRY(hipGetLastError());
  return NBX_OK;
}

template <bool KICK, typename O>
int enqueue_tracers_any(O* o, double h) {
  return o->precision == 32 ? enqueue_tracers<float, KICK>(o, h) : enqueue_tracers<double, KICK>(o, h);
}

// ---------------------------------------------------------------------------------------------------------------------------
// buffers
// ---------------------------------------------------------------------------------------------------------------------------
int ensure_table(nbx_ctx*, const char*, std::vector<TracerMember>*) { return NBX_OK; }
int ensure_table(nbx_ensemble*, const char*, std::vector<TracerMember>*) { return NBX_OK; }
// `table` lives until the caller has synchronised
int ensure_table(nbx_ragged* r, const char* where, std::vector<TracerMember>* table) {
  return ragged_member_table<TracerMember>(r, &r->tr_tab, table, where, [](const MemberSpan& mem, unsigned long long) {
    return TracerMember{{(unsigned long long)mem.pos_off, mem.n, 0}};
  });
}

void forget(Object* o) {
  o->tr_m = 0;
  o->tr_have.clear();
}

// a new set of m tracers per system: the buffers for all systems, no system's tracers there yet
template <typename O>
int begin_set(O* o, const char* where, int m, std::vector<TracerMember>* table) {
  const int S = systems(o);
  forget(o);
  int rows = 1;
  for (int k = 0; k < S; ++k) rows = std::max(rows, field_shape(m, bodies(o, k)).splits);
  const size_t total = (size_t)S * (size_t)m;
  std::vector<char> have((size_t)S, 0);
  int rc = ensure_bytes(&o->tr_pos, &o->tr_pos_cap, o->rec * total, where, "the tracer positions");
  if (rc) return rc;
  rc = ensure_bytes(&o->tr_vel, &o->tr_vel_cap, o->rec * total, where, "the tracer velocities");
  if (rc) return rc;
  rc = ensure_bytes(&o->tr_part, &o->tr_part_cap, o->rec * total * (size_t)rows, where, "the partials");
  if (rc) return rc;
  rc = ensure_table(o, where, table);
  if (rc) return rc;
  o->tr_have.swap(have);
  o->tr_m = m;
  o->tr_rows = rows;
  return NBX_OK;
}

struct In { const void *px, *py, *pz, *vx, *vy, *vz; };
struct Out { void *px, *py, *pz, *vx, *vy, *vz; };

template <typename T>
int upload_t(Object* o, int first, int count, const In& a) {
  using T4 = typename V4<T>::type;
  const size_t m = (size_t)o->tr_m, total = (size_t)count * m, at = sizeof(T4) * (size_t)first * m;
  std::vector<T4> hp(total), hv(total);
  const T *px = (const T*)a.px, *py = (const T*)a.py, *pz = (const T*)a.pz, *vx = (const T*)a.vx, *vy = (const T*)a.vy, *vz = (const T*)a.vz;
  for (size_t i = 0; i < total; ++i) {
    T4 q; q.x = px[i]; q.y = py[i]; q.z = pz[i]; q.w = (T)0;
    hp[i] = q;
    T4 u; u.x = vx[i]; u.y = vy[i]; u.z = vz[i]; u.w = (T)0;  // no mass: the update's energy term is nothing
    hv[i] = u;
  }
  HIP_TRY(hipMemcpyAsync((char*)o->tr_pos + at, hp.data(), sizeof(T4) * total, hipMemcpyHostToDevice, o->stream));
  HIP_TRY(hipMemcpyAsync((char*)o->tr_vel + at, hv.data(), sizeof(T4) * total, hipMemcpyHostToDevice, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  return NBX_OK;
}

template <typename T>
int download_t(Object* o, int first, int count, const Out& a) {
  using T4 = typename V4<T>::type;
  const size_t m = (size_t)o->tr_m, total = (size_t)count * m, at = sizeof(T4) * (size_t)first * m;
  const bool pos = a.px || a.py || a.pz, vel = a.vx || a.vy || a.vz;
  std::vector<T4> hp(pos ? total : 0), hv(vel ? total : 0);
  if (pos) HIP_TRY(hipMemcpyAsync(hp.data(), (const char*)o->tr_pos + at, sizeof(T4) * total, hipMemcpyDeviceToHost, o->stream));
  if (vel) HIP_TRY(hipMemcpyAsync(hv.data(), (const char*)o->tr_vel + at, sizeof(T4) * total, hipMemcpyDeviceToHost, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  T *px = (T*)a.px, *py = (T*)a.py, *pz = (T*)a.pz, *vx = (T*)a.vx, *vy = (T*)a.vy, *vz = (T*)a.vz;
  for (size_t i = 0; i < total; ++i) {
    if (px) px[i] = hp[i].x;
    if (py) py[i] = hp[i].y;
    if (pz) pz[i] = hp[i].z;
    if (vx) vx[i] = hv[i].x;
    if (vy) vy[i] = hv[i].y;
    if (vz) vz[i] = hv[i].z;
  }
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the entry points of the three kinds: every check before the first HIP call, in the header's order.  A context is the range
// (0, 1) of one system.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename O>
constexpr bool is_batch = !std::is_same<O, nbx_ctx>::value;

int check_members(const nbx_ctx*, const char*, int, int) { return NBX_OK; }
int check_members(const Batch* b, const char* where, int first, int count) { return check_range(b, where, first, count); }

template <typename O>
int tracers_upload(O* o, const char* where, int32_t first, int32_t count, int32_t m, const In& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (m < 0) return fail(NBX_ERR_ARG, std::string(where) + ": m < 0");
  if (m > 0 && (!a.px || !a.py || !a.pz || !a.vx || !a.vy || !a.vz)) return fail(NBX_ERR_ARG, std::string(where) + ": NULL array");
  int rc = check_members(o, where, first, count);
  if (rc) return rc;
  const int S = systems(o);
  if ((long long)S * m > kFieldMaxPoints)
    return fail(NBX_ERR_ARG, std::string(where) + (is_batch<O> ? ": members * m exceeds 4194304" : ": m exceeds 4194304"));
  const bool all = first == 0 && count == S;
  if (m != o->tr_m && o->tr_m != 0 && !all)
    return fail(NBX_ERR_ARG, std::string(where) + ": m differs from the object's " + std::to_string(o->tr_m) +
                                 " tracers per member and the range does not cover all members");
  if (m == 0) {  // removes the set (all members, or there is none); the buffers stay
    if (all || o->tr_m == 0) forget(o);
    return NBX_OK;
  }
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  std::vector<TracerMember> table;  // lives until upload_t has synchronised
  if (m != o->tr_m) {
    rc = begin_set(o, where, m, &table);
    if (rc) {
      (void)hipStreamSynchronize(o->stream);  // no copy may outlive `table`
      return rc;
    }
  }
  rc = o->precision == 32 ? upload_t<float>(o, first, count, a) : upload_t<double>(o, first, count, a);
  if (rc) {
    (void)hipStreamSynchronize(o->stream);
    return rc;
  }
  for (int k = first; k < first + count; ++k) o->tr_have[(size_t)k] = 1;
  return NBX_OK;
  });
}

template <typename O>
int tracers_download(O* o, const char* where, int32_t first, int32_t count, const Out& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_members(o, where, first, count);
  if (rc) return rc;
  rc = check_tracers(o, where, first, count, is_batch<O>);
  if (rc) return rc;
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? download_t<float>(o, first, count, a) : download_t<double>(o, first, count, a);
  });
}

template <typename O>
int tracers_count(O* o, const char* where, int32_t* m) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!m) return fail(NBX_ERR_ARG, std::string(where) + ": m is NULL");
  *m = o->tr_m;
  return NBX_OK;
  });
}

template <typename O>
int tracers_step(O* o, const char* where, double dt, int32_t nsteps, double* ke_out) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (nsteps < 0) return fail(NBX_ERR_ARG, std::string(where) + ": nsteps < 0");
  if (!std::isfinite(dt)) return fail(NBX_ERR_ARG, std::string(where) + ": dt is not finite");
  int rc = check_bodies(o, where);
  if (rc) return rc;
  rc = check_tracers(o, where, 0, systems(o), is_batch<O>);
  if (rc) return rc;
  rc = check_whole(o, where);
  if (rc) return rc;
  rc = use_device(o);
  if (rc) return rc;
  if (ke_out) {
    rc = ensure_energy(o, where);
    if (rc) return rc;
  }
  for (int s = 0; s < nsteps; ++s) {
    rc = enqueue_tracers_any<false>(o, dt);  // at posm[cur]: the positions the bodies' force launch of this step reads
    if (rc) return rc;
    rc = body_step(o, dt);
    if (rc) return rc;
    if (ke_out && s == nsteps - 1) {
      rc = enqueue_ke_reduce(o, 0);
      if (rc) return rc;
    }
  }
  return read_energies(o, (size_t)systems(o), nsteps, have_parts(o), ke_out, nullptr, [&] { return enqueue_ke_reduce(o, 0); });
  });
}

template <typename O>
int tracers_kick(O* o, const char* where, double h) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!std::isfinite(h)) return fail(NBX_ERR_ARG, std::string(where) + ": h is not finite");
  int rc = check_bodies(o, where);
  if (rc) return rc;
  rc = check_tracers(o, where, 0, systems(o), is_batch<O>);
  if (rc) return rc;
  rc = check_whole(o, where);
  if (rc) return rc;
  rc = use_device(o);
  if (rc) return rc;
  return enqueue_tracers_any<true>(o, h);
  });
}

}  // namespace

extern "C" {

int nbx_tracers_upload(nbx_ctx* c, int32_t m, const void* px, const void* py, const void* pz, const void* vx, const void* vy, const void* vz) {
  return tracers_upload(c, "nbx_tracers_upload", 0, 1, m, In{px, py, pz, vx, vy, vz});
}
int nbx_tracers_download(nbx_ctx* c, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return tracers_download(c, "nbx_tracers_download", 0, 1, Out{px, py, pz, vx, vy, vz});
}
int nbx_tracers_count(nbx_ctx* c, int32_t* m) { return tracers_count(c, "nbx_tracers_count", m); }
int nbx_tracers_step(nbx_ctx* c, double dt, int32_t nsteps, double* kenergy_out) {
  return tracers_step(c, "nbx_tracers_step", dt, nsteps, kenergy_out);
}
int nbx_tracers_kick(nbx_ctx* c, double h) { return tracers_kick(c, "nbx_tracers_kick", h); }

int nbx_ensemble_tracers_upload(nbx_ensemble* e, int32_t first, int32_t count, int32_t m, const void* px, const void* py, const void* pz,
                                const void* vx, const void* vy, const void* vz) {
  return tracers_upload(e, "nbx_ensemble_tracers_upload", first, count, m, In{px, py, pz, vx, vy, vz});
}
int nbx_ensemble_tracers_download(nbx_ensemble* e, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return tracers_download(e, "nbx_ensemble_tracers_download", first, count, Out{px, py, pz, vx, vy, vz});
}
int nbx_ensemble_tracers_count(nbx_ensemble* e, int32_t* m) { return tracers_count(e, "nbx_ensemble_tracers_count", m); }
int nbx_ensemble_tracers_step(nbx_ensemble* e, double dt, int32_t nsteps, double* kenergy_out) {
  return tracers_step(e, "nbx_ensemble_tracers_step", dt, nsteps, kenergy_out);
}
int nbx_ensemble_tracers_kick(nbx_ensemble* e, double h) { return tracers_kick(e, "nbx_ensemble_tracers_kick", h); }

int nbx_ragged_tracers_upload(nbx_ragged* r, int32_t first, int32_t count, int32_t m, const void* px, const void* py, const void* pz,
                              const void* vx, const void* vy, const void* vz) {
  return tracers_upload(r, "nbx_ragged_tracers_upload", first, count, m, In{px, py, pz, vx, vy, vz});
}
int nbx_ragged_tracers_download(nbx_ragged* r, int32_t first, int32_t count, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return tracers_download(r, "nbx_ragged_tracers_download", first, count, Out{px, py, pz, vx, vy, vz});
}
int nbx_ragged_tracers_count(nbx_ragged* r, int32_t* m) { return tracers_count(r, "nbx_ragged_tracers_count", m); }
int nbx_ragged_tracers_step(nbx_ragged* r, double dt, int32_t nsteps, double* kenergy_out) {
  return tracers_step(r, "nbx_ragged_tracers_step", dt, nsteps, kenergy_out);
}
int nbx_ragged_tracers_kick(nbx_ragged* r, double h) { return tracers_kick(r, "nbx_ragged_tracers_kick", h); }

}  // extern "C"
