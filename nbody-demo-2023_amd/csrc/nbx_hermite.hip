// nbx_hermite.hip -- nbx_hermite_step, nbx_ensemble_hermite_step and nbx_ragged_hermite_step (include/nbx_hermite.h) over the
// kernels of nbx_hermite_kernels.hpp: fourth-order Hermite P(EC) steps of every body of a context, or of every member of a batch
// object, two launches a step, nothing read back and no synchronisation.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp), as for the acceleration's time derivative:
// the host evaluates it for a context and an ensemble, the device for every member of a ragged ensemble.  A call reads and
// writes posm[cur] and velm in place and keeps herm_part and herm_keep, buffers of its own: cur, steps_done, the profile, the
// cached graphs, the tracers and every analysis call's scratch do not see it.  The kinetic-energy partials belong to no state
// afterwards, as after an upload.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nbx_hermite.h"
#include "nbx_analysis.hpp"           // object_bodies, bodies_noun, ragged_member_table, ragged_extents
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_uploaded
#include "nbx_hermite_kernels.hpp"
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

// what a kind's launch is told besides its own layout
template <typename T>
struct PairLaunch {
  typename V4<T>::type* parts;
  const typename V4<T>::type* keep;
  int predict;
  HermiteConsts hc;
};

// the kinetic-energy partials: do any exist, and "none belong to this state" (as after an upload)
bool has_partials(const nbx_ctx* c) { return c->ke_parts > 0; }
bool has_partials(const Batch* b) { return b->have_parts; }
void drop_partials(nbx_ctx* c) { c->ke_parts = 0; }
void drop_partials(Batch* b) { b->have_parts = false; }

// status 8: what the library can see of the caller's promise
template <typename O>
int check_resume(const O* o, const char* where) {
  if (!o->herm_have) return fail(NBX_ERR_STATE, std::string(where) + ": resume without a previous Hermite call on this object");
  if (o->herm_steps != o->steps_done || o->herm_cur != o->cur)
    return fail(NBX_ERR_STATE, std::string(where) + ": resume after a step (steps_done or the current position buffer is not what the previous Hermite call left)");
  if (has_partials(o))
    return fail(NBX_ERR_STATE, std::string(where) + ": resume after a step or a kick (kinetic-energy partials have been written since the previous Hermite call)");
  return NBX_OK;
}

// What the three kinds share once the checks are through.  total: the bodies of the object; vel_records: the records of velm;
// `fin`: the finish launch's layout (parts, keep, correct and the constants are filled in here); `launch(PairLaunch)`: the
// kind's pair work over `row_splits` rows per member.
template <typename T, typename O, typename Launch>
int run_hermite(O* o, const char* where, size_t total, int row_splits, size_t vel_records, double dt, int nsteps, int resume,
                HermiteFinishArgs<T> fin, Launch launch) {
  using T4 = typename V4<T>::type;
  if (!o->herm_part) {
    char* dev = nullptr;
    const int rc = device_alloc(&dev, sizeof(T4) * 2 * total * (size_t)row_splits, where, "the partials");
    if (rc) return rc;
    o->herm_part = dev;
  }
  if (!o->herm_keep) {
    char* dev = nullptr;
    const int rc = device_alloc(&dev, sizeof(T4) * 2 * vel_records, where, "the kept records");
    if (rc) return rc;
    o->herm_keep = dev;
  }
  HermiteConsts hc;
  hc.h = (double)(T)dt;  // rounded once to T, widened
  hc.k2 = hc.h * 0.5;
  hc.k6 = hc.h / 6.0;
  hc.h3 = hc.h / 3.0;
  fin.parts = (const T4*)o->herm_part;
  fin.keep = (T4*)o->herm_keep;
  fin.posm = (T4*)o->posm[o->cur];
  fin.velm = (T4*)o->velm;
  fin.row_splits = row_splits;
  fin.total = (unsigned)total;
  fin.hc = hc;
  o->herm_have = false;  // until every launch of this call has been enqueued
  for (int s = resume ? 0 : -1; s < nsteps; ++s) {  // -1: the evaluation at the resident state, the same two launches
    const int moving = s >= 0;
    launch(PairLaunch<T>{(T4*)o->herm_part, (const T4*)o->herm_keep, moving, hc});
    HIP_TRY(hipGetLastError());
    fin.correct = moving;
    hipLaunchKernelGGL(hermite_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream, fin);
    HIP_TRY(hipGetLastError());
  }
  drop_partials(o);
  o->herm_have = true;
  o->herm_steps = o->steps_done;
  o->herm_cur = o->cur;
  return NBX_OK;
}

template <typename T>
int hermite_t(nbx_ctx* c, const char* where, double dt, int nsteps, int resume) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  HermiteFinishArgs<T> fin{};
  fin.table = nullptr;
  fin.members = 1;
  fin.n_all = c->n;
  return run_hermite<T>(c, where, (size_t)c->n, s.splits, (size_t)c->own_pad, dt, nsteps, resume, fin, [&](const PairLaunch<T>& p) {
    HermiteArgs<T> a{};
    a.posm = (const T4*)c->posm[c->cur];
    a.velm = (const T4*)c->velm;
    a.keep = p.keep;
    a.parts = p.parts;
    a.n = c->n;
    a.tiles_per_split = s.tiles_per_split;
    a.predict = p.predict;
    a.hc = p.hc;
    hipLaunchKernelGGL(hermite_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, a);
  });
}

template <typename T>
int hermite_t(nbx_ensemble* e, const char* where, double dt, int nsteps, int resume) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  HermiteFinishArgs<T> fin{};
  fin.table = nullptr;
  fin.members = e->members;
  fin.n_all = e->n;
  fin.pos_stride = (unsigned)e->pos_stride;
  fin.vel_stride = (unsigned)e->own_pad;
  return run_hermite<T>(e, where, (size_t)e->members * (size_t)e->n, s.splits, (size_t)e->members * (size_t)e->own_pad, dt, nsteps, resume, fin,
                        [&](const PairLaunch<T>& p) {
    EnsembleHermiteArgs<T> k{};
    k.member0.posm = (const T4*)e->posm[e->cur];
    k.member0.velm = (const T4*)e->velm;
    k.member0.keep = p.keep;
    k.member0.parts = p.parts;
    k.member0.n = e->n;
    k.member0.tiles_per_split = s.tiles_per_split;
    k.member0.predict = p.predict;
    k.member0.hc = p.hc;
    k.pos_stride = (unsigned)e->pos_stride;
    k.vel_stride = (unsigned)e->own_pad;
    hipLaunchKernelGGL(ensemble_hermite_kernel<T>, dim3(s.columns, s.splits, e->members), dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member has, a member's workgroups beyond its own return at once.
template <typename T>
int hermite_t(nbx_ragged* r, const char* where, double dt, int nsteps, int resume) {
  using T4 = typename V4<T>::type;
  // the copy's source, herm_tab_src, lives with the object: nothing here waits for it
  const int rc = ragged_member_table<HermiteMember>(r, &r->herm_tab, &r->herm_tab_src, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return HermiteMember{{(unsigned long long)mem.pos_off, (unsigned long long)mem.vel_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, 0, r->members);
  const HermiteMember* dev = (const HermiteMember*)r->herm_tab;
  HermiteFinishArgs<T> fin{};
  fin.table = dev;
  fin.members = r->members;
  return run_hermite<T>(r, where, (size_t)object_bodies(r), g.splits, span_of(r, 0, r->members).vel_count, dt, nsteps, resume, fin, [&](const PairLaunch<T>& p) {
    RaggedHermiteArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.velm = (const T4*)r->velm;
    k.keep = p.keep;
    k.table = dev;
    k.parts = p.parts;
    k.predict = p.predict;
    k.hc = p.hc;
    hipLaunchKernelGGL(ragged_hermite_kernel<T>, dim3(g.columns, g.splits, r->members), dim3(kBlock), 0, r->stream, k);
  });
}

// dt as the object's precision holds it: a double that rounds to an infinite float is not a time step either
bool dt_finite(int precision, double dt) { return std::isfinite(dt) && (precision != 32 || std::isfinite((float)dt)); }

// nbx_ensemble_hermite_step and nbx_ragged_hermite_step: every check before the first HIP call, in the header's order
template <typename O>
int batch_hermite(O* o, const char* where, double dt, int32_t nsteps, int32_t resume) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!dt_finite(o->precision, dt)) return fail(NBX_ERR_ARG, std::string(where) + ": dt is not finite");
  if (nsteps < 0) return fail(NBX_ERR_ARG, std::string(where) + ": nsteps < 0");
  if (object_bodies(o) > kHermiteMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + bodies_noun(o) + " 4194304");
  int rc = check_uploaded(o, where, 0, o->members);
  if (rc) return rc;
  if (resume) {
    rc = check_resume(o, where);
    if (rc) return rc;
  }
  if (nsteps == 0 || o->members == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? hermite_t<float>(o, where, dt, nsteps, resume) : hermite_t<double>(o, where, dt, nsteps, resume);
  });
}

}  // namespace

extern "C" {

int nbx_hermite_step(nbx_ctx* c, double dt, int32_t nsteps, int32_t resume) {
  constexpr const char* where = "nbx_hermite_step";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_hermite_step: ctx is NULL");
  if (!dt_finite(c->precision, dt)) return fail(NBX_ERR_ARG, "nbx_hermite_step: dt is not finite");
  if (nsteps < 0) return fail(NBX_ERR_ARG, "nbx_hermite_step: nsteps < 0");
  if ((long long)c->n > kHermiteMaxBodies) return fail(NBX_ERR_ARG, "nbx_hermite_step: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_hermite_step: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_hermite_step: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_hermite_step: the context owns a slice of the bodies (the velocities of the others are not resident)");
  if (resume) {
    const int rc = check_resume(c, where);
    if (rc) return rc;
  }
  if (nsteps == 0) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? hermite_t<float>(c, where, dt, nsteps, resume) : hermite_t<double>(c, where, dt, nsteps, resume);
  });
}

int nbx_ensemble_hermite_step(nbx_ensemble* e, double dt, int32_t nsteps, int32_t resume) {
  return batch_hermite(e, "nbx_ensemble_hermite_step", dt, nsteps, resume);
}

int nbx_ragged_hermite_step(nbx_ragged* r, double dt, int32_t nsteps, int32_t resume) {
  return batch_hermite(r, "nbx_ragged_hermite_step", dt, nsteps, resume);
}

}  // extern "C"
