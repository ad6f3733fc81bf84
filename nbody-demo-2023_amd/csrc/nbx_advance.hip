// nbx_advance.hip -- nbx_advance, nbx_ensemble_advance and nbx_ragged_advance, and nbx_clock, nbx_ensemble_clock and
// nbx_ragged_clock (include/nbx_advance.h) over the kernels of nbx_advance_kernels.hpp: fourth-order Hermite P(EC) steps whose
// size every system chooses for itself on the device, three launches a step, nothing read back and no synchronisation; the clock
// calls read the systems' clock records back, one synchronisation each.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp), as for the fixed stepper.  A call reads and
// writes posm[cur] and velm in place, shares herm_part, herm_keep and herm_tab with the fixed stepper (the same sizes and
// layout; whichever call comes first makes them) and keeps adv_cand and adv_clock, buffers of its own: cur, steps_done, the
// profile, the cached graphs, the tracers and every analysis call's scratch do not see it.  The kinetic-energy partials belong to
// no state afterwards, as after an upload.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nbx_advance.h"
#include "nbx_analysis.hpp"           // object_bodies, bodies_noun, ragged_member_table, ragged_extents
#include "nbx_advance_kernels.hpp"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

static_assert(sizeof(AdvanceClock) == 80, "the clock record is read back whole");

// the arguments of an advance call once checked
struct AdvancePlan {
  double t_end, dt_cap, eta2;
  int k_cap, levels, max_steps, resume;
};

// what a kind's launch is told besides its own layout
template <typename T>
struct PairLaunch {
  typename V4<T>::type* parts;
  const typename V4<T>::type* keep;
  int predict;
  AdvanceTime tm;
};

// the kinetic-energy partials: do any exist, and "none belong to this state" (as after an upload)
bool has_partials(const nbx_ctx* c) { return c->ke_parts > 0; }
bool has_partials(const Batch* b) { return b->have_parts; }
void drop_partials(nbx_ctx* c) { c->ke_parts = 0; }
void drop_partials(Batch* b) { b->have_parts = false; }

// status 10: what the library can see of the caller's promise
template <typename O>
int check_resume(const O* o, const char* where, const AdvancePlan& p) {
  if (!o->adv_have) return fail(NBX_ERR_STATE, std::string(where) + ": resume without a previous advance call on this object");
  if (o->herm_have)
    return fail(NBX_ERR_STATE, std::string(where) + ": resume after a fixed Hermite step (the kept records are no longer what the previous advance call left)");
  if (o->adv_steps != o->steps_done || o->adv_cur != o->cur)
    return fail(NBX_ERR_STATE, std::string(where) + ": resume after a step (steps_done or the current position buffer is not what the previous advance call left)");
  if (has_partials(o))
    return fail(NBX_ERR_STATE, std::string(where) + ": resume after a step or a kick (kinetic-energy partials have been written since the previous advance call)");
  if (o->adv_dt_cap != p.dt_cap || o->adv_levels != p.levels)
    return fail(NBX_ERR_STATE, std::string(where) + ": resume with another dt_cap or levels than the previous advance call's");
  return NBX_OK;
}

// What the three kinds share once the checks are through.  total: the bodies of the object; systems: its clock records;
// vel_records: the records of velm; `fin` and `clk`: the finish and the clock launch's layout (the buffers, the flags and the
// time are filled in here); `launch(PairLaunch)`: the kind's pair work over `row_splits` rows per member.
template <typename T, typename O, typename Launch>
int run_advance(O* o, const char* where, size_t total, size_t systems, int row_splits, size_t vel_records, const AdvancePlan& p,
                AdvanceFinishArgs<T> fin, AdvanceClockArgs clk, Launch launch) {
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
  if (!o->adv_cand) {
    double* dev = nullptr;
    const int rc = device_alloc(&dev, total, where, "the candidates");
    if (rc) return rc;
    o->adv_cand = dev;
  }
  if (!o->adv_clock) {
    AdvanceClock* dev = nullptr;
    const int rc = device_alloc(&dev, systems, where, "the clock records");
    if (rc) return rc;
    o->adv_clock = dev;
  }
  const AdvanceTime tm{(const AdvanceClock*)o->adv_clock, p.t_end};
  fin.parts = (const T4*)o->herm_part;
  fin.keep = (T4*)o->herm_keep;
  fin.posm = (T4*)o->posm[o->cur];
  fin.velm = (T4*)o->velm;
  fin.cand = (double*)o->adv_cand;
  fin.row_splits = row_splits;
  fin.total = (unsigned)total;
  fin.tm = tm;
  clk.cand = (const double*)o->adv_cand;
  clk.clocks = (AdvanceClock*)o->adv_clock;
  clk.t_end = p.t_end;
  clk.eta2 = p.eta2;
  clk.dt_cap = p.dt_cap;
  clk.inv_cap = 1.0 / p.dt_cap;  // exact: a power of two
  clk.k_cap = p.k_cap;
  clk.levels = p.levels;
  o->adv_have = false;   // until every launch of this call has been enqueued
  o->herm_have = false;  // the kept records are an advance call's from here on
  for (int s = p.resume ? 0 : -1; s < p.max_steps; ++s) {  // -1: the evaluation at the resident state, the same three launches
    const int moving = s >= 0;
    launch(PairLaunch<T>{(T4*)o->herm_part, (const T4*)o->herm_keep, moving, tm});
    HIP_TRY(hipGetLastError());
    fin.correct = moving;
    hipLaunchKernelGGL(advance_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream, fin);
    HIP_TRY(hipGetLastError());
    clk.start = !moving;
    hipLaunchKernelGGL(advance_clock_kernel, dim3((unsigned)systems), dim3(kBlock), 0, o->stream, clk);
    HIP_TRY(hipGetLastError());
  }
  drop_partials(o);
  o->adv_have = true;
  o->adv_steps = o->steps_done;
  o->adv_cur = o->cur;
  o->adv_dt_cap = p.dt_cap;
  o->adv_levels = p.levels;
  o->adv_t_end = p.t_end;
  return NBX_OK;
}

template <typename T>
int advance_t(nbx_ctx* c, const char* where, const AdvancePlan& p) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  AdvanceFinishArgs<T> fin{};
  fin.table = nullptr;
  fin.members = 1;
  fin.n_all = c->n;
  AdvanceClockArgs clk{};
  clk.table = nullptr;
  clk.n_all = c->n;
  return run_advance<T>(c, where, (size_t)c->n, 1, s.splits, (size_t)c->own_pad, p, fin, clk, [&](const PairLaunch<T>& l) {
    AdvanceArgs<T> a{};
    a.posm = (const T4*)c->posm[c->cur];
    a.velm = (const T4*)c->velm;
    a.keep = l.keep;
    a.parts = l.parts;
    a.n = c->n;
    a.tiles_per_split = s.tiles_per_split;
    a.predict = l.predict;
    a.tm = l.tm;
    hipLaunchKernelGGL(advance_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, a);
  });
}

template <typename T>
int advance_t(nbx_ensemble* e, const char* where, const AdvancePlan& p) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  AdvanceFinishArgs<T> fin{};
  fin.table = nullptr;
  fin.members = e->members;
  fin.n_all = e->n;
  fin.pos_stride = (unsigned)e->pos_stride;
  fin.vel_stride = (unsigned)e->own_pad;
  AdvanceClockArgs clk{};
  clk.table = nullptr;
  clk.n_all = e->n;
  return run_advance<T>(e, where, (size_t)e->members * (size_t)e->n, (size_t)e->members, s.splits, (size_t)e->members * (size_t)e->own_pad, p, fin,
                        clk, [&](const PairLaunch<T>& l) {
    EnsembleAdvanceArgs<T> k{};
    k.member0.posm = (const T4*)e->posm[e->cur];
    k.member0.velm = (const T4*)e->velm;
    k.member0.keep = l.keep;
    k.member0.parts = l.parts;
    k.member0.n = e->n;
    k.member0.tiles_per_split = s.tiles_per_split;
    k.member0.predict = l.predict;
    k.member0.tm = l.tm;
    k.pos_stride = (unsigned)e->pos_stride;
    k.vel_stride = (unsigned)e->own_pad;
    hipLaunchKernelGGL(ensemble_advance_kernel<T>, dim3(s.columns, s.splits, e->members), dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is the fixed stepper's: built and put on the device by whichever call comes first; the grid's x and y extents
// are the largest number of columns and of splits any member has, a member's workgroups beyond its own return at once.
template <typename T>
int advance_t(nbx_ragged* r, const char* where, const AdvancePlan& p) {
  using T4 = typename V4<T>::type;
  // the copy's source, herm_tab_src, lives with the object: nothing here waits for it
  const int rc = ragged_member_table<AdvanceMember>(r, &r->herm_tab, &r->herm_tab_src, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return AdvanceMember{{(unsigned long long)mem.pos_off, (unsigned long long)mem.vel_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, 0, r->members);
  const AdvanceMember* dev = (const AdvanceMember*)r->herm_tab;
  AdvanceFinishArgs<T> fin{};
  fin.table = dev;
  fin.members = r->members;
  AdvanceClockArgs clk{};
  clk.table = dev;
  return run_advance<T>(r, where, (size_t)object_bodies(r), (size_t)r->members, g.splits, span_of(r, 0, r->members).vel_count, p, fin, clk, [&](const PairLaunch<T>& l) {
    RaggedAdvanceArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.velm = (const T4*)r->velm;
    k.keep = l.keep;
    k.table = dev;
    k.parts = l.parts;
    k.predict = l.predict;
    k.tm = l.tm;
    hipLaunchKernelGGL(ragged_advance_kernel<T>, dim3(g.columns, g.splits, r->members), dim3(kBlock), 0, r->stream, k);
  });
}

// a context's side of object_bodies and bodies_noun (nbx_analysis.hpp has the batch kinds'): check_arguments serves all three
using nbx_detail::bodies_noun;
using nbx_detail::object_bodies;
long long object_bodies(const nbx_ctx* c) { return (long long)c->n; }
const char* bodies_noun(const nbx_ctx*) { return "n exceeds"; }

bool positive(double x) { return std::isfinite(x) && x > 0.0; }

// Statuses 2 to 7 of include/nbx_advance.h, the ones the arguments alone decide, in the header's order; *p filled in.
template <typename O>
int check_arguments(const O* o, const char* where, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume,
                    AdvancePlan* p) {
  const std::string w(where);
  if (!positive(t_end)) return fail(NBX_ERR_ARG, w + ": t_end is not finite or not positive");
  if (!positive(dt_cap)) return fail(NBX_ERR_ARG, w + ": dt_cap is not finite or not positive");
  const double eta2 = eta * eta;
  if (!positive(eta) || !positive(eta2)) return fail(NBX_ERR_ARG, w + ": eta is not finite or not positive");  // nor may its square leave the range
  int e = 0;
  const bool pow2 = std::frexp(dt_cap, &e) == 0.5;  // dt_cap = 2^(e - 1)
  const int k_cap = e - 1;
  const int k_min = o->precision == 32 ? -126 : -1022, k_max = o->precision == 32 ? 127 : 1023;
  if (!pow2 || k_cap < k_min || k_cap > k_max)
    return fail(NBX_ERR_ARG, w + ": dt_cap is not a power of two that is a normal value of the object's precision");
  if (levels < 0 || levels > kAdvanceMaxLevels) return fail(NBX_ERR_ARG, w + ": levels is outside [0, 40]");
  const double whole = t_end / dt_cap;  // exact: dt_cap is a power of two (an overflow to inf fails the next test)
  if (whole != std::floor(whole) || !(std::ldexp(whole, levels) <= 4503599627370496.0))
    return fail(NBX_ERR_ARG, w + ": t_end is not a whole multiple of dt_cap, or more than 2^52 steps of the smallest size away");
  if (max_steps < 0) return fail(NBX_ERR_ARG, w + ": max_steps < 0");
  if (object_bodies(o) > kAdvanceMaxBodies) return fail(NBX_ERR_ARG, w + ": " + bodies_noun(o) + " 4194304");
  *p = AdvancePlan{t_end, dt_cap, eta2, k_cap, (int)levels, (int)max_steps, resume != 0};
  return NBX_OK;
}

// nbx_ensemble_advance and nbx_ragged_advance: every check before the first HIP call, in the header's order
template <typename O>
int batch_advance(O* o, const char* where, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  AdvancePlan p{};
  int rc = check_arguments(o, where, t_end, dt_cap, levels, eta, max_steps, resume, &p);
  if (rc) return rc;
  rc = check_uploaded(o, where, 0, o->members);
  if (rc) return rc;
  if (resume) {
    rc = check_resume(o, where, p);
    if (rc) return rc;
  }
  if ((max_steps == 0 && resume) || o->members == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? advance_t<float>(o, where, p) : advance_t<double>(o, where, p);
  });
}

bool size_ok(const nbx_clock_t& t) { return t.struct_size == 0 || t.struct_size == (int32_t)sizeof(nbx_clock_t); }

// one system's record -> the public struct
void clock_fill(const AdvanceClock& ck, int32_t n, double t_end, nbx_clock_t* out) {
  std::memset(out, 0, sizeof(*out));
  out->struct_size = (int32_t)sizeof(nbx_clock_t);
  out->n = n;
  out->t = ck.t;
  out->dt_last = ck.h_last;
  out->dt_next = ck.h;
  out->steps = ck.steps;
  out->floor_steps = ck.floor_steps;
  out->done = ck.t >= t_end ? 1 : 0;
}

// records [first, first + count) of the object's clocks, ordered on its stream: one read-back, one synchronisation
int read_clocks(Object* o, int first, int count, AdvanceClock* raw) {
  HIP_TRY(hipMemcpyAsync(raw, (const AdvanceClock*)o->adv_clock + first, sizeof(AdvanceClock) * (size_t)count, hipMemcpyDeviceToHost, o->stream));
  HIP_TRY(hipStreamSynchronize(o->stream));
  return NBX_OK;
}

// nbx_ensemble_clock and nbx_ragged_clock: every check before the first HIP call
template <typename O>
int batch_clock(O* o, const char* where, int32_t first, int32_t count, nbx_clock_t* out) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!out) return fail(NBX_ERR_ARG, std::string(where) + ": out is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  for (int k = 0; k < count; ++k)
    if (!size_ok(out[k]))
      return fail(NBX_ERR_ARG, std::string(where) + ": out[" + std::to_string(k) + "].struct_size does not match this library");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (!o->adv_have) return fail(NBX_ERR_STATE, std::string(where) + ": no advance call has been made on this object");
  if (count == 0) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  std::vector<AdvanceClock> raw((size_t)count);
  rc = read_clocks(o, first, count, raw.data());
  if (rc) return rc;
  for (int k = 0; k < count; ++k) clock_fill(raw[(size_t)k], o->layout(first + k).n, o->adv_t_end, out + k);
  return NBX_OK;
  });
}

}  // namespace

extern "C" {

int nbx_advance(nbx_ctx* c, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume) {
  constexpr const char* where = "nbx_advance";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_advance: ctx is NULL");
  AdvancePlan p{};
  int rc = check_arguments(c, where, t_end, dt_cap, levels, eta, max_steps, resume, &p);
  if (rc) return rc;
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_advance: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_advance: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_advance: the context owns a slice of the bodies (the velocities of the others are not resident)");
  if (resume) {
    rc = check_resume(c, where, p);
    if (rc) return rc;
  }
  if (max_steps == 0 && resume) return NBX_OK;
  rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? advance_t<float>(c, where, p) : advance_t<double>(c, where, p);
  });
}

int nbx_ensemble_advance(nbx_ensemble* e, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume) {
  return batch_advance(e, "nbx_ensemble_advance", t_end, dt_cap, levels, eta, max_steps, resume);
}

int nbx_ragged_advance(nbx_ragged* r, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume) {
  return batch_advance(r, "nbx_ragged_advance", t_end, dt_cap, levels, eta, max_steps, resume);
}

int nbx_clock(nbx_ctx* c, nbx_clock_t* out) {
  constexpr const char* where = "nbx_clock";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_clock: ctx is NULL");
  if (!out) return fail(NBX_ERR_ARG, "nbx_clock: out is NULL");
  if (!size_ok(*out)) return fail(NBX_ERR_ARG, "nbx_clock: nbx_clock_t.struct_size does not match this library");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_clock: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_clock: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_clock: the context owns a slice of the bodies (the velocities of the others are not resident)");
  if (!c->adv_have) return fail(NBX_ERR_STATE, "nbx_clock: no advance call has been made on this object");
  const int rc = use_device(c);
  if (rc) return rc;
  AdvanceClock raw;
  const int rd = read_clocks(c, 0, 1, &raw);
  if (rd) return rd;
  clock_fill(raw, c->n, c->adv_t_end, out);
  return NBX_OK;
  });
}

int nbx_ensemble_clock(nbx_ensemble* e, int32_t first, int32_t count, nbx_clock_t* out) {
  return batch_clock(e, "nbx_ensemble_clock", first, count, out);
}

int nbx_ragged_clock(nbx_ragged* r, int32_t first, int32_t count, nbx_clock_t* out) {
  return batch_clock(r, "nbx_ragged_clock", first, count, out);
}

}  // extern "C"
