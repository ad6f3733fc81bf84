// nbx_jerk.hip -- nbx_jerk, nbx_ensemble_jerk and nbx_ragged_jerk (include/nbx_jerk.h) over the kernels of
// nbx_jerk_kernels.hpp: for every body of a context's state, or of any range of members, its acceleration and the time
// derivative of that acceleration: one pair-work launch, one finish launch and one read-back for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it for a context and an
// ensemble, the device for every member of a ragged ensemble; a function of n alone, so a member's partial rows, and with them
// its bits, are a lone context's.  The call reads posm[cur] and velm and writes jerk_part and jerk_out, buffers of its own: the
// trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nbx_jerk.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_jerk_kernels.hpp"
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

bool no_output(const nbx_jerk_out_t& a) {
  for (int k = 0; k < 3; ++k)
    if (a.acc[k] || a.jerk[k]) return false;
  return true;
}

// What the three kinds share once the checks are through: `launch` the kind's pair work over `row_splits` rows per member,
// finish, read back, synchronise, scatter.  table: the ragged ensemble's device table (nullptr: every system has n_all bodies).
template <typename T, typename Launch>
int run_jerk(Object* o, const char* where, size_t total, int row_splits, const JerkMember* table, unsigned first, int count, int n_all,
             const nbx_jerk_out_t& a, Launch launch) {
  using T4 = typename V4<T>::type;
  int rc = ensure_bytes(&o->jerk_part, &o->jerk_part_cap, sizeof(T4) * 2 * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->jerk_out, &o->jerk_out_cap, sizeof(T4) * 2 * total, where, "the results");
  if (rc) return rc;
  std::vector<T4> res(2 * total);
  rc = read_back(o, res.data(), o->jerk_out, sizeof(T4) * 2 * total, [&]() -> int {
    launch((T4*)o->jerk_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jerk_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                       (const T4*)o->jerk_part, table, first, count, n_all, row_splits, (unsigned)total, (T4*)o->jerk_out);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;
  T* const ax = (T*)a.acc[0]; T* const ay = (T*)a.acc[1]; T* const az = (T*)a.acc[2];
  T* const jx = (T*)a.jerk[0]; T* const jy = (T*)a.jerk[1]; T* const jz = (T*)a.jerk[2];
  for (size_t i = 0; i < total; ++i) {
    const T4 p = res[2 * i], q = res[2 * i + 1];
    if (ax) ax[i] = p.x;
    if (ay) ay[i] = p.y;
    if (az) az[i] = p.z;
    if (jx) jx[i] = q.x;
    if (jy) jy[i] = q.y;
    if (jz) jz[i] = q.z;
  }
  return NBX_OK;
}

template <typename T>
int jerk_ctx_t(nbx_ctx* c, const char* where, const nbx_jerk_out_t& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  return run_jerk<T>(c, where, (size_t)c->n, s.splits, nullptr, 0u, 1, c->n, a, [&](T4* parts) {
    hipLaunchKernelGGL(jerk_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], (const T4*)c->velm,
                       c->n, s.tiles_per_split, parts);
  });
}

template <typename T>
int jerk_members_t(nbx_ensemble* e, const char* where, int first, int count, const nbx_jerk_out_t& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  return run_jerk<T>(e, where, (size_t)count * (size_t)e->n, s.splits, nullptr, (unsigned)first, count, e->n, a, [&](T4* parts) {
    EnsembleJerkArgs<T> k{};
    k.posm = (const T4*)e->posm[e->cur];
    k.velm = (const T4*)e->velm;
    k.parts = parts;
    k.first = (unsigned)first;
    k.pos_stride = (unsigned)e->pos_stride;
    k.vel_stride = (unsigned)e->own_pad;
    k.n = e->n;
    k.tiles_per_split = s.tiles_per_split;
    hipLaunchKernelGGL(ensemble_jerk_kernel<T>, dim3(s.columns, s.splits, count), dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int jerk_members_t(nbx_ragged* r, const char* where, int first, int count, const nbx_jerk_out_t& a) {
  using T4 = typename V4<T>::type;
  std::vector<JerkMember> table;  // lives until run_jerk has synchronised
  const int rc = ragged_member_table<JerkMember>(r, &r->jerk_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return JerkMember{{(unsigned long long)mem.pos_off, (unsigned long long)mem.vel_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count);
  const JerkMember* dev = (const JerkMember*)r->jerk_tab;
  return run_jerk<T>(r, where, (size_t)range_bodies(r, first, count), g.splits, dev, (unsigned)first, count, 0, a, [&](T4* parts) {
    RaggedJerkArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.velm = (const T4*)r->velm;
    k.table = dev;
    k.parts = parts;
    k.first = (unsigned)first;
    hipLaunchKernelGGL(ragged_jerk_kernel<T>, dim3(g.columns, g.splits, count), dim3(kBlock), 0, r->stream, k);
  });
}

// nbx_ensemble_jerk and nbx_ragged_jerk: every check before the first HIP call, in the header's order
template <typename O>
int batch_jerk(O* o, const char* where, int32_t first, int32_t count, const nbx_jerk_out_t* out) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!out) return fail(NBX_ERR_ARG, std::string(where) + ": out is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kJerkMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(*out)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? jerk_members_t<float>(o, where, first, count, *out) : jerk_members_t<double>(o, where, first, count, *out);
  });
}

}  // namespace

extern "C" {

int nbx_jerk(nbx_ctx* c, const nbx_jerk_out_t* out) {
  constexpr const char* where = "nbx_jerk";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_jerk: ctx is NULL");
  if (!out) return fail(NBX_ERR_ARG, "nbx_jerk: out is NULL");
  if ((long long)c->n > kJerkMaxBodies) return fail(NBX_ERR_ARG, "nbx_jerk: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_jerk: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_jerk: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_jerk: the context owns a slice of the bodies (the velocities of the others are not resident)");
  if (no_output(*out)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? jerk_ctx_t<float>(c, where, *out) : jerk_ctx_t<double>(c, where, *out);
  });
}

int nbx_ensemble_jerk(nbx_ensemble* e, int32_t first, int32_t count, const nbx_jerk_out_t* out) {
  return batch_jerk(e, "nbx_ensemble_jerk", first, count, out);
}

int nbx_ragged_jerk(nbx_ragged* r, int32_t first, int32_t count, const nbx_jerk_out_t* out) {
  return batch_jerk(r, "nbx_ragged_jerk", first, count, out);
}

}  // extern "C"
