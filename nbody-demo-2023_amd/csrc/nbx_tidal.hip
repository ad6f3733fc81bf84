// nbx_tidal.hip -- the six entry points of include/nbx_tidal.h over the kernels of nbx_tidal_kernels.hpp: the tidal tensor of a
// context's state, or of any range of members, at points the caller supplies (nbx_tidal, nbx_ensemble_tidal, nbx_ragged_tidal)
// or at the resident bodies themselves, the body's own term never formed (nbx_tidal_bodies, nbx_ensemble_tidal_bodies,
// nbx_ragged_tidal_bodies): one upload of the points (none in bodies mode), one pair-work launch, one finish launch and one
// read-back for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair function is compiled once for the
// three kinds.  The launch shape of a system is field_shape(m, n) in points mode and field_shape(n, n) in bodies mode
// (nbx_field_shape.hpp) and nothing else: the host evaluates it for a context and an ensemble, the device for every member of a
// ragged ensemble.  The call reads posm[cur] and writes tidal_pts, tidal_part and tidal_out, buffers of its own: the trajectory,
// ke_part, have_parts, the profile, the cached graphs and the other analysis calls' buffers do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nbx_tidal.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged
#include "nbx_tidal_kernels.hpp"

using namespace nbx;
using namespace nbx_detail;

namespace {

// points == nullptr: bodies mode
struct Points {
  const void *px, *py, *pz;
};

bool no_output(void* const* t) {
  for (int c = 0; c < 6; ++c)
    if (t[c]) return false;
  return true;
}

// What the six entry points share once the checks are through: in points mode pack and upload the `total` = count * m points;
// `launch` the kind's pair work over `row_splits` rows per system, finish, read back, synchronise, scatter.  m: points per system
// (0: bodies mode, `total` the bodies of the range).  table: the ragged ensemble's device table (nullptr: every system has n_all
// bodies).
template <typename T, typename Launch>
int run_tidal(Object* o, const char* where, size_t total, int count, int m, int row_splits, const TidalMember* table, unsigned first,
              int n_all, const Points* p, void* const* t, Launch launch) {
  using T4 = typename V4<T>::type;
  int rc = NBX_OK;
  if (p) {
    rc = ensure_bytes(&o->tidal_pts, &o->tidal_pts_cap, sizeof(T4) * total, where, "the points");
    if (rc) return rc;
  }
  rc = ensure_bytes(&o->tidal_part, &o->tidal_part_cap, 2 * sizeof(T4) * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->tidal_out, &o->tidal_out_cap, 2 * sizeof(T4) * total, where, "the results");
  if (rc) return rc;
  std::vector<T4> host;
  if (p) {
    host.resize(total);
    const T *px = (const T*)p->px, *py = (const T*)p->py, *pz = (const T*)p->pz;
    for (size_t i = 0; i < total; ++i) {
      T4 q; q.x = px[i]; q.y = py[i]; q.z = pz[i]; q.w = (T)0;
      host[i] = q;
    }
  }
  std::vector<T4> res(2 * total);  // not `host`: the points may still be leaving it
  rc = read_back(o, res.data(), o->tidal_out, 2 * sizeof(T4) * total, [&]() -> int {
    if (p) HIP_TRY(hipMemcpyAsync(o->tidal_pts, host.data(), sizeof(T4) * total, hipMemcpyHostToDevice, o->stream));
    launch((const T4*)o->tidal_pts, (T4*)o->tidal_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tidal_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                       (const T4*)o->tidal_part, table, first, count, n_all, m, row_splits, (unsigned)total, (T4*)o->tidal_out);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;  // read_back has synchronised: no copy outlives `host` and `res`
  T* out[6];
  for (int c = 0; c < 6; ++c) out[c] = (T*)t[c];
  for (size_t i = 0; i < total; ++i) {
    const T4 a = res[2 * i], b = res[2 * i + 1];
    if (out[0]) out[0][i] = a.x;
    if (out[1]) out[1][i] = a.y;
    if (out[2]) out[2][i] = a.z;
    if (out[3]) out[3][i] = a.w;
    if (out[4]) out[4][i] = b.x;
    if (out[5]) out[5][i] = b.y;
  }
  return NBX_OK;
}

// a context: m points (points mode) or its n bodies (p == nullptr)
template <typename T>
int tidal_ctx_t(nbx_ctx* c, const char* where, int m, const Points* p, void* const* t) {
  using T4 = typename V4<T>::type;
  const int pts = p ? m : c->n;
  const FieldShape s = field_shape(pts, c->n);
  return run_tidal<T>(c, where, (size_t)pts, 1, p ? m : 0, s.splits, nullptr, 0u, c->n, p, t, [&](const T4* dpts, T4* parts) {
    const dim3 grid(s.columns, s.splits);
    const T4* posm = (const T4*)c->posm[c->cur];
    if (p) hipLaunchKernelGGL((tidal_kernel<T, false>), grid, dim3(kBlock), 0, c->stream, posm, c->n, dpts, m, s.tiles_per_split, parts);
    else hipLaunchKernelGGL((tidal_kernel<T, true>), grid, dim3(kBlock), 0, c->stream, posm, c->n, posm, c->n, s.tiles_per_split, parts);
  });
}

template <typename T>
int tidal_members_t(nbx_ensemble* e, const char* where, int first, int count, int m, const Points* p, void* const* t) {
  using T4 = typename V4<T>::type;
  const int pts = p ? m : e->n;
  const FieldShape s = field_shape(pts, e->n);
  return run_tidal<T>(e, where, (size_t)count * (size_t)pts, count, p ? m : 0, s.splits, nullptr, (unsigned)first, e->n, p, t,
                      [&](const T4* dpts, T4* parts) {
    EnsembleTidalArgs<T> k{};
    k.posm = (const T4*)e->posm[e->cur];
    k.pts = dpts;
    k.parts = parts;
    k.first = (unsigned)first;
    k.pos_stride = (unsigned)e->pos_stride;
    k.n = e->n;
    k.m = pts;
    k.tiles_per_split = s.tiles_per_split;
    const dim3 grid(s.columns, s.splits, count);
    if (p) hipLaunchKernelGGL((ensemble_tidal_kernel<T, false>), grid, dim3(kBlock), 0, e->stream, k);
    else hipLaunchKernelGGL((ensemble_tidal_kernel<T, true>), grid, dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call of either mode; the grid's x and y extents are the largest
// number of columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int tidal_members_t(nbx_ragged* r, const char* where, int first, int count, int m, const Points* p, void* const* t) {
  using T4 = typename V4<T>::type;
  std::vector<TidalMember> table;  // lives until run_tidal has synchronised
  const int rc = ragged_member_table<TidalMember>(r, &r->tidal_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return TidalMember{{(unsigned long long)mem.pos_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count, p ? m : 0);
  const size_t total = p ? (size_t)count * (size_t)m : (size_t)range_bodies(r, first, count);
  const TidalMember* dev = (const TidalMember*)r->tidal_tab;
  return run_tidal<T>(r, where, total, count, p ? m : 0, g.splits, dev, (unsigned)first, 0, p, t, [&](const T4* dpts, T4* parts) {
    RaggedTidalArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.table = dev;
    k.pts = dpts;
    k.parts = parts;
    k.first = (unsigned)first;
    k.m = m;
    const dim3 grid(g.columns, g.splits, count);
    if (p) hipLaunchKernelGGL((ragged_tidal_kernel<T, false>), grid, dim3(kBlock), 0, r->stream, k);
    else hipLaunchKernelGGL((ragged_tidal_kernel<T, true>), grid, dim3(kBlock), 0, r->stream, k);
  });
}

// nbx_ensemble_tidal and nbx_ragged_tidal: every check before the first HIP call, in the header's order
template <typename O>
int batch_tidal(O* o, const char* where, int32_t first, int32_t count, int32_t m, const Points& p, void* const* t) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (m < 0) return fail(NBX_ERR_ARG, std::string(where) + ": m < 0");
  if (m > 0 && (!p.px || !p.py || !p.pz)) return fail(NBX_ERR_ARG, std::string(where) + ": NULL point array");
  if (!t) return fail(NBX_ERR_ARG, std::string(where) + ": t is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if ((long long)count * m > kTidalMaxPoints) return fail(NBX_ERR_ARG, std::string(where) + ": count * m exceeds 2097152");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (m == 0 || count == 0 || no_output(t)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? tidal_members_t<float>(o, where, first, count, m, &p, t)
                            : tidal_members_t<double>(o, where, first, count, m, &p, t);
  });
}

// nbx_ensemble_tidal_bodies and nbx_ragged_tidal_bodies, likewise
template <typename O>
int batch_tidal_bodies(O* o, const char* where, int32_t first, int32_t count, void* const* t) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!t) return fail(NBX_ERR_ARG, std::string(where) + ": t is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kTidalMaxPoints) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 2097152");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(t)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? tidal_members_t<float>(o, where, first, count, 0, nullptr, t)
                            : tidal_members_t<double>(o, where, first, count, 0, nullptr, t);
  });
}

}  // namespace

extern "C" {

int nbx_tidal(nbx_ctx* c, int32_t m, const void* px, const void* py, const void* pz, void* t[6]) {
  constexpr const char* where = "nbx_tidal";
  const Points p{px, py, pz};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_tidal: ctx is NULL");
  if (m < 0) return fail(NBX_ERR_ARG, "nbx_tidal: m < 0");
  if (m > 0 && (!px || !py || !pz)) return fail(NBX_ERR_ARG, "nbx_tidal: NULL point array");
  if (!t) return fail(NBX_ERR_ARG, "nbx_tidal: t is NULL");
  if ((long long)m > kTidalMaxPoints) return fail(NBX_ERR_ARG, "nbx_tidal: m exceeds 2097152");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_tidal: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_tidal: a local step awaits nbx_commit");
  if (m == 0 || no_output(t)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? tidal_ctx_t<float>(c, where, m, &p, t) : tidal_ctx_t<double>(c, where, m, &p, t);
  });
}

int nbx_ensemble_tidal(nbx_ensemble* e, int32_t first, int32_t count, int32_t m, const void* px, const void* py, const void* pz,
                       void* t[6]) {
  return batch_tidal(e, "nbx_ensemble_tidal", first, count, m, Points{px, py, pz}, t);
}

int nbx_ragged_tidal(nbx_ragged* r, int32_t first, int32_t count, int32_t m, const void* px, const void* py, const void* pz, void* t[6]) {
  return batch_tidal(r, "nbx_ragged_tidal", first, count, m, Points{px, py, pz}, t);
}

int nbx_tidal_bodies(nbx_ctx* c, void* t[6]) {
  constexpr const char* where = "nbx_tidal_bodies";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_tidal_bodies: ctx is NULL");
  if (!t) return fail(NBX_ERR_ARG, "nbx_tidal_bodies: t is NULL");
  if ((long long)c->n > kTidalMaxPoints) return fail(NBX_ERR_ARG, "nbx_tidal_bodies: n exceeds 2097152");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_tidal_bodies: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_tidal_bodies: a local step awaits nbx_commit");
  if (no_output(t)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? tidal_ctx_t<float>(c, where, 0, nullptr, t) : tidal_ctx_t<double>(c, where, 0, nullptr, t);
  });
}

int nbx_ensemble_tidal_bodies(nbx_ensemble* e, int32_t first, int32_t count, void* t[6]) {
  return batch_tidal_bodies(e, "nbx_ensemble_tidal_bodies", first, count, t);
}

int nbx_ragged_tidal_bodies(nbx_ragged* r, int32_t first, int32_t count, void* t[6]) {
  return batch_tidal_bodies(r, "nbx_ragged_tidal_bodies", first, count, t);
}

}  // extern "C"
