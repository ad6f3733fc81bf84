// nbx_field.hip -- nbx_field, nbx_ensemble_field and nbx_ragged_field (include/nbx_field.h) over the kernels of
// nbx_field_kernels.hpp: the softened acceleration and potential of a context's state, or of any range of members, at points
// the caller supplies: one upload of the points, one pair-work launch, one finish launch and one read-back for all systems asked
// for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair function is compiled once for the
// three kinds.  The launch shape of a system is field_shape(m, n) (nbx_field_shape.hpp) and nothing else: the host evaluates it
// for a context and an ensemble, the device for every member of a ragged ensemble.  The call reads posm[cur] and writes
// field_pts, field_part and field_out, buffers of its own: the trajectory, ke_part, have_parts, the profile and the cached
// graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nbx_field.h"
#include "nbx_analysis.hpp"           // ensure_bytes, ragged_member_table, ragged_extents, read_back
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded
#include "nbx_field_kernels.hpp"
#include "nbx_internal.hpp"         // struct nbx_ctx
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

struct Arrays {
  const void *px, *py, *pz;
  void *ax, *ay, *az, *phi;
};

// What the three kinds share once the checks are through: pack and upload the `total` = count * m points, `launch` the kind's
// pair work over `row_splits` rows of m records per member, finish, read back, synchronise, scatter.  table: the ragged
// ensemble's device table (nullptr: every system has n_all bodies).
template <typename T, typename Launch>
int run_field(Object* o, const char* where, int count, int m, int row_splits, const FieldMember* table, unsigned first, int n_all,
              const Arrays& a, Launch launch) {
  using T4 = typename V4<T>::type;
  const size_t total = (size_t)count * (size_t)m;
  int rc = ensure_bytes(&o->field_pts, &o->field_pts_cap, sizeof(T4) * total, where, "the points");
  if (rc) return rc;
  rc = ensure_bytes(&o->field_part, &o->field_part_cap, sizeof(T4) * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->field_out, &o->field_out_cap, sizeof(T4) * total, where, "the results");
  if (rc) return rc;
  std::vector<T4> host(total);
  const T *px = (const T*)a.px, *py = (const T*)a.py, *pz = (const T*)a.pz;
  for (size_t i = 0; i < total; ++i) {
    T4 q; q.x = px[i]; q.y = py[i]; q.z = pz[i]; q.w = (T)0;
    host[i] = q;
  }
  std::vector<T4> res(total);  // not `host`: the points may still be leaving it
  rc = read_back(o, res.data(), o->field_out, sizeof(T4) * total, [&]() -> int {
    HIP_TRY(hipMemcpyAsync(o->field_pts, host.data(), sizeof(T4) * total, hipMemcpyHostToDevice, o->stream));
    launch((const T4*)o->field_pts, (T4*)o->field_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(field_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                       (const T4*)o->field_part, table, first, n_all, m, row_splits, (unsigned)total, (T4*)o->field_out);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;  // read_back has synchronised: no copy outlives `host` and `res`
  T *ax = (T*)a.ax, *ay = (T*)a.ay, *az = (T*)a.az, *phi = (T*)a.phi;
  for (size_t i = 0; i < total; ++i) {
    if (ax) ax[i] = res[i].x;
    if (ay) ay[i] = res[i].y;
    if (az) az[i] = res[i].z;
    if (phi) phi[i] = res[i].w;
  }
  return NBX_OK;
}

template <typename T>
int field_ctx_t(nbx_ctx* c, const char* where, int m, const Arrays& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(m, c->n);
  return run_field<T>(c, where, 1, m, s.splits, nullptr, 0u, c->n, a, [&](const T4* pts, T4* parts) {
    hipLaunchKernelGGL(field_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], c->n, pts, m,
                       s.tiles_per_split, parts);
  });
}

template <typename T>
int field_members_t(nbx_ensemble* e, const char* where, int first, int count, int m, const Arrays& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(m, e->n);
  return run_field<T>(e, where, count, m, s.splits, nullptr, (unsigned)first, e->n, a, [&](const T4* pts, T4* parts) {
    EnsembleFieldArgs<T> k{};
    k.posm = (const T4*)e->posm[e->cur];
    k.pts = pts;
    k.parts = parts;
    k.first = (unsigned)first;
    k.pos_stride = (unsigned)e->pos_stride;
    k.n = e->n;
    k.m = m;
    k.tiles_per_split = s.tiles_per_split;
    hipLaunchKernelGGL(ensemble_field_kernel<T>, dim3(s.columns, s.splits, count), dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's y extent is the largest number of splits any
// member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int field_members_t(nbx_ragged* r, const char* where, int first, int count, int m, const Arrays& a) {
  using T4 = typename V4<T>::type;
  std::vector<FieldMember> table;  // lives until run_field has synchronised
  const int rc = ragged_member_table<FieldMember>(r, &r->field_tab, &table, where, [](const MemberSpan& mem, unsigned long long) {
    return FieldMember{{(unsigned long long)mem.pos_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count, m);  // m > 0: every member has the same columns
  const FieldMember* dev = (const FieldMember*)r->field_tab;
  return run_field<T>(r, where, count, m, g.splits, dev, (unsigned)first, 0, a, [&](const T4* pts, T4* parts) {
    RaggedFieldArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.table = dev;
    k.pts = pts;
    k.parts = parts;
    k.first = (unsigned)first;
    k.m = m;
    hipLaunchKernelGGL(ragged_field_kernel<T>, dim3(g.columns, g.splits, count), dim3(kBlock), 0, r->stream, k);
  });
}

bool no_output(const Arrays& a) { return !a.ax && !a.ay && !a.az && !a.phi; }

// nbx_ensemble_field and nbx_ragged_field: every check before the first HIP call, in the header's order
template <typename O>
int batch_field(O* o, const char* where, int32_t first, int32_t count, int32_t m, const Arrays& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (m < 0) return fail(NBX_ERR_ARG, std::string(where) + ": m < 0");
  if (m > 0 && (!a.px || !a.py || !a.pz)) return fail(NBX_ERR_ARG, std::string(where) + ": NULL point array");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if ((long long)count * m > kFieldMaxPoints) return fail(NBX_ERR_ARG, std::string(where) + ": count * m exceeds 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (m == 0 || count == 0 || no_output(a)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? field_members_t<float>(o, where, first, count, m, a) : field_members_t<double>(o, where, first, count, m, a);
  });
}

}  // namespace

extern "C" {

int nbx_field(nbx_ctx* c, int32_t m, const void* px, const void* py, const void* pz, void* ax, void* ay, void* az, void* phi) {
  constexpr const char* where = "nbx_field";
  const Arrays a{px, py, pz, ax, ay, az, phi};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_field: ctx is NULL");
  if (m < 0) return fail(NBX_ERR_ARG, "nbx_field: m < 0");
  if (m > 0 && (!px || !py || !pz)) return fail(NBX_ERR_ARG, "nbx_field: NULL point array");
  if ((long long)m > kFieldMaxPoints) return fail(NBX_ERR_ARG, "nbx_field: m exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_field: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_field: a local step awaits nbx_commit");
  if (m == 0 || no_output(a)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? field_ctx_t<float>(c, where, m, a) : field_ctx_t<double>(c, where, m, a);
  });
}

int nbx_ensemble_field(nbx_ensemble* e, int32_t first, int32_t count, int32_t m, const void* px, const void* py, const void* pz, void* ax,
                       void* ay, void* az, void* phi) {
  return batch_field(e, "nbx_ensemble_field", first, count, m, Arrays{px, py, pz, ax, ay, az, phi});
}

int nbx_ragged_field(nbx_ragged* r, int32_t first, int32_t count, int32_t m, const void* px, const void* py, const void* pz, void* ax,
                     void* ay, void* az, void* phi) {
  return batch_field(r, "nbx_ragged_field", first, count, m, Arrays{px, py, pz, ax, ay, az, phi});
}

}  // extern "C"
