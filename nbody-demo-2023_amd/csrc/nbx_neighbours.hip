// nbx_neighbours.hip -- nbx_neighbours, nbx_ensemble_neighbours and nbx_ragged_neighbours (include/nbx_neighbours.h) over the
// kernels of nbx_neighbours_kernels.hpp: for every body of a context's state, or of any range of members, its nearest neighbour,
// the softened squared distance to it and the number of bodies within a radius: one pair-work launch, one finish launch and one
// read-back for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it for a context and an
// ensemble, the device for every member of a ragged ensemble -- but nothing here depends on it: the results are a minimum with a
// lowest-index tie-break and an integer sum.  The call reads posm[cur] and writes nb_part and nb_out, buffers of its own: the
// trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/nbx_neighbours.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_neighbours_kernels.hpp"
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

struct Outputs {
  int32_t* index;
  void* r2;
  int32_t* within;
};

bool no_output(const Outputs& a) { return !a.index && !a.r2 && !a.within; }
bool bad_radius(double radius) { return !(radius >= 0.0); }  // NaN or negative

// h2 = fma(rT, rT, eps2), once, in T
template <typename T>
T radius2(double radius) {
  const T r = (T)radius;
  return std::fma(r, r, softening2<T>());
}

// What the three kinds share once the checks are through: `launch` the kind's pair work over `row_splits` rows per member,
// finish, read back, synchronise, scatter.  table: the ragged ensemble's device table (nullptr: every system has n_all bodies).
template <typename T, typename Launch>
int run_neighbours(Object* o, const char* where, size_t total, int row_splits, const NbMember* table, unsigned first, int count, int n_all,
                   const Outputs& a, Launch launch) {
  using Rec = NbRecord<T>;
  int rc = ensure_bytes(&o->nb_part, &o->nb_part_cap, sizeof(Rec) * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->nb_out, &o->nb_out_cap, sizeof(Rec) * total, where, "the results");
  if (rc) return rc;
  std::vector<Rec> res(total);
  rc = read_back(o, res.data(), o->nb_out, sizeof(Rec) * total, [&]() -> int {
    launch((Rec*)o->nb_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(neighbour_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                       (const Rec*)o->nb_part, table, first, count, n_all, row_splits, (unsigned)total, (Rec*)o->nb_out);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;
  T* r2 = (T*)a.r2;
  for (size_t i = 0; i < total; ++i) {
    if (a.index) a.index[i] = res[i].j;
    if (r2) r2[i] = res[i].r2;
    if (a.within) a.within[i] = res[i].count;
  }
  return NBX_OK;
}

template <typename T>
int neighbours_ctx_t(nbx_ctx* c, const char* where, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  const T h2 = radius2<T>(radius);
  return run_neighbours<T>(c, where, (size_t)c->n, s.splits, nullptr, 0u, 1, c->n, a, [&](NbRecord<T>* parts) {
    const dim3 grid(s.columns, s.splits);
    if (a.within)
      hipLaunchKernelGGL((neighbour_kernel<T, true>), grid, dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], c->n, s.tiles_per_split, h2,
                         parts);
    else
      hipLaunchKernelGGL((neighbour_kernel<T, false>), grid, dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], c->n, s.tiles_per_split, h2,
                         parts);
  });
}

template <typename T>
int neighbours_members_t(nbx_ensemble* e, const char* where, int first, int count, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  return run_neighbours<T>(e, where, (size_t)count * (size_t)e->n, s.splits, nullptr, (unsigned)first, count, e->n, a, [&](NbRecord<T>* parts) {
    EnsembleNbArgs<T> k{};
    k.posm = (const T4*)e->posm[e->cur];
    k.parts = parts;
    k.h2 = radius2<T>(radius);
    k.first = (unsigned)first;
    k.pos_stride = (unsigned)e->pos_stride;
    k.n = e->n;
    k.tiles_per_split = s.tiles_per_split;
    const dim3 grid(s.columns, s.splits, count);
    if (a.within) hipLaunchKernelGGL((ensemble_neighbour_kernel<T, true>), grid, dim3(kBlock), 0, e->stream, k);
    else hipLaunchKernelGGL((ensemble_neighbour_kernel<T, false>), grid, dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int neighbours_members_t(nbx_ragged* r, const char* where, int first, int count, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  std::vector<NbMember> table;  // lives until run_neighbours has synchronised
  const int rc = ragged_member_table<NbMember>(r, &r->nb_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return NbMember{{(unsigned long long)mem.pos_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count);
  const NbMember* dev = (const NbMember*)r->nb_tab;
  return run_neighbours<T>(r, where, (size_t)range_bodies(r, first, count), g.splits, dev, (unsigned)first, count, 0, a, [&](NbRecord<T>* parts) {
    RaggedNbArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.table = dev;
    k.parts = parts;
    k.h2 = radius2<T>(radius);
    k.first = (unsigned)first;
    const dim3 grid(g.columns, g.splits, count);
    if (a.within) hipLaunchKernelGGL((ragged_neighbour_kernel<T, true>), grid, dim3(kBlock), 0, r->stream, k);
    else hipLaunchKernelGGL((ragged_neighbour_kernel<T, false>), grid, dim3(kBlock), 0, r->stream, k);
  });
}

// nbx_ensemble_neighbours and nbx_ragged_neighbours: every check before the first HIP call, in the header's order
template <typename O>
int batch_neighbours(O* o, const char* where, int32_t first, int32_t count, double radius, const Outputs& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (bad_radius(radius)) return fail(NBX_ERR_ARG, std::string(where) + ": radius is NaN or negative");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kNbMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(a)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? neighbours_members_t<float>(o, where, first, count, radius, a)
                            : neighbours_members_t<double>(o, where, first, count, radius, a);
  });
}

}  // namespace

extern "C" {

int nbx_neighbours(nbx_ctx* c, double radius, int32_t* index, void* r2, int32_t* within) {
  constexpr const char* where = "nbx_neighbours";
  const Outputs a{index, r2, within};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_neighbours: ctx is NULL");
  if (bad_radius(radius)) return fail(NBX_ERR_ARG, "nbx_neighbours: radius is NaN or negative");
  if ((long long)c->n > kNbMaxBodies) return fail(NBX_ERR_ARG, "nbx_neighbours: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_neighbours: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_neighbours: a local step awaits nbx_commit");
  if (no_output(a)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? neighbours_ctx_t<float>(c, where, radius, a) : neighbours_ctx_t<double>(c, where, radius, a);
  });
}

int nbx_ensemble_neighbours(nbx_ensemble* e, int32_t first, int32_t count, double radius, int32_t* index, void* r2, int32_t* within) {
  return batch_neighbours(e, "nbx_ensemble_neighbours", first, count, radius, Outputs{index, r2, within});
}

int nbx_ragged_neighbours(nbx_ragged* r, int32_t first, int32_t count, double radius, int32_t* index, void* r2, int32_t* within) {
  return batch_neighbours(r, "nbx_ragged_neighbours", first, count, radius, Outputs{index, r2, within});
}

}  // extern "C"
