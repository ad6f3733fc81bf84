// nbx_binaries.hip -- nbx_binaries, nbx_ensemble_binaries and nbx_ragged_binaries (include/nbx_binaries.h) over the kernels of
// nbx_binaries_kernels.hpp: for every body of a context's state, or of any range of members, its most bound partner, the
// specific two-body energy of that pair and the number of bodies it is bound to: one pair-work launch, one finish launch and
// one read-back for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it for a context and an
// ensemble, the device for every member of a ragged ensemble -- but nothing here depends on it: the results are a minimum with a
// lowest-index tie-break and an integer sum.  The call reads posm[cur] and velm and writes bin_part and bin_out, buffers of its
// own: the trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nbx_binaries.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_binaries_kernels.hpp"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

struct Outputs {
  int32_t* partner;
  void* energy;
  int32_t* bound;
};

bool no_output(const Outputs& a) { return !a.partner && !a.energy && !a.bound; }

// What the three kinds share once the checks are through: `launch` the kind's pair work over `row_splits` rows per member,
// finish, read back, synchronise, scatter.  table: the ragged ensemble's device table (nullptr: every system has n_all bodies).
template <typename T, typename Launch>
int run_binaries(Object* o, const char* where, size_t total, int row_splits, const BoundMember* table, unsigned first, int count, int n_all,
                 const Outputs& a, Launch launch) {
  using Rec = BoundRecord<T>;
  int rc = ensure_bytes(&o->bin_part, &o->bin_part_cap, sizeof(Rec) * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->bin_out, &o->bin_out_cap, sizeof(Rec) * total, where, "the results");
  if (rc) return rc;
  std::vector<Rec> res(total);
  rc = read_back(o, res.data(), o->bin_out, sizeof(Rec) * total, [&]() -> int {
    launch((Rec*)o->bin_part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bound_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                       (const Rec*)o->bin_part, table, first, count, n_all, row_splits, (unsigned)total, (Rec*)o->bin_out);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;
  T* energy = (T*)a.energy;
  for (size_t i = 0; i < total; ++i) {
    if (a.partner) a.partner[i] = res[i].j;
    if (energy) energy[i] = res[i].e;
    if (a.bound) a.bound[i] = res[i].count;
  }
  return NBX_OK;
}

template <typename T>
int binaries_ctx_t(nbx_ctx* c, const char* where, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  return run_binaries<T>(c, where, (size_t)c->n, s.splits, nullptr, 0u, 1, c->n, a, [&](BoundRecord<T>* parts) {
    const dim3 grid(s.columns, s.splits);
    if (a.bound)
      hipLaunchKernelGGL((bound_kernel<T, true>), grid, dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], (const T4*)c->velm, c->n,
                         s.tiles_per_split, parts);
    else
      hipLaunchKernelGGL((bound_kernel<T, false>), grid, dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], (const T4*)c->velm, c->n,
                         s.tiles_per_split, parts);
  });
}

template <typename T>
int binaries_members_t(nbx_ensemble* e, const char* where, int first, int count, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  return run_binaries<T>(e, where, (size_t)count * (size_t)e->n, s.splits, nullptr, (unsigned)first, count, e->n, a, [&](BoundRecord<T>* parts) {
    EnsembleBoundArgs<T> k{};
    k.posm = (const T4*)e->posm[e->cur];
    k.velm = (const T4*)e->velm;
    k.parts = parts;
    k.first = (unsigned)first;
    k.pos_stride = (unsigned)e->pos_stride;
    k.vel_stride = (unsigned)e->own_pad;
    k.n = e->n;
    k.tiles_per_split = s.tiles_per_split;
    const dim3 grid(s.columns, s.splits, count);
    if (a.bound) hipLaunchKernelGGL((ensemble_bound_kernel<T, true>), grid, dim3(kBlock), 0, e->stream, k);
    else hipLaunchKernelGGL((ensemble_bound_kernel<T, false>), grid, dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int binaries_members_t(nbx_ragged* r, const char* where, int first, int count, const Outputs& a) {
  using T4 = typename V4<T>::type;
  std::vector<BoundMember> table;  // lives until run_binaries has synchronised
  const int rc = ragged_member_table<BoundMember>(r, &r->bin_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return BoundMember{{(unsigned long long)mem.pos_off, (unsigned long long)mem.vel_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count);
  const BoundMember* dev = (const BoundMember*)r->bin_tab;
  return run_binaries<T>(r, where, (size_t)range_bodies(r, first, count), g.splits, dev, (unsigned)first, count, 0, a, [&](BoundRecord<T>* parts) {
    RaggedBoundArgs<T> k{};
    k.posm = (const T4*)r->posm[r->cur];
    k.velm = (const T4*)r->velm;
    k.table = dev;
    k.parts = parts;
    k.first = (unsigned)first;
    const dim3 grid(g.columns, g.splits, count);
    if (a.bound) hipLaunchKernelGGL((ragged_bound_kernel<T, true>), grid, dim3(kBlock), 0, r->stream, k);
    else hipLaunchKernelGGL((ragged_bound_kernel<T, false>), grid, dim3(kBlock), 0, r->stream, k);
  });
}

// nbx_ensemble_binaries and nbx_ragged_binaries: every check before the first HIP call, in the header's order
template <typename O>
int batch_binaries(O* o, const char* where, int32_t first, int32_t count, const Outputs& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kBoundMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(a)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? binaries_members_t<float>(o, where, first, count, a) : binaries_members_t<double>(o, where, first, count, a);
  });
}

}  // namespace

extern "C" {

int nbx_binaries(nbx_ctx* c, int32_t* partner, void* energy, int32_t* bound) {
  constexpr const char* where = "nbx_binaries";
  const Outputs a{partner, energy, bound};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_binaries: ctx is NULL");
  if ((long long)c->n > kBoundMaxBodies) return fail(NBX_ERR_ARG, "nbx_binaries: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_binaries: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_binaries: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_binaries: the context owns a slice of the bodies (the velocities of the others are not resident)");
  if (no_output(a)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? binaries_ctx_t<float>(c, where, a) : binaries_ctx_t<double>(c, where, a);
  });
}

int nbx_ensemble_binaries(nbx_ensemble* e, int32_t first, int32_t count, int32_t* partner, void* energy, int32_t* bound) {
  return batch_binaries(e, "nbx_ensemble_binaries", first, count, Outputs{partner, energy, bound});
}

int nbx_ragged_binaries(nbx_ragged* r, int32_t first, int32_t count, int32_t* partner, void* energy, int32_t* bound) {
  return batch_binaries(r, "nbx_ragged_binaries", first, count, Outputs{partner, energy, bound});
}

}  // extern "C"
