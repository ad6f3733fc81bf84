// nbx_knn.hip -- nbx_knn, nbx_ensemble_knn and nbx_ragged_knn (include/nbx_knn.h) over the kernels of nbx_knn_kernels.hpp: for
// every body of a context's state, or of any range of members, its k nearest neighbours and the softened squared distances to
// them: one pair-work launch, one finish launch and one read-back for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once per list
// capacity for the three kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it
// for a context and an ensemble, the device for every member of a ragged ensemble -- but nothing here depends on it, nor on the
// capacity the call picks: a row is a selection under a total order.  The call reads posm[cur] and writes knn_part and knn_out,
// buffers of its own: the trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nbx_knn.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_knn_kernels.hpp"
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

static_assert(kKnnMax == NBX_KNN_MAX && knn_capacity(NBX_KNN_MAX) == NBX_KNN_MAX, "the largest capacity serves the largest k");

namespace {

struct Outputs {
  int32_t* index;
  void* r2;
};

bool no_output(const Outputs& a) { return !a.index && !a.r2; }
bool bad_k(int32_t k) { return k < 1 || k > NBX_KNN_MAX; }

// f(std::integral_constant<int, K>) with K the compiled capacity of k
template <typename F>
void with_capacity(int k, F f) {
  switch (knn_capacity(k)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

// What the three kinds share once the checks are through: `launch` the kind's pair work over `row_splits` rows per member,
// finish, read back, synchronise, scatter.  table: the ragged ensemble's device table (nullptr: every system has n_all bodies).
template <typename T, typename Launch>
int run_knn(Object* o, const char* where, size_t total, int row_splits, const KnnMember* table, unsigned first, int count, int n_all, int k,
            const Outputs& a, Launch launch) {
  using Rec = KnnRecord<T>;
  const size_t entries = total * (size_t)k;
  int rc = ensure_bytes(&o->knn_part, &o->knn_part_cap, sizeof(Rec) * entries * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->knn_out, &o->knn_out_cap, sizeof(Rec) * entries, where, "the results");
  if (rc) return rc;
  std::vector<Rec> res(entries);
  rc = read_back(o, res.data(), o->knn_out, sizeof(Rec) * entries, [&]() -> int {
    launch((Rec*)o->knn_part);
    HIP_TRY(hipGetLastError());
    with_capacity(k, [&](auto cap) {
      hipLaunchKernelGGL((knn_finish_kernel<T, decltype(cap)::value>), dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                         (const Rec*)o->knn_part, table, first, count, n_all, row_splits, k, (unsigned)total, (Rec*)o->knn_out);
    });
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;
  T* r2 = (T*)a.r2;
  for (size_t i = 0; i < entries; ++i) {
    if (a.index) a.index[i] = res[i].j;
    if (r2) r2[i] = res[i].r2;
  }
  return NBX_OK;
}

template <typename T>
int knn_ctx_t(nbx_ctx* c, const char* where, int k, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  return run_knn<T>(c, where, (size_t)c->n, s.splits, nullptr, 0u, 1, c->n, k, a, [&](KnnRecord<T>* parts) {
    const dim3 grid(s.columns, s.splits);
    with_capacity(k, [&](auto cap) {
      hipLaunchKernelGGL((knn_kernel<T, decltype(cap)::value>), grid, dim3(kBlock), 0, c->stream, (const T4*)c->posm[c->cur], c->n,
                         s.tiles_per_split, k, parts);
    });
  });
}

// the words of the size bound, which here is on the entries: the bodies of the range times k
const char* entries_noun(const nbx_ensemble*) { return "count * n * k exceeds"; }
const char* entries_noun(const nbx_ragged*) { return "the bodies of the range times k exceed"; }

template <typename T>
int knn_members_t(nbx_ensemble* e, const char* where, int first, int count, int k, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  return run_knn<T>(e, where, (size_t)count * (size_t)e->n, s.splits, nullptr, (unsigned)first, count, e->n, k, a, [&](KnnRecord<T>* parts) {
    EnsembleKnnArgs<T> w{};
    w.posm = (const T4*)e->posm[e->cur];
    w.parts = parts;
    w.first = (unsigned)first;
    w.pos_stride = (unsigned)e->pos_stride;
    w.n = e->n;
    w.tiles_per_split = s.tiles_per_split;
    w.k = k;
    const dim3 grid(s.columns, s.splits, count);
    with_capacity(k, [&](auto cap) { hipLaunchKernelGGL((ensemble_knn_kernel<T, decltype(cap)::value>), grid, dim3(kBlock), 0, e->stream, w); });
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int knn_members_t(nbx_ragged* r, const char* where, int first, int count, int k, const Outputs& a) {
  using T4 = typename V4<T>::type;
  std::vector<KnnMember> table;  // lives until run_knn has synchronised
  const int rc = ragged_member_table<KnnMember>(r, &r->knn_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return KnnMember{{(unsigned long long)mem.pos_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count);
  const KnnMember* dev = (const KnnMember*)r->knn_tab;
  return run_knn<T>(r, where, (size_t)range_bodies(r, first, count), g.splits, dev, (unsigned)first, count, 0, k, a, [&](KnnRecord<T>* parts) {
    RaggedKnnArgs<T> w{};
    w.posm = (const T4*)r->posm[r->cur];
    w.table = dev;
    w.parts = parts;
    w.first = (unsigned)first;
    w.k = k;
    const dim3 grid(g.columns, g.splits, count);
    with_capacity(k, [&](auto cap) { hipLaunchKernelGGL((ragged_knn_kernel<T, decltype(cap)::value>), grid, dim3(kBlock), 0, r->stream, w); });
  });
}

// nbx_ensemble_knn and nbx_ragged_knn: every check before the first HIP call, in the header's order
template <typename O>
int batch_knn(O* o, const char* where, int32_t first, int32_t count, int32_t k, const Outputs& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (bad_k(k)) return fail(NBX_ERR_ARG, std::string(where) + ": k is outside [1, 16]");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) * (long long)k > kKnnMaxEntries) return fail(NBX_ERR_ARG, std::string(where) + ": " + entries_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(a)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? knn_members_t<float>(o, where, first, count, k, a) : knn_members_t<double>(o, where, first, count, k, a);
  });
}

}  // namespace

extern "C" {

int nbx_knn(nbx_ctx* c, int32_t k, int32_t* index, void* r2) {
  constexpr const char* where = "nbx_knn";
  const Outputs a{index, r2};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_knn: ctx is NULL");
  if (bad_k(k)) return fail(NBX_ERR_ARG, "nbx_knn: k is outside [1, 16]");
  if ((long long)c->n * (long long)k > kKnnMaxEntries) return fail(NBX_ERR_ARG, "nbx_knn: n * k exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_knn: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_knn: a local step awaits nbx_commit");
  if (no_output(a)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? knn_ctx_t<float>(c, where, k, a) : knn_ctx_t<double>(c, where, k, a);
  });
}

int nbx_ensemble_knn(nbx_ensemble* e, int32_t first, int32_t count, int32_t k, int32_t* index, void* r2) {
  return batch_knn(e, "nbx_ensemble_knn", first, count, k, Outputs{index, r2});
}

int nbx_ragged_knn(nbx_ragged* r, int32_t first, int32_t count, int32_t k, int32_t* index, void* r2) {
  return batch_knn(r, "nbx_ragged_knn", first, count, k, Outputs{index, r2});
}

}  // extern "C"
