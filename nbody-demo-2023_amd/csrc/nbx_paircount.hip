// nbx_paircount.hip -- nbx_paircount, nbx_ensemble_paircount and nbx_ragged_paircount (include/nbx_paircount.h) over the kernels
// of nbx_paircount_kernels.hpp: for a context's state, or for every member of any range, the number of pairs within each of a
// list of radii: ceil(nradii / 16) pair-work launches back to back, one finish launch, one read-back and one synchronisation
// for all systems asked for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set.  The launch shape of a system is
// field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it for a context and an ensemble, the device for every member of a
// ragged ensemble -- but nothing here depends on it: the results are integer sums.  The call reads posm[cur] and writes pc_part
// and pc_out, buffers of its own: the trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
//
// The counting scheme (nbx_paircount_kernels.hpp: lane counters or wave counters) is kPcDefaultWave, the faster of the two in
// profiles/paircount_cost.json; NBX_PAIRCOUNT_SCHEME=lane|wave, read per call, picks the other for experiments and for the test
// that holds the two to equal results.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nbx_paircount.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_paircount_kernels.hpp"
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

static_assert(NBX_PAIRCOUNT_MAX_RADII == kPcMaxRadii, "the header's bound is the kernels'");

namespace {

constexpr bool kPcDefaultWave = false;  // profiles/paircount_cost.json, context_n131072: lane_us against wave_us

bool wave_scheme() {
  if (const char* e = getenv("NBX_PAIRCOUNT_SCHEME")) {  // experiments
    if (!strcmp(e, "wave")) return true;
    if (!strcmp(e, "lane")) return false;
  }
  return kPcDefaultWave;
}

// statuses 2 and 3 of the header
int check_radii(const char* where, int32_t nradii, const double* radii) {
  if (nradii < 1 || nradii > kPcMaxRadii || !radii) return fail(NBX_ERR_ARG, std::string(where) + ": nradii is outside [1, 256] or radii is NULL");
  for (int k = 0; k < nradii; ++k)
    if (!(radii[k] >= 0.0)) return fail(NBX_ERR_ARG, std::string(where) + ": radii[" + std::to_string(k) + "] is NaN or negative");
  return NBX_OK;
}

// h2 = fma(rT, rT, eps2), once, in T
template <typename T>
T radius2(double radius) {
  const T r = (T)radius;
  return std::fma(r, r, softening2<T>());
}

// the radii of pass `pass` in the smallest E that holds them; unused slots carry -1
template <typename T, int E>
PcRadii<T, E> pass_radii(const double* radii, int nradii, int pass) {
  PcRadii<T, E> h;
  for (int k = 0; k < E; ++k) {
    const int g = pass * kPcSlots + k;
    h.h2[k] = g < nradii ? radius2<T>(radii[g]) : (T)-1;
  }
  return h;
}

// f(E, WAVE as integral constants) for the pass's instance
template <typename F>
void with_instance(int left, bool wave, F f) {
  auto by_scheme = [&](auto e) {
    if (wave) f(e, std::true_type{});
    else f(e, std::false_type{});
  };
  if (left <= 4) by_scheme(std::integral_constant<int, 4>{});
  else if (left <= 8) by_scheme(std::integral_constant<int, 8>{});
  else by_scheme(std::integral_constant<int, 16>{});
}

// What the three kinds share once the checks are through: per pass `launch(E, WAVE, pass, this pass's records of the first
// member, uint32 between members)`, then the finish, the read-back and the synchronisation.  table: the ragged ensemble's device
// table (nullptr: every system has n_all bodies).
template <typename Launch>
int run_paircount(Object* o, const char* where, int count, int nradii, int row_columns, int row_splits, const PcMember* table, unsigned first,
                  int n_all, uint64_t* counts, Launch launch) {
  const int passes = (nradii + kPcSlots - 1) / kPcSlots;
  const size_t pass_stride = (size_t)row_splits * (size_t)row_columns * kPcSlots, member_stride = pass_stride * (size_t)passes;
  const size_t total = (size_t)count * (size_t)nradii;
  int rc = ensure_bytes(&o->pc_part, &o->pc_part_cap, sizeof(unsigned) * member_stride * (size_t)count, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->pc_out, &o->pc_out_cap, sizeof(unsigned long long) * total, where, "the results");
  if (rc) return rc;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the device's counts are the caller's");
  const bool wave = wave_scheme();
  return read_back(o, counts, o->pc_out, sizeof(uint64_t) * total, [&]() -> int {
    for (int pass = 0; pass < passes; ++pass) {
      with_instance(nradii - pass * kPcSlots, wave,
                    [&](auto e, auto w) { launch(e, w, pass, (unsigned*)o->pc_part + (size_t)pass * pass_stride, member_stride); });
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(paircount_finish_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream,
                       (const unsigned*)o->pc_part, table, first, nradii, n_all, passes, row_splits, row_columns, (unsigned)total,
                       (unsigned long long*)o->pc_out);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
}

template <typename T>
int paircount_ctx_t(nbx_ctx* c, const char* where, int nradii, const double* radii, uint64_t* counts) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  return run_paircount(c, where, 1, nradii, s.columns, s.splits, nullptr, 0u, c->n, counts,
                       [&](auto e, auto w, int pass, unsigned* parts, size_t) {
                         constexpr int E = decltype(e)::value;
                         constexpr bool W = decltype(w)::value;
                         hipLaunchKernelGGL((paircount_kernel<T, E, W>), dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream,
                                            (const T4*)c->posm[c->cur], c->n, s.tiles_per_split, pass_radii<T, E>(radii, nradii, pass), parts);
                       });
}

template <typename T>
int paircount_members_t(nbx_ensemble* en, const char* where, int first, int count, int nradii, const double* radii, uint64_t* counts) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(en->n, en->n);
  return run_paircount(en, where, count, nradii, s.columns, s.splits, nullptr, (unsigned)first, en->n, counts,
                       [&](auto e, auto w, int pass, unsigned* parts, size_t member_stride) {
                         constexpr int E = decltype(e)::value;
                         constexpr bool W = decltype(w)::value;
                         EnsemblePcArgs<T, E> k{};
                         k.posm = (const T4*)en->posm[en->cur];
                         k.parts = parts;
                         k.member_stride = member_stride;
                         k.h = pass_radii<T, E>(radii, nradii, pass);
                         k.first = (unsigned)first;
                         k.pos_stride = (unsigned)en->pos_stride;
                         k.n = en->n;
                         k.tiles_per_split = s.tiles_per_split;
                         hipLaunchKernelGGL((ensemble_paircount_kernel<T, E, W>), dim3(s.columns, s.splits, count), dim3(kBlock), 0, en->stream, k);
                       });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int paircount_members_t(nbx_ragged* r, const char* where, int first, int count, int nradii, const double* radii, uint64_t* counts) {
  using T4 = typename V4<T>::type;
  std::vector<PcMember> table;  // lives until run_paircount has synchronised
  int rc = ragged_member_table<PcMember>(r, &r->pc_tab, &table, where, [](const MemberSpan& mem, unsigned long long) {
    return PcMember{{(unsigned long long)mem.pos_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count);
  const PcMember* dev = (const PcMember*)r->pc_tab;
  rc = run_paircount(r, where, count, nradii, g.columns, g.splits, dev, (unsigned)first, 0, counts,
                               [&](auto e, auto w, int pass, unsigned* parts, size_t member_stride) {
                                 constexpr int E = decltype(e)::value;
                                 constexpr bool W = decltype(w)::value;
                                 RaggedPcArgs<T, E> k{};
                                 k.posm = (const T4*)r->posm[r->cur];
                                 k.table = dev;
                                 k.parts = parts;
                                 k.member_stride = member_stride;
                                 k.h = pass_radii<T, E>(radii, nradii, pass);
                                 k.first = (unsigned)first;
                                 hipLaunchKernelGGL((ragged_paircount_kernel<T, E, W>), dim3(g.columns, g.splits, count), dim3(kBlock), 0, r->stream, k);
                               });
  if (rc && !table.empty()) (void)hipStreamSynchronize(r->stream);  // the table's copy may not outlive `table`
  return rc;
}

// nbx_ensemble_paircount and nbx_ragged_paircount: every check before the first HIP call, in the header's order
template <typename O>
int batch_paircount(O* o, const char* where, int32_t first, int32_t count, int32_t nradii, const double* radii, uint64_t* counts) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_radii(where, nradii, radii);
  if (rc) return rc;
  rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kPcMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || !counts) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? paircount_members_t<float>(o, where, first, count, nradii, radii, counts)
                            : paircount_members_t<double>(o, where, first, count, nradii, radii, counts);
  });
}

}  // namespace

extern "C" {

int nbx_paircount(nbx_ctx* c, int32_t nradii, const double* radii, uint64_t* counts) {
  constexpr const char* where = "nbx_paircount";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_paircount: ctx is NULL");
  int rc = check_radii(where, nradii, radii);
  if (rc) return rc;
  if ((long long)c->n > kPcMaxBodies) return fail(NBX_ERR_ARG, "nbx_paircount: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_paircount: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_paircount: a local step awaits nbx_commit");
  if (!counts) return NBX_OK;
  rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? paircount_ctx_t<float>(c, where, nradii, radii, counts) : paircount_ctx_t<double>(c, where, nradii, radii, counts);
  });
}

int nbx_ensemble_paircount(nbx_ensemble* e, int32_t first, int32_t count, int32_t nradii, const double* radii, uint64_t* counts) {
  return batch_paircount(e, "nbx_ensemble_paircount", first, count, nradii, radii, counts);
}

int nbx_ragged_paircount(nbx_ragged* r, int32_t first, int32_t count, int32_t nradii, const double* radii, uint64_t* counts) {
  return batch_paircount(r, "nbx_ragged_paircount", first, count, nradii, radii, counts);
}

}  // extern "C"
