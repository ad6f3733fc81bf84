// nbx_nlist.hip -- nbx_nlist, nbx_ensemble_nlist and nbx_ragged_nlist (include/nbx_nlist.h) over the kernels of
// nbx_nlist_kernels.hpp: for every body of a context's state, or of any range of members, the list of the bodies within a radius,
// in ascending index, with the softened squared distances, lists end to end behind an offsets array.
//
// The first call here whose output size depends on the state.  A call counts (one pair-work launch, a finish, three launches of a
// 64-bit prefix sum), reads offsets[] -- its last element is the total -- back into the caller's array and synchronises; where
// the lists fit the caller's capacity it sizes the device lists by the total, runs the pair work again to fill them, reads them
// back and synchronises again.  A translation unit of its own: every other unit keeps its pinned kernel set.  The launch shape
// of a system is field_shape(n, n); the segment rows depend on it, the lists do not.  The call reads posm[cur] and writes
// nl_seg, nl_scan, nl_index and nl_r2, buffers of its own: the trajectory, ke_part, have_parts, the profile and the cached graphs
// do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/nbx_nlist.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_nlist_kernels.hpp"
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

static_assert(sizeof(long long) == sizeof(int64_t), "offsets are scanned as long long and handed out as int64_t");

namespace {

struct Outputs {
  int64_t capacity;
  int64_t* offsets;
  int32_t* index;
  void* r2;
  int64_t* total;
};

bool bad_radius(double radius) { return !(radius >= 0.0); }  // NaN or negative

// statuses 2 to 4 of the header, the same for the three kinds
int check_args(const char* where, double radius, const Outputs& a) {
  if (bad_radius(radius)) return fail(NBX_ERR_ARG, std::string(where) + ": radius is NaN or negative");
  if (a.capacity < 0 || a.capacity > kNlMaxCapacity)
    return fail(NBX_ERR_ARG, std::string(where) + ": capacity is negative or exceeds 268435456 (3 GiB of device lists in fp64)");
  if (a.capacity > 0 && !a.index && !a.r2) return fail(NBX_ERR_ARG, std::string(where) + ": capacity > 0 but index and r2 are both NULL");
  if (!a.offsets || !a.total) return fail(NBX_ERR_ARG, std::string(where) + ": offsets or total is NULL");
  return NBX_OK;
}

// h2 = fma(rT, rT, eps2), once, in T
template <typename T>
T radius2(double radius) {
  const T r = (T)radius;
  return std::fma(r, r, softening2<T>());
}

// What the three kinds share once the checks are through.  bodies: of the call; table: the ragged ensemble's device table
// (nullptr: every system has n_all bodies); count(seg) and fill(seg, lists): the kind's pair work over `row_splits` rows per member.
template <typename T, typename Count, typename Fill>
int run_nlist(Object* o, const char* where, size_t bodies, int row_splits, const NlMember* table, unsigned first, int count, int n_all,
              const Outputs& a, Count count_pass, Fill fill_pass) {
  const int blocks = nl_scan_blocks((long long)bodies);
  int rc = ensure_bytes(&o->nl_seg, &o->nl_seg_cap, sizeof(NlSegment) * bodies * (size_t)row_splits, where, "the segments");
  if (rc) return rc;
  // within[bodies], offsets[bodies + 1], the block sums
  rc = ensure_bytes(&o->nl_scan, &o->nl_scan_cap, sizeof(long long) * (2 * bodies + 1 + (size_t)kNlScanBlock), where, "the offsets");
  if (rc) return rc;
  NlSegment* seg = (NlSegment*)o->nl_seg;
  long long* within = (long long*)o->nl_scan;
  long long* offsets = within + bodies;
  long long* sums = offsets + bodies + 1;
  const int rc_count = [&]() -> int {
    count_pass(seg);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nlist_finish_kernel, dim3((unsigned)((bodies + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream, seg, table, first, count,
                       n_all, row_splits, (unsigned)bodies, within);
    hipLaunchKernelGGL(nlist_scan_sums_kernel, dim3(blocks), dim3(kNlScanThreads), 0, o->stream, (const long long*)within, (long long)bodies, sums);
    hipLaunchKernelGGL(nlist_scan_blocks_kernel, dim3(1), dim3(kNlScanThreads), 0, o->stream, sums, blocks, offsets + bodies);
    hipLaunchKernelGGL(nlist_scan_apply_kernel, dim3(blocks), dim3(kNlScanThreads), 0, o->stream, (const long long*)within, (long long)bodies,
                       (const long long*)sums, offsets);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a.offsets, offsets, sizeof(int64_t) * (bodies + 1), hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return NBX_OK;
  }();
  if (rc_count) {
    (void)hipStreamSynchronize(o->stream);  // no copy may outlive the call
    return rc_count;
  }
  const int64_t total = a.offsets[bodies];
  *a.total = total;
  if (total > a.capacity || total == 0 || (!a.index && !a.r2)) return NBX_OK;
  // the device lists are sized by the total, never by the capacity
  rc = ensure_bytes(&o->nl_index, &o->nl_index_cap, sizeof(int) * (size_t)total, where, "the index lists");
  if (rc) return rc;
  rc = ensure_bytes(&o->nl_r2, &o->nl_r2_cap, sizeof(T) * (size_t)total, where, "the r2 lists");
  if (rc) return rc;
  const NlLists<T> lists{offsets, (int*)o->nl_index, (T*)o->nl_r2};
  const int rc_fill = [&]() -> int {
    fill_pass(seg, lists);
    HIP_TRY(hipGetLastError());
    if (a.index) HIP_TRY(hipMemcpyAsync(a.index, lists.index, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, o->stream));
    if (a.r2) HIP_TRY(hipMemcpyAsync(a.r2, lists.r2, sizeof(T) * (size_t)total, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return NBX_OK;
  }();
  if (rc_fill) (void)hipStreamSynchronize(o->stream);
  return rc_fill;
}

template <typename T>
int nlist_ctx_t(nbx_ctx* c, const char* where, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  const T h2 = radius2<T>(radius);
  const dim3 grid(s.columns, s.splits);
  const T4* posm = (const T4*)c->posm[c->cur];
  return run_nlist<T>(
      c, where, (size_t)c->n, s.splits, nullptr, 0u, 1, c->n, a,
      [&](NlSegment* seg) {
        hipLaunchKernelGGL((nlist_kernel<T, false>), grid, dim3(kBlock), 0, c->stream, posm, c->n, s.tiles_per_split, h2, seg, NlLists<T>{});
      },
      [&](NlSegment* seg, const NlLists<T>& lists) {
        hipLaunchKernelGGL((nlist_kernel<T, true>), grid, dim3(kBlock), 0, c->stream, posm, c->n, s.tiles_per_split, h2, seg, lists);
      });
}

template <typename T>
int nlist_members_t(nbx_ensemble* e, const char* where, int first, int count, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  EnsembleNlArgs<T> k{};
  k.posm = (const T4*)e->posm[e->cur];
  k.h2 = radius2<T>(radius);
  k.first = (unsigned)first;
  k.pos_stride = (unsigned)e->pos_stride;
  k.n = e->n;
  k.tiles_per_split = s.tiles_per_split;
  const dim3 grid(s.columns, s.splits, count);
  return run_nlist<T>(
      e, where, (size_t)count * (size_t)e->n, s.splits, nullptr, (unsigned)first, count, e->n, a,
      [&](NlSegment* seg) {
        k.seg = seg;
        hipLaunchKernelGGL((ensemble_nlist_kernel<T, false>), grid, dim3(kBlock), 0, e->stream, k, NlLists<T>{});
      },
      [&](NlSegment* seg, const NlLists<T>& lists) {
        k.seg = seg;
        hipLaunchKernelGGL((ensemble_nlist_kernel<T, true>), grid, dim3(kBlock), 0, e->stream, k, lists);
      });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int nlist_members_t(nbx_ragged* r, const char* where, int first, int count, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  std::vector<NlMember> table;  // lives until run_nlist has synchronised
  const int rc = ragged_member_table<NlMember>(r, &r->nl_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return NlMember{{(unsigned long long)mem.pos_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;
  const GridExtents g = ragged_extents(r, first, count);
  const NlMember* dev = (const NlMember*)r->nl_tab;
  RaggedNlArgs<T> k{};
  k.posm = (const T4*)r->posm[r->cur];
  k.table = dev;
  k.h2 = radius2<T>(radius);
  k.first = (unsigned)first;
  const dim3 grid(g.columns, g.splits, count);
  return run_nlist<T>(
      r, where, (size_t)range_bodies(r, first, count), g.splits, dev, (unsigned)first, count, 0, a,
      [&](NlSegment* seg) {
        k.seg = seg;
        hipLaunchKernelGGL((ragged_nlist_kernel<T, false>), grid, dim3(kBlock), 0, r->stream, k, NlLists<T>{});
      },
      [&](NlSegment* seg, const NlLists<T>& lists) {
        k.seg = seg;
        hipLaunchKernelGGL((ragged_nlist_kernel<T, true>), grid, dim3(kBlock), 0, r->stream, k, lists);
      });
}

// nbx_ensemble_nlist and nbx_ragged_nlist: every check before the first HIP call, in the header's order
template <typename O>
int batch_nlist(O* o, const char* where, int32_t first, int32_t count, double radius, const Outputs& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  int rc = check_args(where, radius, a);
  if (rc) return rc;
  rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kNlMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0) {
    a.offsets[0] = 0;
    *a.total = 0;
    return NBX_OK;
  }
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? nlist_members_t<float>(o, where, first, count, radius, a) : nlist_members_t<double>(o, where, first, count, radius, a);
  });
}

}  // namespace

extern "C" {

int nbx_nlist(nbx_ctx* c, double radius, int64_t capacity, int64_t* offsets, int32_t* index, void* r2, int64_t* total) {
  constexpr const char* where = "nbx_nlist";
  const Outputs a{capacity, offsets, index, r2, total};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_nlist: ctx is NULL");
  int rc = check_args(where, radius, a);
  if (rc) return rc;
  if ((long long)c->n > kNlMaxBodies) return fail(NBX_ERR_ARG, "nbx_nlist: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_nlist: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_nlist: a local step awaits nbx_commit");
  rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? nlist_ctx_t<float>(c, where, radius, a) : nlist_ctx_t<double>(c, where, radius, a);
  });
}

int nbx_ensemble_nlist(nbx_ensemble* e, int32_t first, int32_t count, double radius, int64_t capacity, int64_t* offsets, int32_t* index, void* r2,
                       int64_t* total) {
  return batch_nlist(e, "nbx_ensemble_nlist", first, count, radius, Outputs{capacity, offsets, index, r2, total});
}

int nbx_ragged_nlist(nbx_ragged* r, int32_t first, int32_t count, double radius, int64_t capacity, int64_t* offsets, int32_t* index, void* r2,
                     int64_t* total) {
  return batch_nlist(r, "nbx_ragged_nlist", first, count, radius, Outputs{capacity, offsets, index, r2, total});
}

}  // extern "C"
