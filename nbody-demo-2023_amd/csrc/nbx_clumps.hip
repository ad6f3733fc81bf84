// nbx_clumps.hip -- nbx_clumps, nbx_ensemble_clumps and nbx_ragged_clumps (include/nbx_clumps.h) over the kernels of
// nbx_clumps_kernels.hpp: for every body of a context's state, or of any range of members, under a caller-supplied label, the
// members, G m, centre and velocity of its clump, the potential of the clump's other members at the body and the body's specific
// energy in the clump's frame: one label upload, one pair-work launch, one finish launch and one read-back for all systems asked
// for.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it for a context and an
// ensemble, the device for every member of a ragged ensemble.  The call reads posm[cur] and velm and writes clump_lab, clump_part
// and clump_out, buffers of its own: the trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/nbx_clumps.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents, read_back
#include "nbx_clumps_kernels.hpp"
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_internal.hpp"           // struct nbx_ctx
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

namespace {

bool no_output(const nbx_clumps_out_t& a) {
  return !a.members && !a.gm && !a.centre[0] && !a.centre[1] && !a.centre[2] && !a.velocity[0] && !a.velocity[1] && !a.velocity[2] &&
         !a.phi && !a.energy;
}

// where the call's kernels find the state: a context's or a batch object's buffers
template <typename T>
struct Resident {
  const typename V4<T>::type* posm;
  const typename V4<T>::type* velm;
  const ClumpMember* table;  // a ragged ensemble's device table, else nullptr
  unsigned first;
  int count;
  int n_all;                 // table == nullptr: the bodies of every system
  unsigned pos_stride, vel_stride;
};

// The call's three buffers, before anything is enqueued: a failed allocation returns with nothing in flight.
template <typename T>
int reserve_clumps(Object* o, const char* where, size_t total, int row_splits) {
  using T4 = typename V4<T>::type;
  int rc = ensure_bytes(&o->clump_lab, &o->clump_lab_cap, sizeof(int) * total, where, "the labels");
  if (rc) return rc;
  rc = ensure_bytes(&o->clump_part, &o->clump_part_cap, (sizeof(T4) * 2 + sizeof(int)) * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  return ensure_bytes(&o->clump_out, &o->clump_out_cap, (sizeof(T4) * kClumpOutRecords + sizeof(int)) * total, where, "the results");
}

// What the three kinds share once the checks are through: upload the labels, `launch` the kind's pair work over `row_splits`
// rows per member, finish, read back, synchronise, scatter.  clump_part holds the partial records followed by the count rows,
// clump_out the result records followed by the members.
template <typename T, typename Launch>
int run_clumps(Object* o, const char* where, size_t total, int row_splits, const Resident<T>& res, const int32_t* label,
               const nbx_clumps_out_t& a, Launch launch) {
  using T4 = typename V4<T>::type;
  const size_t rows = total * (size_t)row_splits;
  const size_t out_bytes = (sizeof(T4) * kClumpOutRecords + sizeof(int)) * total;
  int rc = reserve_clumps<T>(o, where, total, row_splits);  // a ragged ensemble has them already: nothing happens
  if (rc) return rc;
  T4* parts = (T4*)o->clump_part;
  int* counts = (int*)(parts + 2 * rows);
  T4* out = (T4*)o->clump_out;
  int* members = (int*)(out + (size_t)kClumpOutRecords * total);
  std::vector<char> host(out_bytes);
  rc = read_back(o, host.data(), o->clump_out, out_bytes, [&]() -> int {
    HIP_TRY(hipMemcpyAsync(o->clump_lab, label, sizeof(int) * total, hipMemcpyHostToDevice, o->stream));
    launch((const int*)o->clump_lab, parts, counts);
    HIP_TRY(hipGetLastError());
    ClumpFinishArgs<T> f{};
    f.posm = res.posm;
    f.velm = res.velm;
    f.lab = (const int*)o->clump_lab;
    f.parts = parts;
    f.counts = counts;
    f.table = res.table;
    f.first = res.first;
    f.count = res.count;
    f.n_all = res.n_all;
    f.pos_stride = res.pos_stride;
    f.vel_stride = res.vel_stride;
    f.row_splits = row_splits;
    f.total = (unsigned)total;
    f.out = out;
    f.members = members;
    hipLaunchKernelGGL(clump_finish_kernel<T>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, o->stream, f);
    HIP_TRY(hipGetLastError());
    return NBX_OK;
  });
  if (rc) return rc;  // read_back has synchronised: no copy outlives `host` or still reads `label`
  const T* rec = (const T*)host.data();  // 12 values of T per body
  const int* mem = (const int*)(host.data() + sizeof(T4) * kClumpOutRecords * total);
  T* dst[9] = {(T*)a.gm, (T*)a.centre[0], (T*)a.centre[1], (T*)a.centre[2], (T*)a.velocity[0], (T*)a.velocity[1], (T*)a.velocity[2],
               (T*)a.phi, (T*)a.energy};
  for (int v = 0; v < 9; ++v)
    if (dst[v])
      for (size_t i = 0; i < total; ++i) dst[v][i] = rec[12 * i + (size_t)v];
  if (a.members)
    for (size_t i = 0; i < total; ++i) a.members[i] = mem[i];
  return NBX_OK;
}

template <typename T>
int clumps_ctx_t(nbx_ctx* c, const char* where, const int32_t* label, const nbx_clumps_out_t& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  const Resident<T> res{(const T4*)c->posm[c->cur], (const T4*)c->velm, nullptr, 0u, 1, c->n, 0u, 0u};
  return run_clumps<T>(c, where, (size_t)c->n, s.splits, res, label, a, [&](const int* lab, T4* parts, int* counts) {
    hipLaunchKernelGGL(clump_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, res.posm, res.velm, lab, c->n,
                       s.tiles_per_split, parts, counts);
  });
}

template <typename T>
int clumps_members_t(nbx_ensemble* e, const char* where, int first, int count, const int32_t* label, const nbx_clumps_out_t& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  const Resident<T> res{(const T4*)e->posm[e->cur], (const T4*)e->velm, nullptr, (unsigned)first, count, e->n, (unsigned)e->pos_stride,
                        (unsigned)e->own_pad};
  return run_clumps<T>(e, where, (size_t)count * (size_t)e->n, s.splits, res, label, a, [&](const int* lab, T4* parts, int* counts) {
    EnsembleClumpArgs<T> k{};
    k.posm = res.posm;
    k.velm = res.velm;
    k.lab = lab;
    k.parts = parts;
    k.counts = counts;
    k.first = (unsigned)first;
    k.pos_stride = res.pos_stride;
    k.vel_stride = res.vel_stride;
    k.n = e->n;
    k.tiles_per_split = s.tiles_per_split;
    hipLaunchKernelGGL(ensemble_clump_kernel<T>, dim3(s.columns, s.splits, count), dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has, a member's workgroups beyond its own return at once.
template <typename T>
int clumps_members_t(nbx_ragged* r, const char* where, int first, int count, const int32_t* label, const nbx_clumps_out_t& a) {
  using T4 = typename V4<T>::type;
  const GridExtents g = ragged_extents(r, first, count);
  const size_t total = (size_t)range_bodies(r, first, count);
  // every allocation of the call before the table's copy is enqueued: from there on every path ends in run_clumps'
  // synchronisation, which `table` outlives
  int rc = reserve_clumps<T>(r, where, total, g.splits);
  if (rc) return rc;
  std::vector<ClumpMember> table;
  // declared after `table`, so it runs first: if an exception (out of host memory) leaves this call while the table's copy is
  // in flight, the stream is drained before the vector goes
  struct Drain {
    hipStream_t stream;
    bool armed;
    ~Drain() { if (armed) (void)hipStreamSynchronize(stream); }
  } drain{r->stream, false};
  rc = ragged_member_table<ClumpMember>(r, &r->clump_tab, &table, where, [](const MemberSpan& mem, unsigned long long out_off) {
    return ClumpMember{{(unsigned long long)mem.pos_off, (unsigned long long)mem.vel_off, out_off, mem.n, 0}};
  });
  if (rc) return rc;  // nothing was enqueued
  drain.armed = !table.empty();  // this call has built the table: its copy is in flight
  const Resident<T> res{(const T4*)r->posm[r->cur], (const T4*)r->velm, (const ClumpMember*)r->clump_tab, (unsigned)first, count, 0, 0u, 0u};
  rc = run_clumps<T>(r, where, total, g.splits, res, label, a, [&](const int* lab, T4* parts, int* counts) {
    RaggedClumpArgs<T> k{};
    k.posm = res.posm;
    k.velm = res.velm;
    k.table = res.table;
    k.lab = lab;
    k.parts = parts;
    k.counts = counts;
    k.first = (unsigned)first;
    hipLaunchKernelGGL(ragged_clump_kernel<T>, dim3(g.columns, g.splits, count), dim3(kBlock), 0, r->stream, k);
  });
  drain.armed = false;  // run_clumps has synchronised on every path it returns by
  return rc;
}

// nbx_ensemble_clumps and nbx_ragged_clumps: every check before the first HIP call, in the header's order
template <typename O>
int batch_clumps(O* o, const char* where, int32_t first, int32_t count, const int32_t* label, const nbx_clumps_out_t* out) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (!label || !out) return fail(NBX_ERR_ARG, std::string(where) + ": label or out is NULL");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kClumpMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(*out)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? clumps_members_t<float>(o, where, first, count, label, *out)
                            : clumps_members_t<double>(o, where, first, count, label, *out);
  });
}

}  // namespace

extern "C" {

int nbx_clumps(nbx_ctx* c, const int32_t* label, const nbx_clumps_out_t* out) {
  constexpr const char* where = "nbx_clumps";
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_clumps: ctx is NULL");
  if (!label || !out) return fail(NBX_ERR_ARG, "nbx_clumps: label or out is NULL");
  if ((long long)c->n > kClumpMaxBodies) return fail(NBX_ERR_ARG, "nbx_clumps: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_clumps: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_clumps: a local step awaits nbx_commit");
  if (c->i_begin != 0 || c->i_count != c->n)
    return fail(NBX_ERR_STATE, "nbx_clumps: the context owns a slice of the bodies (the velocities of the others are not resident)");
  if (no_output(*out)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? clumps_ctx_t<float>(c, where, label, *out) : clumps_ctx_t<double>(c, where, label, *out);
  });
}

int nbx_ensemble_clumps(nbx_ensemble* e, int32_t first, int32_t count, const int32_t* label, const nbx_clumps_out_t* out) {
  return batch_clumps(e, "nbx_ensemble_clumps", first, count, label, out);
}

int nbx_ragged_clumps(nbx_ragged* r, int32_t first, int32_t count, const int32_t* label, const nbx_clumps_out_t* out) {
  return batch_clumps(r, "nbx_ragged_clumps", first, count, label, out);
}

}  // extern "C"
