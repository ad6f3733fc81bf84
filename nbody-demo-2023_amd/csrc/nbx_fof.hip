// nbx_fof.hip -- nbx_fof, nbx_ensemble_fof and nbx_ragged_fof (include/nbx_fof.h) over the kernels of nbx_fof_kernels.hpp: the
// friends-of-friends groups of a context's state, or of every member of a range: per body the lowest index of its group and the
// group's size, per system the number of groups and the largest.
//
// A translation unit of its own: every other unit keeps its pinned kernel set, and the pair loop is compiled once for the three
// kinds.  The launch shape of a system is field_shape(n, n) (nbx_field_shape.hpp): the host evaluates it for a context and an
// ensemble, the device for every member of a ragged ensemble -- but nothing here depends on it: a partition with lowest-index
// labels is a function of the state alone.  The call iterates passes to a fixed point (the kernels' header says what a pass is)
// and reads one word back per pass.  It reads posm[cur] once, into staged records of its own, and writes fof_rec, fof_part,
// fof_work and fof_out: the trajectory, ke_part, have_parts, the profile and the cached graphs do not see it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/nbx_fof.h"
#include "nbx_analysis.hpp"           // ensure_bytes, range_bodies, ragged_member_table, ragged_extents
#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: check_range, check_uploaded, device_table
#include "nbx_fof_kernels.hpp"
#include "nbx_internal.hpp"         // struct nbx_ctx
#include "nbx_ragged_internal.hpp"  // struct nbx_ragged

using namespace nbx;
using namespace nbx_detail;

static_assert(sizeof(nbx_fof_info_t) == 2 * sizeof(int32_t), "the gather kernel writes {groups, largest} as two int32");

namespace {

struct Outputs {
  int32_t* label;
  int32_t* size;
  nbx_fof_info_t* info;
  int32_t* passes;
};

bool no_output(const Outputs& a) { return !a.label && !a.size && !a.info; }
bool bad_radius(double radius) { return !(radius >= 0.0); }  // NaN or negative

// h2 = fma(rT, rT, eps2), once, in T
template <typename T>
T radius2(double radius) {
  const T r = (T)radius;
  return std::fma(r, r, softening2<T>());
}

int padded(int n) { return (n + kTile - 1) / kTile * kTile; }
unsigned blocks_for(size_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

// What the three kinds share once the checks are through.  g: where the systems of the range lie; total / rec_total: its
// bodies / staged records; n_max: its largest system; launch(rec, parts): the kind's pair work over row_splits rows.
template <typename T, typename Launch>
int run_fof(Object* o, const char* where, const FofRange& g, size_t total, size_t rec_total, int row_splits, int n_max, const Outputs& a,
            Launch launch) {
  using T4 = typename V4<T>::type;
  const size_t count = (size_t)g.count;
  int rc = ensure_bytes(&o->fof_rec, &o->fof_rec_cap, sizeof(T4) * rec_total, where, "the staged records");
  if (rc) return rc;
  rc = ensure_bytes(&o->fof_part, &o->fof_part_cap, sizeof(int) * total * (size_t)row_splits, where, "the partials");
  if (rc) return rc;
  rc = ensure_bytes(&o->fof_work, &o->fof_work_cap, sizeof(int) * (4 * total + 2), where, "the labels");
  if (rc) return rc;
  rc = ensure_bytes(&o->fof_out, &o->fof_out_cap, sizeof(int) * (2 * total + 2 * count), where, "the results");
  if (rc) return rc;
  T4* rec = (T4*)o->fof_rec;
  int* parts = (int*)o->fof_part;
  int* lab = (int*)o->fof_work;
  int* nxt = lab + total;
  unsigned* slot = (unsigned*)(nxt + total);
  int* hist = nxt + 2 * total;
  int* changed = hist + total;  // [2]: pass p reports in word p & 1
  int* out = (int*)o->fof_out;
  const unsigned bodies = (unsigned)total;
  const dim3 per_body(blocks_for(total)), block(kBlock);
  const int rounds = fof_rounds(n_max);
  std::vector<int32_t> res(2 * total + 2 * count);
  int passes = 0;
  const int rc_run = [&]() -> int {
    hipLaunchKernelGGL(fof_init_kernel<T>, dim3(blocks_for(rec_total)), block, 0, o->stream, (const T4*)o->posm[o->cur], g, (unsigned)rec_total, rec,
                       lab, nxt, slot, changed);
    HIP_TRY(hipGetLastError());
    for (;;) {
      if (passes > n_max) return fail(NBX_ERR_INTERNAL, std::string(where) + ": the labels did not settle in n + 1 passes");
      int* word = changed + (passes & 1);
      launch(rec, parts);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(fof_hook_kernel, per_body, block, 0, o->stream, (const int*)parts, row_splits, bodies, (const int*)lab, nxt,
                         changed + ((passes + 1) & 1));
      for (int k = 0; k + 1 < rounds; ++k)
        hipLaunchKernelGGL((fof_shortcut_kernel<T, false>), per_body, block, 0, o->stream, bodies, lab, nxt, (const unsigned*)slot, rec, word);
      hipLaunchKernelGGL((fof_shortcut_kernel<T, true>), per_body, block, 0, o->stream, bodies, lab, nxt, (const unsigned*)slot, rec, word);
      HIP_TRY(hipGetLastError());
      int flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, word, sizeof(int), hipMemcpyDeviceToHost, o->stream));
      HIP_TRY(hipStreamSynchronize(o->stream));
      ++passes;
      if (!flag) break;
    }
    HIP_TRY(hipMemsetAsync(hist, 0, sizeof(int) * total, o->stream));
    HIP_TRY(hipMemsetAsync(out + 2 * total, 0, sizeof(int) * 2 * count, o->stream));
    hipLaunchKernelGGL(fof_count_kernel, per_body, block, 0, o->stream, bodies, (const int*)lab, hist);
    hipLaunchKernelGGL(fof_gather_kernel, per_body, block, 0, o->stream, g, bodies, (const int*)lab, (const int*)hist, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(res.data(), out, sizeof(int32_t) * res.size(), hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return NBX_OK;
  }();
  if (rc_run) {
    (void)hipStreamSynchronize(o->stream);  // no copy may outlive `res`
    return rc_run;
  }
  if (a.label) std::copy(res.begin(), res.begin() + total, a.label);
  if (a.size) std::copy(res.begin() + total, res.begin() + 2 * total, a.size);
  if (a.info)
    for (size_t k = 0; k < count; ++k) a.info[k] = nbx_fof_info_t{res[2 * total + 2 * k], res[2 * total + 2 * k + 1]};
  if (a.passes) *a.passes = passes;
  return NBX_OK;
}

template <typename T>
int fof_ctx_t(nbx_ctx* c, const char* where, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(c->n, c->n);
  const T h2 = radius2<T>(radius);
  const FofRange g{nullptr, 0u, 1, c->n, (unsigned)padded(c->n), 0u};
  return run_fof<T>(c, where, g, (size_t)c->n, (size_t)padded(c->n), s.splits, c->n, a, [&](const T4* rec, int* parts) {
    hipLaunchKernelGGL(fof_pass_kernel<T>, dim3(s.columns, s.splits), dim3(kBlock), 0, c->stream, rec, c->n, s.tiles_per_split, h2, parts);
  });
}

template <typename T>
int fof_members_t(nbx_ensemble* e, const char* where, int first, int count, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  const FieldShape s = field_shape(e->n, e->n);
  const unsigned stride = (unsigned)padded(e->n);
  const FofRange g{nullptr, (unsigned)first, count, e->n, stride, (unsigned)e->pos_stride};
  return run_fof<T>(e, where, g, (size_t)count * (size_t)e->n, (size_t)count * stride, s.splits, e->n, a, [&](const T4* rec, int* parts) {
    EnsembleFofArgs<T> k{};
    k.rec = rec;
    k.parts = parts;
    k.h2 = radius2<T>(radius);
    k.rec_stride = stride;
    k.n = e->n;
    k.tiles_per_split = s.tiles_per_split;
    hipLaunchKernelGGL(ensemble_fof_pass_kernel<T>, dim3(s.columns, s.splits, count), dim3(kBlock), 0, e->stream, k);
  });
}

// The member table is built and put on the device by the first call; the grid's x and y extents are the largest number of
// columns and of splits any member of the range has.
template <typename T>
int fof_members_t(nbx_ragged* r, const char* where, int first, int count, double radius, const Outputs& a) {
  using T4 = typename V4<T>::type;
  std::vector<FofMember> table;  // lives until run_fof has synchronised
  unsigned long long rec_off = 0;  // the staged records of the members before the one being made
  const int rc = ragged_member_table<FofMember>(r, &r->fof_tab, &table, where, [&](const MemberSpan& mem, unsigned long long out_off) {
    const FofMember entry{(unsigned long long)mem.pos_off, out_off, rec_off, mem.n, 0};
    rec_off += (unsigned long long)padded(mem.n);
    return entry;
  });
  if (rc) return rc;
  const GridExtents ext = ragged_extents(r, first, count);
  int n_max = 1;
  size_t rec_total = 0;
  for (int k = first; k < first + count; ++k) {
    const int n = r->layout(k).n;
    n_max = std::max(n_max, n);
    rec_total += (size_t)padded(n);
  }
  const size_t total = (size_t)range_bodies(r, first, count);
  const FofMember* dev = (const FofMember*)r->fof_tab;
  const FofRange g{dev, (unsigned)first, count, 0, 0u, 0u};
  return run_fof<T>(r, where, g, total, rec_total, ext.splits, n_max, a, [&](const T4* rec, int* parts) {
    RaggedFofArgs<T> k{};
    k.rec = rec;
    k.table = dev;
    k.parts = parts;
    k.h2 = radius2<T>(radius);
    k.first = (unsigned)first;
    k.total = (unsigned)total;
    hipLaunchKernelGGL(ragged_fof_pass_kernel<T>, dim3(ext.columns, ext.splits, count), dim3(kBlock), 0, r->stream, k);
  });
}

// nbx_ensemble_fof and nbx_ragged_fof: every check before the first HIP call, in the header's order
template <typename O>
int batch_fof(O* o, const char* where, int32_t first, int32_t count, double radius, const Outputs& a) {
  return guarded(where, [&]() -> int {
  if (!o) return fail(NBX_ERR_ARG, std::string(where) + ": " + O::names.noun + " is NULL");
  if (bad_radius(radius)) return fail(NBX_ERR_ARG, std::string(where) + ": radius is NaN or negative");
  int rc = check_range(o, where, first, count);
  if (rc) return rc;
  if (range_bodies(o, first, count) > kFofMaxBodies) return fail(NBX_ERR_ARG, std::string(where) + ": " + range_noun(o) + " 4194304");
  rc = check_uploaded(o, where, first, count);
  if (rc) return rc;
  if (count == 0 || no_output(a)) return NBX_OK;
  rc = use_device(o);
  if (rc) return rc;
  return o->precision == 32 ? fof_members_t<float>(o, where, first, count, radius, a) : fof_members_t<double>(o, where, first, count, radius, a);
  });
}

}  // namespace

extern "C" {

int nbx_fof(nbx_ctx* c, double radius, int32_t* label, int32_t* size, nbx_fof_info_t* info, int32_t* passes) {
  constexpr const char* where = "nbx_fof";
  const Outputs a{label, size, info, passes};
  return guarded(where, [&]() -> int {
  if (!c) return fail(NBX_ERR_ARG, "nbx_fof: ctx is NULL");
  if (bad_radius(radius)) return fail(NBX_ERR_ARG, "nbx_fof: radius is NaN or negative");
  if ((long long)c->n > kFofMaxBodies) return fail(NBX_ERR_ARG, "nbx_fof: n exceeds 4194304");
  if (!c->uploaded) return fail(NBX_ERR_STATE, "nbx_fof: nbx_upload has not been called");
  if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_fof: a local step awaits nbx_commit");
  if (no_output(a)) return NBX_OK;
  const int rc = use_device(c);
  if (rc) return rc;
  return c->precision == 32 ? fof_ctx_t<float>(c, where, radius, a) : fof_ctx_t<double>(c, where, radius, a);
  });
}

int nbx_ensemble_fof(nbx_ensemble* e, int32_t first, int32_t count, double radius, int32_t* label, int32_t* size, nbx_fof_info_t* info,
                     int32_t* passes) {
  return batch_fof(e, "nbx_ensemble_fof", first, count, radius, Outputs{label, size, info, passes});
}

int nbx_ragged_fof(nbx_ragged* r, int32_t first, int32_t count, double radius, int32_t* label, int32_t* size, nbx_fof_info_t* info,
                   int32_t* passes) {
  return batch_fof(r, "nbx_ragged_fof", first, count, radius, Outputs{label, size, info, passes});
}

}  // extern "C"
