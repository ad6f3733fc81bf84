// nbx_group.hip -- multi-GPU drivers of include/nbx.h over the contexts of nbx_api.hip: one process with k GPUs
// (nbx_group_create) and one process per GPU (nbx_comm_unique_id + nbx_group_create_rank), both exchanging the freshly
// integrated position blocks with one in-place RCCL all-gather per time step.  Replaces init_mpi + mpi_bcast_all +
// mpi_gather_acc of the reference (ver5_all/GSimulation.cpp:93-115,170-214) and its OpenCL multi-device loop
// (opencl/Compute.cpp:241-284).  The driver only: who owns what and when a retune moves it is decided in nbx_shares.hpp (host-only).
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is dlopen'ed (struct Rccl), never linked

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nbx_kick.h"  // nbx_kick, nbx_group_kick
#include "nbx_internal.hpp"
#include "nbx_shares.hpp"  // who owns what, and the tuner: all the arithmetic of this file
#include "nbx_watchdog.hpp"

using namespace nbx_detail;

// a call of the library's own that failed ends the caller with its code; its text is in last_error() already (HIP_TRY's sibling)
#define NBX_TRY(expr) do { const int rc_ = (expr); if (rc_ != NBX_OK) return rc_; } while (0)

namespace {
constexpr double kRcclInitAllowanceSeconds = 30.0;  // added to the collective timeout for ncclCommInitRank (see there)
}  // namespace

// =============================================================================================
// nbx_group: single-process multi-GPU driver (see include/nbx.h)
// =============================================================================================
namespace {

// The RCCL entry points used, resolved at run time so libnbx.so has no link-time dependency on librccl (and binds to
// the copy already in the process when a host such as PyTorch brought its own).  Every pointer takes its type from
// rccl.h's own prototype (decltype), so a signature or enum change in the header is a compile error here, not a
// silent ABI mismatch at the first multi-GPU run.
struct Rccl {
  typedef ncclComm_t comm_t;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;  // weighted groups: blocks of unequal size, one broadcast per owner
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  bool ok = false;
  template <typename F> static void sym(void* h, const char* name, F& fn) { fn = reinterpret_cast<F>(dlsym(h, name)); }
  bool load() {
    if (ok) return true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    sym(h, "ncclCommInitAll", CommInitAll);
    sym(h, "ncclCommInitRank", CommInitRank);
    sym(h, "ncclGetUniqueId", GetUniqueId);
    sym(h, "ncclCommDestroy", CommDestroy);
    sym(h, "ncclGroupStart", GroupStart);
    sym(h, "ncclGroupEnd", GroupEnd);
    sym(h, "ncclAllGather", AllGather);
    sym(h, "ncclBroadcast", Broadcast);
    sym(h, "ncclGetErrorString", GetErrorString);
    ok = CommInitAll && CommInitRank && GetUniqueId && CommDestroy && GroupStart && GroupEnd && AllGather && Broadcast;
    return ok;
  }
  std::string text(ncclResult_t e) const { return GetErrorString ? std::string(GetErrorString(e)) : std::string("RCCL error ") + std::to_string((int)e); }
};
Rccl g_rccl;
static_assert(std::is_same<decltype(Rccl::AllGather), ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)>::value,
              "ncclAllGather is called as (send, recv, bytes, ncclChar, comm, stream)");
static_assert(kExitCollectiveTimeout == NBX_EXIT_COLLECTIVE_TIMEOUT, "include/nbx.h documents the watchdog's exit status");
static_assert(sizeof(ncclUniqueId) == NBX_UNIQUE_ID_BYTES, "include/nbx.h promises callers the size of the rendezvous token");

}  // namespace

struct nbx_group {
  int n = 0, precision = 32;
  nbx::Shares own;                   // rank r owns [own.begin[r], own.begin[r] + own.count[r]) (nbx_shares.hpp)
  int my_rank = -1;                  // >= 0: one-process-per-GPU group (nbx_group_create_rank): `rank` holds this process's context only
  std::vector<nbx_ctx*> rank;
  std::vector<int> dev;
  std::vector<hipEvent_t> done;      // rank r's NEXT block is complete (copy path)
  std::vector<Rccl::comm_t> comm;    // RCCL path
  bool use_rccl = false;
  double* ke_all = nullptr;          // rank groups: [ranks] sum m v^2 of every rank, all-gathered
  double* diag_all = nullptr;        // rank groups, nbx_group_diagnostics: [ranks][kDiagFields] raw sums of every rank, all-gathered
  void* vel_stage = nullptr;         // rank groups, nbx_group_download: own velocities padded to `block` records
  void* vel_all = nullptr;           //   and the all-gathered [ranks * block] records
  // watchdog bookkeeping (nbx_watchdog.hpp): steps enqueued since the last host synchronisation, and what one step took
  long long steps_unsynced = 0;
  double step_s_est = 0.0;           // seconds per step measured over the last fully synchronised nbx_group_step call; 0 = not yet
  // weighted groups (nbx_group_create_weighted): whole 256-record tiles in proportion to the ranks' weights; the per-step exchange
  // is one broadcast per owner instead of the equal-block all-gather
  bool weighted = false;
  nbx::Tuner tuner;                  // nbx_group_retune accepts improvements only: what it remembers between calls
  nbx_opts opts{};                   // launch-shape options the contexts were made with (nbx_group_retune rebuilds them)
  std::vector<char> mass_host;       // the masses as uploaded (n elements of the group's precision): needed to re-upload after a retune
  bool uploaded = false;
  long long retunes = 0;
  bool broken = false;               // a retune failed half-way (contexts could not be rebuilt): only nbx_group_destroy is left
};

namespace {

// Seconds of legitimately queued work in front of a synchronisation: the watchdog's deadline is its timeout PLUS this, so
// that a long print window is not mistaken for a dead peer.  Four times the measured step time once a window has been
// timed; before that a rate no shape is slower than (2e10 pair/s: the validation kernel runs at ~5e11).
double queued_allowance(const nbx_group* g) {
  if (g->steps_unsynced <= 0 || g->rank.empty()) return 0.0;
  double per_step = 4.0 * g->step_s_est;
  if (!(per_step > 0.0)) {
    per_step = 1e-3;
    for (const nbx_ctx* c : g->rank) per_step += (double)c->i_count * (double)c->n / 2e10;  // logical ranks may share a GPU: add them up
  }
  return per_step * (double)g->steps_unsynced;
}

// the host has waited for everything the group enqueued, however the call ends
struct Synced { nbx_group* g; ~Synced() { g->steps_unsynced = 0; } };
// the rank whose context g->rank[k] is: a rank group holds this process's only
int rank_of(const nbx_group* g, size_t k) { return g->my_rank >= 0 ? g->my_rank : (int)k; }

// What the entry points ask of the group before they touch it, reported in this order: it is there, no retune left it without
// its contexts, a state has been uploaded.
enum : int { IS_THERE = 1, HAS_CONTEXTS = 2, HAS_STATE = 4 };
int need(const nbx_group* g, const char* who, int what, const char* which_retune = "a") {
  if ((what & IS_THERE) && !g) return fail(NBX_ERR_ARG, std::string(who) + ": group is NULL");
  if ((what & HAS_CONTEXTS) && g->broken)
    return fail(NBX_ERR_STATE, std::string(who) + ": " + which_retune + " retune failed while rebuilding the contexts; destroy the group");
  if ((what & HAS_STATE) && !g->uploaded) return fail(NBX_ERR_STATE, std::string(who) + ": nbx_group_upload has not been called");
  return NBX_OK;
}

int rccl_fail(const char* what, ncclResult_t e) { return fail(NBX_ERR_DEVICE, std::string(what) + ": " + g_rccl.text(e)); }

// One RCCL group over the contexts of this process: each(k, c, buf) enqueues the collectives of g->rank[k] = c on its stream, buf
// being the position records it exchanges in place.  Once the group is open every path reaches ncclGroupEnd: an early return
// would leave RCCL in group mode for the rest of the process.
template <typename Each>
int rccl_group(nbx_group* g, Each each) {
  ncclResult_t e = g_rccl.GroupStart();
  if (e != ncclSuccess) return rccl_fail("ncclGroupStart", e);
  int rc = NBX_OK;
  for (size_t k = 0; k < g->rank.size() && rc == NBX_OK; ++k) {
    nbx_ctx* c = g->rank[k];
    const hipError_t he = hipSetDevice(g->dev[k]);
    if (he != hipSuccess) { rc = fail(NBX_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(he)); break; }
    rc = each(k, c, (char*)c->posm[c->cur ^ 1]);
  }
  e = g_rccl.GroupEnd();
  if (rc == NBX_OK && e != ncclSuccess) rc = rccl_fail("ncclGroupEnd", e);
  return rc;
}

int group_exchange(nbx_group* g) {
  const size_t rec = g->rank[0]->rec;
  const nbx::Shares& own = g->own;
  if (g->use_rccl && g->weighted)  // blocks of unequal size: one in-place broadcast per owner, all of them in one group (single-process groups only)
    return rccl_group(g, [&](size_t k, nbx_ctx* c, char* buf) -> int {
      for (int r = 0; r < own.ranks; ++r) {
        char* blk = buf + (size_t)own.begin[r] * rec;
        const ncclResult_t e = g_rccl.Broadcast(blk, blk, (size_t)own.count[r] * rec, ncclChar, r, g->comm[k], c->stream);
        if (e != ncclSuccess) return rccl_fail("ncclBroadcast", e);
      }
      return NBX_OK;
    });
  if (g->use_rccl)  // in place: rank r sends its own block, receives every block at its natural offset
    return rccl_group(g, [&](size_t k, nbx_ctx* c, char* buf) -> int {
      const ncclResult_t e = g_rccl.AllGather(buf + (size_t)rank_of(g, k) * own.block * rec, buf, (size_t)own.block * rec, ncclChar, g->comm[k], c->stream);
      return e == ncclSuccess ? NBX_OK : rccl_fail("ncclAllGather", e);
    });
  // copy path: every destination pulls every other rank's block, stream-ordered behind the producer's event
  for (int r = 0; r < own.ranks; ++r) {
    HIP_TRY(hipSetDevice(g->dev[r]));
    HIP_TRY(hipEventRecord(g->done[r], g->rank[r]->stream));
  }
  for (int q = 0; q < own.ranks; ++q) {
    nbx_ctx* dst = g->rank[q];
    HIP_TRY(hipSetDevice(g->dev[q]));
    for (int r = 0; r < own.ranks; ++r) {
      if (r == q) continue;
      nbx_ctx* src = g->rank[r];
      const size_t off = (size_t)src->i_begin * rec, bytes = (size_t)src->i_count * rec;
      HIP_TRY(hipStreamWaitEvent(dst->stream, g->done[r], 0));
      char* d = (char*)dst->posm[dst->cur ^ 1] + off;
      const char* s = (const char*)src->posm[src->cur ^ 1] + off;
      if (g->dev[q] == g->dev[r]) HIP_TRY(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, dst->stream));
      else HIP_TRY(hipMemcpyPeerAsync(d, g->dev[q], s, g->dev[r], bytes, dst->stream));
    }
  }
  return NBX_OK;
}

// Rank groups: `bytes` from `row` on every rank's device, all-gathered into `all` ([ranks] rows of that size), the first host_bytes
// of them copied to `host`; synchronises.  Every rank then holds the same rows and adds them up in rank order -- the same number
// on every rank, independent of arrival order.
int gather_rows(nbx_group* g, const void* row, size_t bytes, void* all, void* host, size_t host_bytes, const char* what) {
  nbx_ctx* c = g->rank[0];
  const ncclResult_t e = g_rccl.AllGather(row, all, bytes, ncclChar, g->comm[0], c->stream);
  if (e != ncclSuccess) return rccl_fail(what, e);
  HIP_TRY(hipMemcpyAsync(host, all, host_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return NBX_OK;
}

// sum m v^2 over the ranks from the partials their last step or kick left behind, added in rank order; synchronises every stream
// of this process.  The caller has armed the watchdog: for a rank group this is a collective.
int group_sum_mv2(nbx_group* g, double* out) {
  double sum = 0.0;
  if (g->my_rank >= 0) {
    // one process per GPU: every rank reduces its partial on the device, one 8-byte all-gather, and all ranks add the values
    nbx_ctx* c = g->rank[0];
    NBX_TRY(use_device(c));
    if (c->ke_parts > 0) NBX_TRY(enqueue_ke_reduce(c, 0));
    else HIP_TRY(hipMemsetAsync(c->ke_dev, 0, sizeof(double), c->stream));
    std::vector<double> parts((size_t)g->own.ranks);
    NBX_TRY(gather_rows(g, c->ke_dev, sizeof(double), g->ke_all, parts.data(), sizeof(double) * parts.size(), "ncclAllGather(kenergy)"));
    for (double p : parts) sum += p;
  } else {
    for (nbx_ctx* c : g->rank) {  // rank order: deterministic
      double part = 0.0;
      NBX_TRY(nbx_kenergy_partial(c, &part));
      sum += part;
    }
    for (nbx_ctx* c : g->rank) NBX_TRY(nbx_sync(c));  // the exchange copies of the last step must have landed too
  }
  *out = sum;
  return NBX_OK;
}

// n records -> up to three host arrays (a NULL one is skipped)
template <typename T4, typename T>
void unpack_xyz(const T4* q, int n, T* x, T* y, T* z) {
  for (int i = 0; i < n; ++i) {
    if (x) x[i] = q[i].x;
    if (y) y[i] = q[i].y;
    if (z) z[i] = q[i].z;
  }
}

// The checks of both constructors in the order their errors are reported in -- out, n, the rank count, precision, then the options
// -- and the options every rank's context is made with.
int group_opts(const char* who, nbx_group** out, int n, int precision, int n_ranks, const nbx_opts* opts, nbx_opts* o) {
  if (!out) return fail(NBX_ERR_ARG, std::string(who) + ": out is NULL");
  *out = nullptr;
  if (n <= 0) return fail(NBX_ERR_ARG, std::string(who) + ": n must be > 0");
  if (n_ranks <= 0 || n_ranks > 64) return fail(NBX_ERR_ARG, std::string(who) + ": the number of ranks must be in 1..64");
  if (precision != 32 && precision != 64) return fail(NBX_ERR_ARG, std::string(who) + ": precision must be 32 or 64");
  const int rc = create_opts(who, out, opts, o);
  o->stream = nullptr; o->external_stream = 0; o->use_graph = 2;  // every rank: own stream, plain launches (and its device: set per rank)
  return rc;
}

// the devices there are, or the refusal every constructor gives without one
int device_count(const char* who, int* ndev) {
  if (hipGetDeviceCount(ndev) == hipSuccess && *ndev > 0) return NBX_OK;
  return fail(NBX_ERR_DEVICE, std::string(who) + ": no HIP device available (libnbx has no CPU path)");
}

// one rank's context: its slice of the group's shares on its device
int make_context(nbx_group* g, const char* who, int r, int dev) {
  nbx_opts o = g->opts;
  o.device = dev;
  o.i_begin = g->own.begin[r];
  o.i_count = g->own.count[r];
  o.n_alloc = g->own.n_alloc;
  nbx_ctx* c = nullptr;
  const int rc = nbx_create(&c, g->n, g->precision, &o);
  if (rc != NBX_OK) { const std::string m = last_error(); return fail(rc, std::string(who) + ": rank " + std::to_string(r) + ": " + m); }
  g->rank.push_back(c);
  return NBX_OK;
}

// (re)creates the contexts of a single-process group from g->own
int make_contexts(nbx_group* g, const char* who) {
  for (nbx_ctx* c : g->rank) nbx_destroy(c);
  g->rank.clear();
  for (int r = 0; r < g->own.ranks; ++r) {
    NBX_TRY(make_context(g, who, r, g->dev[r]));
    if (g->weighted) NBX_TRY(nbx_profile(g->rank.back(), 1));  // per-launch timing of the force kernel: what nbx_group_retune weighs the ranks by
  }
  return NBX_OK;
}

int create_single_process(const char* who, nbx_group** out, int n, int precision, int n_ranks, const int32_t* devices, bool weighted, const double* weights, const nbx_opts* opts) {
  nbx_opts o;
  NBX_TRY(group_opts(who, out, n, precision, n_ranks, opts, &o));
  int ndev = 0;
  NBX_TRY(device_count(who, &ndev));
  nbx_group* g = new (std::nothrow) nbx_group();
  if (!g) return fail(NBX_ERR_ALLOC, std::string(who) + ": out of host memory");
  BatchOwner<nbx_group> owner{nbx_group_destroy, g};  // every failure path below frees the group
  g->n = n; g->precision = precision; g->opts = o; g->weighted = weighted;
  if (weighted) {
    const char* msg = "";
    const int rc = nbx::weighted_shares(n, n_ranks, weights, &g->own, &msg);
    if (rc) return fail(rc, std::string(who) + ": " + msg);
    for (int r = 0; r < g->own.ranks; ++r) g->tuner.weight.push_back(weights ? weights[r] : 1.0);
  } else {
    g->own = nbx::equal_shares(n, n_ranks);
  }
  const int P = g->own.ranks;
  bool distinct = true;
  for (int r = 0; r < P; ++r) {
    const int d = devices ? devices[r] : r % ndev;
    if (d < 0 || d >= ndev) return fail(NBX_ERR_ARG, std::string(who) + ": device ordinal out of range");
    for (int q : g->dev) distinct = distinct && q != d;
    g->dev.push_back(d);
  }
  NBX_TRY(make_contexts(g, who));
  const char* force = std::getenv("NBX_EXCHANGE");  // "copy" forces the peer-copy path, "rccl" insists on RCCL
  const bool insist = force && !std::strcmp(force, "rccl");  // also with a single rank: smoke-tests the RCCL binding
  const bool want_rccl = distinct && (P > 1 || insist) && !(force && !std::strcmp(force, "copy"));
  if (want_rccl && g_rccl.load()) {
    g->comm.assign(P, nullptr);
    const ncclResult_t e = g_rccl.CommInitAll(g->comm.data(), P, g->dev.data());
    if (e == ncclSuccess) g->use_rccl = true;
    else g->comm.clear();
  }
  if (insist && !g->use_rccl)
    return fail(NBX_ERR_DEVICE, std::string(who) + ": NBX_EXCHANGE=rccl but RCCL is unavailable for these devices");
  if (!g->use_rccl) {
    g->done.assign(P, nullptr);
    for (int r = 0; r < P; ++r) {
      if (hipSetDevice(g->dev[r]) != hipSuccess || hipEventCreateWithFlags(&g->done[r], hipEventDisableTiming) != hipSuccess)
        return fail(NBX_ERR_DEVICE, std::string(who) + ": hipEventCreate failed");
      for (int q = 0; q < P; ++q)  // best effort: direct peer access speeds hipMemcpyPeerAsync up
        if (g->dev[q] != g->dev[r]) { (void)hipDeviceEnablePeerAccess(g->dev[q], 0); (void)hipGetLastError(); }
    }
  }
  *out = owner.release();
  last_error().clear();
  return NBX_OK;
}

// what nbx_partition and nbx_partition_weighted tell rank `rank` of shares `s`; a dropped rank owns nothing and takes no part
void report_share(const nbx::Shares& s, int n, int rank, int32_t* ranks_used, int32_t* i_begin, int32_t* i_count, int32_t* n_alloc) {
  if (ranks_used) *ranks_used = s.ranks;
  if (i_begin) *i_begin = rank < s.ranks ? s.begin[rank] : n;
  if (i_count) *i_count = rank < s.ranks ? s.count[rank] : 0;
  if (n_alloc) *n_alloc = s.n_alloc;
}

// restart the measurement window of every rank
int restart_timing(nbx_group* g) {
  for (nbx_ctx* x : g->rank) {
    NBX_TRY(nbx_profile(x, 0));
    NBX_TRY(nbx_profile(x, 1));
  }
  return NBX_OK;
}

// Shares move: velocities live with their owners, so the state goes through the host once -- positions from rank 0 (every rank holds
// them all), velocities from each owner -- and comes back to contexts with the new slices.  Values are copied, never recomputed: the
// trajectory is the same bit for bit in reference summation order, whoever owns a body (tests compare).
int move_shares(nbx_group* g, const nbx::Shares& next) {
  const size_t es = g->precision == 32 ? sizeof(float) : sizeof(double);
  std::vector<char> h(6 * es * (size_t)g->n);
  char* a[6];
  for (int k = 0; k < 6; ++k) a[k] = h.data() + (size_t)k * es * (size_t)g->n;
  NBX_TRY(nbx_group_download(g, a[0], a[1], a[2], a[3], a[4], a[5]));
  g->own = next;
  g->broken = true;  // until every new context exists and holds the state
  NBX_TRY(make_contexts(g, "nbx_group_retune"));
  for (nbx_ctx* x : g->rank) NBX_TRY(nbx_upload(x, a[0], a[1], a[2], a[3], a[4], a[5], g->mass_host.data()));
  g->broken = false;
  g->steps_unsynced = 0;
  g->step_s_est = 0.0;
  g->retunes += 1;
  return NBX_OK;
}

}  // namespace

extern "C" {

int nbx_partition(int32_t n, int32_t n_ranks, int32_t rank, int32_t* ranks_used, int32_t* block, int32_t* i_begin, int32_t* i_count, int32_t* n_alloc) {
  return guarded("nbx_partition", [&]() -> int {
  if (n <= 0 || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return fail(NBX_ERR_ARG, "nbx_partition: need n > 0 and 0 <= rank < n_ranks");
  const nbx::Shares s = nbx::equal_shares(n, n_ranks);
  if (block) *block = s.block;
  report_share(s, n, rank, ranks_used, i_begin, i_count, n_alloc);
  return NBX_OK;
  });
}

int nbx_partition_weighted(int32_t n, int32_t n_ranks, const double* weights, int32_t rank, int32_t* ranks_used, int32_t* i_begin, int32_t* i_count, int32_t* n_alloc) {
  return guarded("nbx_partition_weighted", [&]() -> int {
  if (n <= 0 || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return fail(NBX_ERR_ARG, "nbx_partition_weighted: need n > 0 and 0 <= rank < n_ranks");
  nbx::Shares s;
  const char* msg = "";
  const int rc = nbx::weighted_shares(n, n_ranks, weights, &s, &msg);
  if (rc) return fail(rc, std::string("nbx_partition_weighted: ") + msg);
  report_share(s, n, rank, ranks_used, i_begin, i_count, n_alloc);
  return NBX_OK;
  });
}

int nbx_tune_weights(int32_t n_ranks, const int32_t* i_count, const double* force_ms, double* weights_out) {
  return guarded("nbx_tune_weights", [&]() -> int {
  const char* msg = "";
  const int rc = nbx::tune_weights(n_ranks, i_count, force_ms, weights_out, &msg);
  return rc ? fail(rc, msg) : NBX_OK;
  });
}

int nbx_group_create(nbx_group** out, int32_t n, int32_t precision, int32_t n_ranks, const int32_t* devices, const nbx_opts* opts) {
  return guarded("nbx_group_create", [&]() -> int { return create_single_process("nbx_group_create", out, n, precision, n_ranks, devices, false, nullptr, opts); });
}

int nbx_group_create_weighted(nbx_group** out, int32_t n, int32_t precision, int32_t n_ranks, const int32_t* devices, const double* weights, const nbx_opts* opts) {
  return guarded("nbx_group_create_weighted", [&]() -> int { return create_single_process("nbx_group_create_weighted", out, n, precision, n_ranks, devices, true, weights, opts); });
}

int nbx_group_shares(nbx_group* g, int32_t* i_begin, int32_t* i_count, double* force_ms) {
  return guarded("nbx_group_shares", [&]() -> int {
  NBX_TRY(need(g, "nbx_group_shares", IS_THERE | HAS_CONTEXTS));
  for (int r = 0; r < g->own.ranks; ++r) {
    if (i_begin) i_begin[r] = g->own.begin[r];
    if (i_count) i_count[r] = g->own.count[r];
  }
  if (force_ms) {
    for (int r = 0; r < g->own.ranks; ++r) force_ms[r] = 0.0;
    for (size_t k = 0; k < g->rank.size(); ++k) {
      nbx_stats_t st;
      NBX_TRY(nbx_stats(g->rank[k], &st));  // synchronises this rank's stream and drains its events
      force_ms[rank_of(g, k)] = st.force_launches_timed > 0 ? st.force_ms_total / (double)st.force_launches_timed : 0.0;
    }
  }
  return NBX_OK;
  });
}

// measure, decide (nbx::tune_shares), then restart the measurement windows or move the shares
int nbx_group_retune(nbx_group* g, const double* force_ms, int32_t* changed) {
  return guarded("nbx_group_retune", [&]() -> int {
  if (changed) *changed = 0;
  NBX_TRY(need(g, "nbx_group_retune", IS_THERE));
  if (!g->weighted || g->my_rank >= 0) return fail(NBX_ERR_STATE, "nbx_group_retune: needs a single-process group made by nbx_group_create_weighted");
  NBX_TRY(need(g, "nbx_group_retune", HAS_CONTEXTS | HAS_STATE, "an earlier"));
  std::vector<double> ms((size_t)g->own.ranks);
  if (force_ms) {
    ms.assign(force_ms, force_ms + g->own.ranks);
  } else {
    NBX_TRY(nbx_group_shares(g, nullptr, nullptr, ms.data()));
    for (double t : ms)
      if (!(t > 0.0)) return NBX_OK;  // a rank without a timed launch since the last retune: nothing to weigh by, shares stay
  }
  nbx::Shares next;
  const char* msg = "";
  const int verdict = nbx::tune_shares(&g->tuner, g->own, g->n, ms.data(), [g](int r, int own) { return model_force_cost(g->rank[(size_t)r], own); }, &next, &msg);
  if (verdict < 0) return fail(verdict, msg);
  if (verdict == nbx::SHARES_KEEP) return restart_timing(g);  // whether or not the shares move, a new window starts
  NBX_TRY(move_shares(g, next));
  if (changed) *changed = 1;
  return NBX_OK;
  });
}

int nbx_comm_unique_id(void* id_out) {
  return guarded("nbx_comm_unique_id", [&]() -> int {
  if (!id_out) return fail(NBX_ERR_ARG, "nbx_comm_unique_id: id_out is NULL");
  if (!g_rccl.load()) return fail(NBX_ERR_DEVICE, "nbx_comm_unique_id: librccl could not be loaded");
  ncclUniqueId id;
  const ncclResult_t e = g_rccl.GetUniqueId(&id);
  if (e != ncclSuccess) return rccl_fail("ncclGetUniqueId", e);
  std::memcpy(id_out, &id, sizeof id);
  return NBX_OK;
  });
}

int nbx_group_create_rank(nbx_group** out, int32_t n, int32_t precision, int32_t world, int32_t rank, const void* unique_id, int32_t device, const nbx_opts* opts) {
  constexpr const char* who = "nbx_group_create_rank";
  return guarded(who, [&]() -> int {
  nbx_opts o;
  NBX_TRY(group_opts(who, out, n, precision, world, opts, &o));
  if (rank < 0 || rank >= world) return fail(NBX_ERR_ARG, "nbx_group_create_rank: rank must be in [0, world)");
  if (!unique_id) return fail(NBX_ERR_ARG, "nbx_group_create_rank: unique_id is NULL");
  nbx::Shares own = nbx::equal_shares(n, world);
  const int P = own.ranks;
  // every rank computes the same P: a world too large for n is refused by ALL ranks alike (nobody is left waiting in a collective)
  if (P != world)
    return fail(NBX_ERR_ARG, "nbx_group_create_rank: " + std::to_string(n) + " bodies give only " + std::to_string(P) +
                                 " non-empty blocks of 256-aligned size; start at most that many ranks");
  int ndev = 0;
  NBX_TRY(device_count(who, &ndev));
  const int dev = device >= 0 ? device : rank % ndev;
  if (dev >= ndev) return fail(NBX_ERR_ARG, "nbx_group_create_rank: device ordinal out of range");
  if (!g_rccl.load()) return fail(NBX_ERR_DEVICE, "nbx_group_create_rank: librccl could not be loaded");
  nbx_group* g = new (std::nothrow) nbx_group();
  if (!g) return fail(NBX_ERR_ALLOC, "nbx_group_create_rank: out of host memory");
  BatchOwner<nbx_group> owner{nbx_group_destroy, g};
  g->n = n; g->precision = precision; g->own = std::move(own); g->my_rank = rank; g->opts = o;
  g->dev.push_back(dev);
  NBX_TRY(make_context(g, who, rank, dev));
  HIP_TRY(hipSetDevice(dev));
  HIP_TRY(hipMalloc(&g->ke_all, sizeof(double) * (size_t)P));
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof id);
  g->comm.assign(1, nullptr);
  Watchdog::instance().set_identity(rank, P);
  ncclResult_t e;
  {
    // blocks until all P ranks have called it.  RCCL's own set-up -- loading its kernels, topology detection, channel set-up --
    // is legitimate work in front of the hand-shake: 4-5 s for a world of one on a cold process (measured), more on eight GPUs
    double init_allowance = kRcclInitAllowanceSeconds;  // NBX_RCCL_INIT_ALLOWANCE=<seconds> overrides (large nodes; tests)
    if (const char* txt = std::getenv("NBX_RCCL_INIT_ALLOWANCE")) {
      char* end = nullptr;
      const double v = std::strtod(txt, &end);
      if (end != txt && v >= 0.0) init_allowance = v;
    }
    Watchdog::Scope bounded("ncclCommInitRank (nbx_group_create_rank)", init_allowance);
    e = g_rccl.CommInitRank(&g->comm[0], P, id, rank);
  }
  if (e != ncclSuccess) { g->comm.clear(); return rccl_fail("ncclCommInitRank", e); }
  g->use_rccl = true;
  *out = owner.release();
  last_error().clear();
  return NBX_OK;
  });
}

void nbx_group_destroy(nbx_group* g) {
  if (!g) return;
  // draining the streams and tearing the communicators down waits for collectives in flight: bounded like the others
  Watchdog::Scope bounded("nbx_group_destroy (stream synchronisation + ncclCommDestroy)", queued_allowance(g));
  for (nbx_ctx* c : g->rank) if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
  for (auto cm : g->comm) if (cm) (void)g_rccl.CommDestroy(cm);
  for (size_t r = 0; r < g->done.size(); ++r) if (g->done[r]) { (void)hipSetDevice(g->dev[r]); (void)hipEventDestroy(g->done[r]); }
  if (!g->dev.empty()) (void)hipSetDevice(g->dev[0]);
  for (void* p : {(void*)g->ke_all, (void*)g->diag_all, g->vel_stage, g->vel_all})
    if (p) (void)hipFree(p);
  for (nbx_ctx* c : g->rank) nbx_destroy(c);
  delete g;
}

int nbx_group_upload(nbx_group* g, const void* px, const void* py, const void* pz, const void* vx, const void* vy, const void* vz, const void* m) {
  return guarded("nbx_group_upload", [&]() -> int {
  NBX_TRY(need(g, "nbx_group_upload", IS_THERE));
  for (nbx_ctx* c : g->rank) NBX_TRY(nbx_upload(c, px, py, pz, vx, vy, vz, m));
  if (g->weighted && m) {  // nbx_group_retune re-uploads the state to contexts with other slices: it needs the masses again
    const size_t bytes = (g->precision == 32 ? sizeof(float) : sizeof(double)) * (size_t)g->n;
    g->mass_host.assign((const char*)m, (const char*)m + bytes);
  }
  g->uploaded = true;
  return NBX_OK;
  });
}

int nbx_group_step(nbx_group* g, double dt, int32_t nsteps, double* kenergy_out) {
  return guarded("nbx_group_step", [&]() -> int {
  NBX_TRY(need(g, "nbx_group_step", IS_THERE));
  if (nsteps < 0) return fail(NBX_ERR_ARG, "nbx_group_step: nsteps < 0");
  if (!std::isfinite(dt)) return fail(NBX_ERR_ARG, "nbx_group_step: dt is not finite");
  NBX_TRY(need(g, "nbx_group_step", HAS_CONTEXTS));
  const auto t_enter = std::chrono::steady_clock::now();
  const bool window_from_sync = g->steps_unsynced == 0;  // everything this call waits for was enqueued by this call
  g->steps_unsynced += nsteps;
  // Groups that exchange over RCCL are bounded from the FIRST enqueue on, not only at the final synchronisation: the first
  // collective of a communicator sets its channels up on the host inside ncclGroupEnd / ncclAllGather, and a full launch queue
  // blocks the host in hipLaunchKernel -- a peer that died after ncclCommInitRank would otherwise leave this rank in the loop
  // below, which never reaches an armed region (and never at all when kenergy_out == NULL).  Scopes nest: the inner ones stay.
  Watchdog::Scope bounded_enqueue(g->use_rccl, "nbx_group_step (enqueue: local steps + position all-gathers)", queued_allowance(g));
  for (int s = 0; s < nsteps; ++s) {
    for (nbx_ctx* c : g->rank) NBX_TRY(nbx_step_local(c, dt));
    if (g->own.ranks > 1 || g->use_rccl) NBX_TRY(group_exchange(g));
    for (nbx_ctx* c : g->rank) NBX_TRY(nbx_commit(c));
  }
  if (kenergy_out) {
    double sum = 0.0;
    // the one place a stepping group blocks: every all-gather enqueued above completes only if every rank took part
    Watchdog::Scope bounded("nbx_group_step (position all-gathers + kinetic energy: stream synchronisation)", queued_allowance(g));
    NBX_TRY(group_sum_mv2(g, &sum));
    *kenergy_out = 0.5 * sum;
    if (window_from_sync && nsteps > 0)
      g->step_s_est = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_enter).count() / nsteps;
    g->steps_unsynced = 0;
  }
  return NBX_OK;
  });
}

int nbx_group_download(nbx_group* g, void* px, void* py, void* pz, void* vx, void* vy, void* vz) {
  return guarded("nbx_group_download", [&]() -> int {
  NBX_TRY(need(g, "nbx_group_download", IS_THERE | HAS_CONTEXTS));
  Watchdog::Scope bounded("nbx_group_download (stream synchronisation + all-gather of the velocities)", queued_allowance(g));
  Synced synced{g};
  for (nbx_ctx* c : g->rank) NBX_TRY(nbx_sync(c));
  if (g->my_rank >= 0) {
    // collective: every rank calls it.  Positions are complete on every rank; velocities live with their owners, so the
    // owned blocks are all-gathered (padded to `block` records) -- afterwards every caller holds the full final state,
    // as rank 0 of the reference does after mpi_gather (ver5_all/GSimulation.cpp:186-214).
    nbx_ctx* c = g->rank[0];
    NBX_TRY(nbx_download(c, px, py, pz, nullptr, nullptr, nullptr));
    if (!vx && !vy && !vz) return NBX_OK;
    NBX_TRY(use_device(c));
    const size_t rec = c->rec, blk = rec * (size_t)g->own.block;
    if (!g->vel_stage) HIP_TRY(hipMalloc(&g->vel_stage, blk));
    if (!g->vel_all) HIP_TRY(hipMalloc(&g->vel_all, blk * (size_t)g->own.ranks));
    HIP_TRY(hipMemsetAsync(g->vel_stage, 0, blk, c->stream));
    HIP_TRY(hipMemcpyAsync(g->vel_stage, c->velm, rec * (size_t)c->i_count, hipMemcpyDeviceToDevice, c->stream));
    std::vector<char> h(rec * (size_t)g->n);
    NBX_TRY(gather_rows(g, g->vel_stage, blk, g->vel_all, h.data(), h.size(), "ncclAllGather(velocities)"));
    if (c->precision == 32) unpack_xyz((const float4*)h.data(), g->n, (float*)vx, (float*)vy, (float*)vz);
    else unpack_xyz((const double4*)h.data(), g->n, (double*)vx, (double*)vy, (double*)vz);
    return NBX_OK;
  }
  for (size_t r = 0; r < g->rank.size(); ++r)  // positions once (rank 0 holds all), velocities per owner
    NBX_TRY(nbx_download(g->rank[r], r == 0 ? px : nullptr, r == 0 ? py : nullptr, r == 0 ? pz : nullptr, vx, vy, vz));
  return NBX_OK;
  });
}

int nbx_group_diagnostics(nbx_group* g, nbx_diag_t* out) {
  return guarded("nbx_group_diagnostics", [&]() -> int {
  if (!g || !out) return fail(NBX_ERR_ARG, "nbx_group_diagnostics: NULL argument");
  if (out->struct_size != 0 && out->struct_size != (int32_t)sizeof(nbx_diag_t))
    return fail(NBX_ERR_ARG, "nbx_group_diagnostics: nbx_diag_t.struct_size does not match this library");
  NBX_TRY(need(g, "nbx_group_diagnostics", HAS_CONTEXTS | HAS_STATE));
  constexpr int F = kDiagFieldCount;
  double sum[F] = {};
  int32_t bodies = 0;
  if (g->my_rank >= 0) {
    // one process per GPU: every rank reduces its partials on the device, one all-gather of the raw sums, and all ranks add
    // the rows (as the kinetic energy of nbx_group_step)
    Watchdog::Scope bounded("nbx_group_diagnostics (all-gather of the partials: stream synchronisation)", queued_allowance(g));
    Synced synced{g};
    nbx_ctx* c = g->rank[0];
    NBX_TRY(enqueue_diagnostics(c, "nbx_group_diagnostics"));
    std::vector<double> rows((size_t)F * g->own.ranks);
    if (!g->diag_all) HIP_TRY(hipMalloc(&g->diag_all, sizeof(double) * rows.size()));
    NBX_TRY(gather_rows(g, c->diag_dev, sizeof(double) * F, g->diag_all, rows.data(), sizeof(double) * rows.size(), "ncclAllGather(diagnostics)"));
    for (size_t k = 0; k < rows.size(); ++k) sum[k % F] += rows[k];
    bodies = g->n;
  } else {
    for (nbx_ctx* c : g->rank) {  // rank order: deterministic
      NBX_TRY(enqueue_diagnostics(c, "nbx_group_diagnostics"));
      double raw[F];
      HIP_TRY(hipMemcpyAsync(raw, c->diag_dev, sizeof(raw), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      for (int q = 0; q < F; ++q) sum[q] += raw[q];
      bodies += c->i_count;
    }
  }
  diag_fill(sum, bodies, g->rank[0]->steps_done, out);
  return NBX_OK;
  });
}

// include/nbx_kick.h: every rank kicks its owned slice (nbx_kick.hip); positions do not move, so there is nothing to exchange
int nbx_group_kick(nbx_group* g, double h, double* kenergy_out) {
  return guarded("nbx_group_kick", [&]() -> int {
  NBX_TRY(need(g, "nbx_group_kick", IS_THERE));
  if (!std::isfinite(h)) return fail(NBX_ERR_ARG, "nbx_group_kick: h is not finite");
  NBX_TRY(need(g, "nbx_group_kick", HAS_CONTEXTS | HAS_STATE));
  for (const nbx_ctx* c : g->rank)  // before any rank is kicked: no rank may be left half a kick ahead of the others
    if (c->pending_commit) return fail(NBX_ERR_STATE, "nbx_group_kick: a local step awaits nbx_commit");
  g->steps_unsynced += 1;  // a kick is a force launch: queued work that the watchdog's allowance counts as a step's
  for (nbx_ctx* c : g->rank) NBX_TRY(nbx_kick(c, h, nullptr));
  if (kenergy_out) {
    double sum = 0.0;
    // as nbx_group_step: the one place the call blocks, and for a rank group a collective
    Watchdog::Scope bounded("nbx_group_kick (kinetic energy: stream synchronisation)", queued_allowance(g));
    Synced synced{g};
    NBX_TRY(group_sum_mv2(g, &sum));
    *kenergy_out = 0.5 * sum;
  }
  return NBX_OK;
  });
}

int nbx_collective_timeout(double seconds) {
  return guarded("nbx_collective_timeout", [&]() -> int {
  if (std::isnan(seconds)) return fail(NBX_ERR_ARG, "nbx_collective_timeout: seconds is NaN");
  Watchdog::instance().set_timeout(seconds);
  return NBX_OK;
  });
}

int nbx_group_info(nbx_group* g, int32_t* n_ranks, int32_t* uses_rccl, int32_t rank, nbx_stats_t* rank_stats) {
  return guarded("nbx_group_info", [&]() -> int {
  NBX_TRY(need(g, "nbx_group_info", IS_THERE));
  if (n_ranks) *n_ranks = g->own.ranks;
  if (uses_rccl) *uses_rccl = g->use_rccl ? 1 : 0;
  if (rank_stats) {
    if (rank < 0 || rank >= g->own.ranks) return fail(NBX_ERR_ARG, "nbx_group_info: rank out of range");
    // a rank group holds this process's context only: its statistics are returned whatever rank is asked for
    return nbx_stats(g->rank[g->my_rank >= 0 ? 0 : rank], rank_stats);
  }
  return NBX_OK;
  });
}

}  // extern "C"
