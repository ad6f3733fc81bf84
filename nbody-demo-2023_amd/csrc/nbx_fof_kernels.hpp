// nbx_fof_kernels.hpp -- the kernels of nbx_fof, nbx_ensemble_fof and nbx_ragged_fof (include/nbx_fof.h): friends-of-friends
// groups.  Bodies i != j of a system of n bodies are friends where
//     r2(i, j) = |x_j - x_i|^2 + eps^2 <= h2
// and a group is a connected component of that graph; label[i] is the lowest index in i's component.  Instantiated by
// nbx_fof.hip alone.
//
// Labels are int32 and, on the device, indices into the call's bodies (the bodies of the range before the member + the body's
// own index): within a member that is the member-local order shifted, so every minimum is the member-local minimum, and the
// O(n) kernels need no member table.  fof_gather_kernel takes the shift off again.  One PASS over labels L (L[i] = i at first):
//
//   fof_pass_kernel<T>            grid (columns, splits), block 256                     a context
//   ensemble_fof_pass_kernel<T>   grid (columns, splits, count), block 256              member first + blockIdx.z
//   ragged_fof_pass_kernel<T>     grid (largest columns, largest splits, count): the workgroup reads its member's entry, evaluates
//                                 field_shape(n, n) itself; where blockIdx.x is not one of its member's columns it returns at once,
//                                 where blockIdx.y is not one of its splits it writes the neutral row
//     All three run fof_body: 256 threads, two bodies per lane, the j range of the workgroup's split in 256-record tiles staged in
//     LDS (ONE array, read whole), the next tile prefetched into registers.  They read the STAGED records rec[] = {x, y, z,
//     bits(L[j])} -- never posm -- and write parts[split][body] = min over the split's j with r2(i, j) <= h2 of L[j].  No mask: the
//     self pair has r2 = eps2 <= h2 and the body's own label; a record at or beyond n carries kFofNone, the largest int32, and
//     never lowers a minimum.  No atomics.  Columns, splits and tiles per split are field_shape(n, n): nothing depends on it.
//   fof_hook_kernel               one thread per body: m = the minimum over the split rows; atomicMin(&N[i], m) and
//                                 atomicMin(&N[L[i]], m) -- the old root is hooked.  N equals L when the kernel starts, every read
//                                 is from L and every write to N: N afterwards is min(L[k], m[k], m[i] for every i with L[i] == k),
//                                 whatever the order.  The only atomics of a pass, on integers.
//   fof_shortcut_kernel<FINAL>    one thread per body: N[i] = the ancestor up to kFofHops steps up the pointers N (N[k] <= k: a
//                                 forest; values only move towards the root while the kernel runs, so a racing read still sees an
//                                 ancestor).  fof_rounds(n) launches reach the root from any depth below n.  FINAL, the last of
//                                 them: also restages rec[].w, sets *changed where N[i] != L[i] and stores L[i] = N[i].
// A pair, in T (fp32: the lane's two bodies per packed instruction, 3 packed subtracts and 3 packed fma per two pairs):
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)));  in = r2 <= h2;  best = in ? min(best, L[j]) : best
// The label never meets floating-point arithmetic: it is moved as bits and compared as an integer.
//
//   fof_init_kernel<T>            one thread per staged record of the call: position from posm, label = own index (kFofNone and
//                                 the origin at or beyond n); L = N = index; slot[body] = where its record is
//   fof_count_kernel              hist[label] += 1 (atomicAdd on integers)
//   fof_gather_kernel             label - shift and hist[label] per body; per member the number of roots and the largest hist
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kFofBodies = 2;                         // bodies per lane (fp32: one packed pair)
constexpr long long kFofMaxBodies = kFieldMaxPoints;  // per call (include/nbx_fof.h, status 4)
constexpr int kFofNone = 0x7fffffff;                  // the label of a padding record and of an empty row
constexpr int kFofHops = 16;                          // pointer steps of one shortcut launch

// the launches of fof_shortcut_kernel that take every body of a forest of n nodes to its root: a launch divides the depth
// (< n) by kFofHops, rounded up
constexpr int fof_rounds(int n) {
  int r = 1;
  for (long long reach = kFofHops; reach < (long long)n - 1; reach *= kFofHops) ++r;
  return r;
}

template <typename T> struct FofBits;
template <> struct FofBits<float> {
  static __device__ __forceinline__ int get(float w) { return __float_as_int(w); }
  static __device__ __forceinline__ float put(int l) { return __int_as_float(l); }
};
template <> struct FofBits<double> {
  static __device__ __forceinline__ int get(double w) { return __double2loint(w); }
  static __device__ __forceinline__ double put(int l) { return __hiloint2double(0, l); }
};

// one pair against the running minimum: a compare (the caller's), an integer min and a select
__device__ __forceinline__ void fof_take(const bool in, const int lab, int& best) {
  const int low = min(best, lab);
  best = in ? low : best;
}

// One LDS tile against the lane's B bodies.
template <typename T, int B>
__device__ __forceinline__ void fof_tile(const typename V4<T>::type* tile, const T (&xi)[B], const T (&yi)[B], const T (&zi)[B], const T h2,
                                         int (&best)[B]) {
  if constexpr (sizeof(T) == 4 && B % 2 == 0) {
    f32x2 px[B / 2], py[B / 2], pz[B / 2];
#pragma unroll
    for (int h = 0; h < B / 2; ++h) {
      px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
      py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
      pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
    }
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = tile[j];  // the whole record: .w is the label
      const int lab = FofBits<float>::get(r.w);
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        const f32x2 dx = f32x2{r.x, r.x} - px[h], dy = f32x2{r.y, r.y} - py[h], dz = f32x2{r.z, r.z} - pz[h];
        f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        r2 = __builtin_elementwise_fma(dx, dx, r2);
        fof_take(r2.x <= h2, lab, best[2 * h]);
        fof_take(r2.y <= h2, lab, best[2 * h + 1]);
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = tile[j];
      const int lab = FofBits<T>::get(r.w);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const T dx = r.x - xi[b], dy = r.y - yi[b], dz = r.z - zi[b];
        const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
        fof_take(r2 <= h2, lab, best[b]);
      }
    }
  }
}

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose staged records
// rec[0 .. ceil(n / 256) * 256) exist.  Writes, for every body below n of the column, parts[split * total + body]; `parts` points
// at the member's first body of row 0, `total` is the bodies of the call.
template <typename T, int B>
__device__ __forceinline__ void fof_body(const typename V4<T>::type* __restrict__ rec, const int n, const int tiles_per_split, const T h2,
                                         int* __restrict__ parts, const size_t total, const int col, const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  T xi[B], yi[B], zi[B];
  int best[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p;
    p.x = p.y = p.z = p.w = (T)0;
    if (li < n) p = rec[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    best[b] = kFofNone;
  }
  TileWalk<T4> walk(rec, n, split, tiles_per_split);
  for (int k = walk.k0; k < walk.k1; ++k) {
    walk.stage(tile, k);
    fof_tile<T, B>(tile, xi, yi, zi, h2, best);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) parts[(size_t)split * total + (size_t)li] = best[b];
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void fof_pass_kernel(const typename V4<T>::type* __restrict__ rec, int n, int tiles_per_split, T h2,
                                                          int* __restrict__ parts) {
  fof_body<T, kFofBodies>(rec, n, tiles_per_split, h2, parts, (size_t)n, blockIdx.x, blockIdx.y);
}

// rec[count][rec_stride], rec_stride = ceil(n / 256) * 256; parts[gridDim.y][count * n]
template <typename T>
struct EnsembleFofArgs {
  const typename V4<T>::type* rec;
  int* parts;
  T h2;
  unsigned rec_stride;
  int n, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_fof_pass_kernel(const EnsembleFofArgs<T> e) {
  const size_t k = blockIdx.z;
  fof_body<T, kFofBodies>(e.rec + k * e.rec_stride, e.n, e.tiles_per_split, e.h2, e.parts + k * (size_t)e.n, (size_t)gridDim.z * (size_t)e.n,
                          blockIdx.x, blockIdx.y);
}

// one entry per member of a ragged ensemble, built on first use and fixed for the object's life
struct FofMember {
  unsigned long long pos_off;  // the member's first record in posm
  unsigned long long out_off;  // the bodies of the members before it
  unsigned long long rec_off;  // the staged records (each member's n rounded up to the tile) of the members before it
  int n;
  int reserved;
};

template <typename T>
struct RaggedFofArgs {
  const typename V4<T>::type* rec;  // the staged records of member `first`
  const FofMember* table;           // [members]
  int* parts;
  T h2;
  unsigned first;  // member of blockIdx.z == 0
  unsigned total;  // the bodies of the range
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_fof_pass_kernel(const RaggedFofArgs<T> r) {
  const FofMember mem = r.table[r.first + blockIdx.z];
  const FofMember base = r.table[r.first];
  const FieldShape s = field_shape(mem.n, mem.n);
  if ((int)blockIdx.x >= s.columns) return;  // the whole workgroup: another, larger member's column
  int* parts = r.parts + (size_t)(mem.out_off - base.out_off);
  if ((int)blockIdx.y >= s.splits) {  // a row the member has no split for: neutral
#pragma unroll
    for (int b = 0; b < kFofBodies; ++b) {
      const int li = (int)blockIdx.x * (kBlock * kFofBodies) + b * kBlock + (int)threadIdx.x;
      if (li < mem.n) parts[(size_t)blockIdx.y * (size_t)r.total + (size_t)li] = kFofNone;
    }
    return;
  }
  fof_body<T, kFofBodies>(r.rec + (size_t)(mem.rec_off - base.rec_off), mem.n, s.tiles_per_split, r.h2, parts, (size_t)r.total, blockIdx.x,
                          blockIdx.y);
}

// What the O(n) kernels need to place a body or a staged record.  table == nullptr: every system has n_all bodies and
// rec_stride staged records, member k of the range at k * pos_stride records behind posm's member `first`.
struct FofRange {
  const FofMember* table;
  unsigned first;
  int count;
  int n_all;
  unsigned rec_stride;
  unsigned pos_stride;
};

// the member of the range -- counted from `first` -- that holds element `idx` of the range's bodies (REC: staged records)
template <bool REC>
__device__ __forceinline__ int fof_member_of(const FofRange& g, const unsigned idx) {
  if (!g.table) return (int)(idx / (REC ? g.rec_stride : (unsigned)g.n_all));
  const FofMember base = g.table[g.first];
  int lo = 0, hi = g.count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const FofMember m = g.table[g.first + mid];
    if ((REC ? m.rec_off - base.rec_off : m.out_off - base.out_off) <= idx) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Staged record `idx` of the call's rec_total.  changed[0 .. 2) is cleared for the first pass.
template <typename T>
__global__ __launch_bounds__(kBlock) void fof_init_kernel(const typename V4<T>::type* __restrict__ posm, const FofRange g, unsigned rec_total,
                                                          typename V4<T>::type* __restrict__ rec, int* __restrict__ lab, int* __restrict__ nxt,
                                                          unsigned* __restrict__ slot, int* __restrict__ changed) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx == 0) changed[0] = changed[1] = 0;
  if (idx >= rec_total) return;
  const int k = fof_member_of<true>(g, idx);
  size_t pos, rel;  // the member's first position record; the bodies of the range before it
  unsigned j;       // the record within the member
  int n;
  if (g.table) {
    const FofMember m = g.table[g.first + k], base = g.table[g.first];
    pos = (size_t)m.pos_off;
    rel = (size_t)(m.out_off - base.out_off);
    j = idx - (unsigned)(m.rec_off - base.rec_off);
    n = m.n;
  } else {
    pos = (size_t)(g.first + (unsigned)k) * g.pos_stride;
    rel = (size_t)k * (size_t)g.n_all;
    j = idx - (unsigned)k * g.rec_stride;
    n = g.n_all;
  }
  T4 r;
  r.x = r.y = r.z = (T)0;
  int l = kFofNone;
  if ((int)j < n) {
    const T4 p = posm[pos + j];
    r.x = p.x; r.y = p.y; r.z = p.z;
    l = (int)(rel + j);
    lab[l] = l;
    nxt[l] = l;
    slot[l] = idx;
  }
  r.w = FofBits<T>::put(l);
  rec[idx] = r;
}

// Body idx of the call's `total`.  Pass p reports in changed[p & 1]; this kernel clears the word of pass p + 1.
__global__ __launch_bounds__(kBlock) void fof_hook_kernel(const int* __restrict__ parts, int row_splits, unsigned total, const int* __restrict__ lab,
                                                          int* __restrict__ nxt, int* __restrict__ clear) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx == 0) *clear = 0;
  if (idx >= total) return;
  int m = kFofNone;
  for (int s = 0; s < row_splits; ++s) m = min(m, parts[(size_t)s * (size_t)total + idx]);
  atomicMin(&nxt[idx], m);
  atomicMin(&nxt[lab[idx]], m);
}

template <typename T, bool FINAL>
__global__ __launch_bounds__(kBlock) void fof_shortcut_kernel(unsigned total, int* __restrict__ lab, int* nxt, const unsigned* __restrict__ slot,
                                                              typename V4<T>::type* __restrict__ rec, int* __restrict__ changed) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  volatile int* up = nxt;  // other lanes move their pointers while this one walks: every value read is an ancestor
  const int own = up[idx];
  int r = own;
  for (int hop = 0; hop < kFofHops; ++hop) {
    const int above = up[r];
    if (above == r) break;
    r = above;
  }
  if (r != own) up[idx] = r;
  if constexpr (FINAL) {
    if (r != lab[idx]) {
      lab[idx] = r;
      rec[slot[idx]].w = FofBits<T>::put(r);
      *changed = 1;
    }
  }
}

__global__ __launch_bounds__(kBlock) void fof_count_kernel(unsigned total, const int* __restrict__ lab, int* __restrict__ hist) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx < total) atomicAdd(&hist[lab[idx]], 1);
}

// out: label[total], size[total], then {groups, largest} per member of the range, cleared beforehand
__global__ __launch_bounds__(kBlock) void fof_gather_kernel(const FofRange g, unsigned total, const int* __restrict__ lab,
                                                            const int* __restrict__ hist, int* __restrict__ out) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const int k = fof_member_of<false>(g, idx);
  const unsigned rel = g.table ? (unsigned)(g.table[g.first + k].out_off - g.table[g.first].out_off) : (unsigned)k * (unsigned)g.n_all;
  const int l = lab[idx];
  const int members = hist[l];
  out[idx] = l - (int)rel;
  out[(size_t)total + idx] = members;
  if (l == (int)idx) {  // a root: one group
    int* info = out + 2 * (size_t)total + 2 * (size_t)k;
    atomicAdd(&info[0], 1);
    atomicMax(&info[1], members);
  }
}

}  // namespace nbx
