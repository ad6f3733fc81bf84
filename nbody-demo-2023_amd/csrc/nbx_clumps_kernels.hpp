// nbx_clumps_kernels.hpp -- the kernels of nbx_clumps, nbx_ensemble_clumps and nbx_ragged_clumps (include/nbx_clumps.h): for
// every body i of a system of n bodies with a caller-supplied label, over c(i) = { j < n : label[j] == label[i] >= 0 }, the
// number of members, their G m, centre of mass and mean velocity, the potential of the OTHER members at i and i's specific energy
// in the clump's frame.  Instantiated by nbx_clumps.hip alone.
//
//   clump_kernel<T>            grid (columns, splits), block 256          a context that owns all n bodies
//   ensemble_clump_kernel<T>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_clump_kernel<T>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads its
//                              member's {pos_off, vel_off, out_off, n} from the table, evaluates field_shape(n, n) itself and
//                              returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three run clump_body: 256 threads, two bodies per lane, the j range of the workgroup's split in 256-record tiles staged
//     in LDS -- TWO arrays per tile, the position records and the velocity records of the same j, each read whole -- the next tile
//     prefetched into registers.  Columns, splits and tiles per split are field_shape(n, n) (nbx_field_shape.hpp).
//   clump_finish_kernel<T>     one thread per body of the call: adds the body's split records in fp64 in split order, forms the
//                              quotients and the energy in fp64, rounds each value once to T, applies the one-body, gm == 0 and
//                              negative-label cases
//
// The label travels as BITS in the staged velocity record's .w (the resident record keeps the mass there; the tile's copy does not
// need it): an int32 moved through registers and LDS, compared as an integer, never converted.  The sentinel rule: a staged
// record with j >= n or a negative label carries kClumpNoneJ, an i-side body with a negative label (or beyond n) carries
// kClumpNoneI.  Neither is a valid label and they differ, so padding, unlabelled bodies and negative labels among themselves match
// nothing and need no mask of their own.
//
// One pair, in T (the fp32 tile loop is the same operations on the lane's two bodies per packed instruction):
//   g = label_j == label_i ? gm_j : 0                       one integer compare, one select; the count adds the compare's bit
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))           the force kernels' r2
//   inv = rsq(r2)
//   S += g * inv (fma);  M += g;  P_a += g * v_ja (fma, 3);  X_a += g * x_ja (fma, 3)
// fp32 per j record and lane: 4 packed adds (three subtracts, M), 10 packed fma (3 r2, S, 3 P, 3 X), 2 v_rsq_f32, 2 compares and
// 2 selects.  gm_j is the record's .w as stored -- G m in fp32, G m / 8 in fp64, where rsq is 2 / sqrt: S carries 1 / 4 and M
// carries 1 / 8 in fp64, powers of two that the finish undoes once (clump_phi_scale, clump_gm_scale); P / M and X / M carry none.
//
// j == i is counted in M, P, X and the count and never in S: only the tiles that meet the workgroup's own bodies run the loop
// with the j != i compare (clump_tile<..., SELF>), which selects a second g for S; every other tile runs the loop without it.
//
// Every member of a clump recomputes the clump's M, P and X.  The sequence of g a body sees -- gm_j where the labels match, 0
// elsewhere, j ascending within a split, the splits of field_shape(n, n) -- is the same for every member, so every member gets the
// SAME BITS; no atomics, no sort, no second pass.
//
// Partials: two records of T per (split, body), {S, M, Px, Py} and {Pz, Xx, Xy, Xz}, at 2 * (split * n + body) of the member's
// rows, and one int32 count at split * n + body of the member's count rows.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kClumpBodies = 2;                         // bodies per lane (fp32: one packed pair)
constexpr long long kClumpMaxBodies = kFieldMaxPoints;  // per call (include/nbx_clumps.h)
constexpr int kClumpNoneJ = -1;                         // a staged record that is in no clump
constexpr int kClumpNoneI = -2;                         // an i-side body that is in no clump
constexpr int kClumpOutRecords = 3;                     // result records of T per body: {gm, cx, cy, cz} {vx, vy, vz, phi} {energy, 0, 0, 0}

// what S and M are multiplied by in the finish: 1 / (gm_prescale * the numerator of rsq) and 1 / gm_prescale -- powers of two
template <typename T> __host__ __device__ constexpr double clump_phi_scale() { return sizeof(T) == 8 ? 4.0 : 1.0; }
template <typename T> __host__ __device__ constexpr double clump_gm_scale() { return sizeof(T) == 8 ? 8.0 : 1.0; }

// the label bits of a staged velocity record
__device__ __forceinline__ float clump_bits(float, int l) { return __int_as_float(l); }
__device__ __forceinline__ double clump_bits(double, int l) { return __hiloint2double(0, l); }
__device__ __forceinline__ int clump_label(float w) { return __float_as_int(w); }
__device__ __forceinline__ int clump_label(double w) { return __double2loint(w); }

// the eight sums of one body (V: T, or two bodies packed)
template <typename V>
struct ClumpSums {
  V s, m, px, py, pz, xx, xy, xz;
};

// One pair of the scalar form.  g: the selected gm_j for M, P and X; gs: the one for S (0 where j == i).
template <typename T>
__device__ __forceinline__ void clump_pair(T xj, T yj, T zj, T uj, T vj, T wj, T g, T gs, T xi, T yi, T zi, ClumpSums<T>& a) {
  const T dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
  const T inv = rsq(r2);
  a.s = fmaT(gs, inv, a.s);
  a.m = add_rn(a.m, g);
  a.px = fmaT(g, uj, a.px);
  a.py = fmaT(g, vj, a.py);
  a.pz = fmaT(g, wj, a.pz);
  a.xx = fmaT(g, xj, a.xx);
  a.xy = fmaT(g, yj, a.xy);
  a.xz = fmaT(g, zj, a.xz);
}

// two bodies per call on the packed-fp32 pipe
__device__ __forceinline__ void clump_pair2(float4 r, float4 v, f32x2 g, f32x2 gs, f32x2 xi, f32x2 yi, f32x2 zi, ClumpSums<f32x2>& a) {
  const f32x2 dx = f32x2{r.x, r.x} - xi, dy = f32x2{r.y, r.y} - yi, dz = f32x2{r.z, r.z} - zi;
  const f32x2 e2 = {softening2<float>(), softening2<float>()};
  f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dx, dx, r2);
  f32x2 inv;
  inv.x = __builtin_amdgcn_rsqf(r2.x);
  inv.y = __builtin_amdgcn_rsqf(r2.y);
  a.s = __builtin_elementwise_fma(gs, inv, a.s);
  a.m = add_rn(a.m, g);
  a.px = __builtin_elementwise_fma(g, f32x2{v.x, v.x}, a.px);
  a.py = __builtin_elementwise_fma(g, f32x2{v.y, v.y}, a.py);
  a.pz = __builtin_elementwise_fma(g, f32x2{v.z, v.z}, a.pz);
  a.xx = __builtin_elementwise_fma(g, f32x2{r.x, r.x}, a.xx);
  a.xy = __builtin_elementwise_fma(g, f32x2{r.y, r.y}, a.xy);
  a.xz = __builtin_elementwise_fma(g, f32x2{r.z, r.z}, a.xz);
}

// What a lane keeps for its two bodies: fp32 packs them, body 0 in .x and body 1 in .y of every value; fp64 holds two scalars.
template <typename T> struct ClumpLane;
template <> struct ClumpLane<float> {
  f32x2 x, y, z;
  ClumpSums<f32x2> a;
  int l0, l1, i0, i1, c0, c1;  // labels (or kClumpNoneI), own indices, counts
  __device__ __forceinline__ void load(int b, float4 p, int label, int index) {
    if (b == 0) { x.x = p.x; y.x = p.y; z.x = p.z; l0 = label; i0 = index; }
    else { x.y = p.x; y.y = p.y; z.y = p.z; l1 = label; i1 = index; }
  }
  __device__ __forceinline__ void clear() {
    const f32x2 o = {0.0f, 0.0f};
    a.s = a.m = a.px = a.py = a.pz = a.xx = a.xy = a.xz = o;
    c0 = c1 = 0;
  }
  __device__ __forceinline__ ClumpSums<float> sums(int b) const {
    if (b == 0) return ClumpSums<float>{a.s.x, a.m.x, a.px.x, a.py.x, a.pz.x, a.xx.x, a.xy.x, a.xz.x};
    return ClumpSums<float>{a.s.y, a.m.y, a.px.y, a.py.y, a.pz.y, a.xx.y, a.xy.y, a.xz.y};
  }
  __device__ __forceinline__ int count(int b) const { return b == 0 ? c0 : c1; }
  // SELF: the tile may hold the lane's own bodies (j_glob: global index of tile record 0)
  template <bool SELF>
  __device__ __forceinline__ void tile(const float4* ptile, const float4* vtile, const int j_glob) {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = ptile[j];
      const float4 v = vtile[j];
      const int lj = clump_label(v.w);
      const bool m0 = lj == l0, m1 = lj == l1;
      const f32x2 g = {m0 ? r.w : 0.0f, m1 ? r.w : 0.0f};
      f32x2 gs = g;
      if constexpr (SELF) {
        const int jg = j_glob + j;
        gs.x = jg != i0 ? g.x : 0.0f;
        gs.y = jg != i1 ? g.y : 0.0f;
      }
      c0 += m0 ? 1 : 0;
      c1 += m1 ? 1 : 0;
      clump_pair2(r, v, g, gs, x, y, z, a);
    }
  }
};
template <> struct ClumpLane<double> {
  double x0, y0, z0, x1, y1, z1;
  ClumpSums<double> a0, a1;
  int l0, l1, i0, i1, c0, c1;
  __device__ __forceinline__ void load(int b, double4 p, int label, int index) {
    if (b == 0) { x0 = p.x; y0 = p.y; z0 = p.z; l0 = label; i0 = index; }
    else { x1 = p.x; y1 = p.y; z1 = p.z; l1 = label; i1 = index; }
  }
  __device__ __forceinline__ void clear() {
    a0.s = a0.m = a0.px = a0.py = a0.pz = a0.xx = a0.xy = a0.xz = 0.0;
    a1 = a0;
    c0 = c1 = 0;
  }
  __device__ __forceinline__ ClumpSums<double> sums(int b) const { return b == 0 ? a0 : a1; }
  __device__ __forceinline__ int count(int b) const { return b == 0 ? c0 : c1; }
  template <bool SELF>
  __device__ __forceinline__ void tile(const double4* ptile, const double4* vtile, const int j_glob) {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const double4 r = ptile[j];
      const double4 v = vtile[j];
      const int lj = clump_label(v.w);
      const bool m0 = lj == l0, m1 = lj == l1;
      const double g0 = m0 ? r.w : 0.0, g1 = m1 ? r.w : 0.0;
      double gs0 = g0, gs1 = g1;
      if constexpr (SELF) {
        const int jg = j_glob + j;
        gs0 = jg != i0 ? g0 : 0.0;
        gs1 = jg != i1 ? g1 : 0.0;
      }
      c0 += m0 ? 1 : 0;
      c1 += m1 ? 1 : 0;
      clump_pair<double>(r.x, r.y, r.z, v.x, v.y, v.z, g0, gs0, x0, y0, z0, a0);
      clump_pair<double>(r.x, r.y, r.z, v.x, v.y, v.z, g1, gs1, x1, y1, z1, a1);
    }
  }
};

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), whose velocity records velm[0 .. n) and labels lab[0 .. n) are
// read.  Writes, for every body below n of the column, records 2 * (split * n + body) and the next of parts and element
// split * n + body of counts.
template <typename T>
__device__ __forceinline__ void clump_body(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                           const int* __restrict__ lab, const int n, const int tiles_per_split,
                                           typename V4<T>::type* __restrict__ parts, int* __restrict__ counts, const int col,
                                           const int split) {
  using T4 = typename V4<T>::type;
  constexpr int B = kClumpBodies;
  __shared__ T4 ptile[kTile];
  __shared__ T4 vtile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  ClumpLane<T> lane;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    int label = kClumpNoneI;
    if (li < n) {
      p = posm[li];
      const int l = lab[li];
      label = l < 0 ? kClumpNoneI : l;
    }
    lane.load(b, p, label, li);
  }
  lane.clear();
  const int g_lo = l0, g_hi = min(l0 + kBlock * B, n);  // the workgroup's bodies: a tile that meets them runs the loop with j != i
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  T4 next_p = zero, next_v = zero;
  int next_l = kClumpNoneJ;
  if (k0 < k1) {
    const int j = k0 * kTile + t;
    next_p = posm[j];
    if (j < n) {
      next_v = velm[j];
      const int l = lab[j];
      next_l = l < 0 ? kClumpNoneJ : l;
    }
  }
  for (int k = k0; k < k1; ++k) {
    __syncthreads();  // every lane is done with the previous tile
    next_v.w = clump_bits((T)0, next_l);
    ptile[t] = next_p;
    vtile[t] = next_v;
    __syncthreads();
    if (k + 1 < k1) {
      const int j = (k + 1) * kTile + t;
      next_p = posm[j];
      next_v = zero;
      next_l = kClumpNoneJ;
      if (j < n) {
        next_v = velm[j];
        const int l = lab[j];
        next_l = l < 0 ? kClumpNoneJ : l;
      }
    }
    const int j0 = k * kTile;
    if (j0 < g_hi && j0 + kTile > g_lo) lane.template tile<true>(ptile, vtile, j0);
    else lane.template tile<false>(ptile, vtile, j0);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) {
      const ClumpSums<T> s = lane.sums(b);
      T4 o0, o1;
      o0.x = s.s; o0.y = s.m; o0.z = s.px; o0.w = s.py;
      o1.x = s.pz; o1.y = s.xx; o1.z = s.xy; o1.w = s.xz;
      const size_t at = (size_t)split * (size_t)n + (size_t)li;
      parts[2 * at] = o0;
      parts[2 * at + 1] = o1;
      counts[at] = lane.count(b);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void clump_kernel(const typename V4<T>::type* __restrict__ posm,
                                                       const typename V4<T>::type* __restrict__ velm, const int* __restrict__ lab, int n,
                                                       int tiles_per_split, typename V4<T>::type* __restrict__ parts,
                                                       int* __restrict__ counts) {
  clump_body<T>(posm, velm, lab, n, tiles_per_split, parts, counts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as the ensemble's step kernels have it: posm[S][n_alloc + kSgprOverread], velm[S][own_pad]; lab[count][n];
// parts[count][gridDim.y][n][2], counts[count][gridDim.y][n].
template <typename T>
struct EnsembleClumpArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* velm;  // member 0's velocities
  const int* lab;                    // the labels of member `first`
  typename V4<T>::type* parts;       // the partial rows of member `first`
  int* counts;                       // the count rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  unsigned vel_stride;               // records between members in velm
  int n, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_clump_kernel(const EnsembleClumpArgs<T> e) {
  const size_t k = blockIdx.z;
  const size_t rows = k * gridDim.y * (size_t)e.n;
  clump_body<T>(e.posm + (e.first + k) * e.pos_stride, e.velm + (e.first + k) * e.vel_stride, e.lab + k * (size_t)e.n, e.n,
                e.tiles_per_split, e.parts + 2 * rows, e.counts + rows, blockIdx.x, blockIdx.y);
}

struct ClumpMember : VelMember {};

template <typename T>
struct RaggedClumpArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  const ClumpMember* table;          // [members]
  const int* lab;                    // the labels of member `first`
  typename V4<T>::type* parts;       // the partial rows of member `first`
  int* counts;                       // the count rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_clump_kernel(const RaggedClumpArgs<T> r) {
  const MemberGroup<ClumpMember> g = member_group(r.table, r.first);
  if (g.elsewhere()) return;
  const size_t rel = g.rel(), rows = rel * gridDim.y;
  clump_body<T>(r.posm + g.mem.pos_off, r.velm + g.mem.vel_off, r.lab + rel, g.mem.n, g.shape.tiles_per_split, r.parts + 2 * rows,
                r.counts + rows, blockIdx.x, blockIdx.y);
}

// what the finish kernel reads besides the partials: where a body's own records are
template <typename T>
struct ClumpFinishArgs {
  const typename V4<T>::type* posm;  // member 0's current records (a context: its own)
  const typename V4<T>::type* velm;
  const int* lab;                    // the labels of the call
  const typename V4<T>::type* parts;
  const int* counts;
  const ClumpMember* table;          // a ragged ensemble's, else nullptr
  unsigned first;
  int count;
  int n_all;                         // table == nullptr: the bodies of every system
  unsigned pos_stride, vel_stride;   // table == nullptr: records between members
  int row_splits;                    // the gridDim.y of the pair-work launch
  unsigned total;
  typename V4<T>::type* out;         // [total][kClumpOutRecords]
  int* members;                      // [total]
};

// Body idx of the call's `total` bodies.  table == nullptr: member idx / n_all of the range.  Otherwise the member is the last
// of table[first .. first + count) whose out_off, taken from member first, is not above idx.  The member has
// field_shape(n, n).splits rows; its rows begin at (the bodies of the range before it) * row_splits.
template <typename T>
__global__ __launch_bounds__(kBlock) void clump_finish_kernel(const ClumpFinishArgs<T> f) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= f.total) return;
  int n = f.n_all;
  size_t rel = 0;  // the bodies of the range before the body's member
  size_t pos_off = 0, vel_off = 0;
  if (f.table) {
    const unsigned long long base = f.table[f.first].out_off;
    int lo = 0, hi = f.count - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (f.table[f.first + mid].out_off - base <= idx) lo = mid;
      else hi = mid - 1;
    }
    const ClumpMember mem = f.table[f.first + lo];
    n = mem.n;
    rel = (size_t)(mem.out_off - base);
    pos_off = (size_t)mem.pos_off;
    vel_off = (size_t)mem.vel_off;
  } else {
    const unsigned k = idx / (unsigned)f.n_all;
    rel = (size_t)k * (size_t)f.n_all;
    pos_off = (size_t)(f.first + k) * f.pos_stride;
    vel_off = (size_t)(f.first + k) * f.vel_stride;
  }
  const size_t body = (size_t)idx - rel;
  T4 o0, o1, o2;
  o0.x = o0.y = o0.z = o0.w = (T)0;
  o1 = o2 = o0;
  int members = 0;
  if (f.lab[idx] >= 0) {
    const int splits = field_shape(n, n).splits;
    const size_t row = rel * (size_t)f.row_splits + body;
    double s = 0.0, m = 0.0, px = 0.0, py = 0.0, pz = 0.0, xx = 0.0, xy = 0.0, xz = 0.0;
    for (int k = 0; k < splits; ++k) {
      const size_t at = row + (size_t)k * (size_t)n;
      const T4 a = f.parts[2 * at], b = f.parts[2 * at + 1];
      s += (double)a.x; m += (double)a.y; px += (double)a.z; py += (double)a.w;
      pz += (double)b.x; xx += (double)b.y; xy += (double)b.z; xz += (double)b.w;
      members += f.counts[at];
    }
    const T4 p = f.posm[pos_off + body];
    const T4 v = f.velm[vel_off + body];
    o0.x = (T)(m * clump_gm_scale<T>());
    if (members == 1) {  // the body alone: its own position and velocity, exactly
      o0.y = p.x; o0.z = p.y; o0.w = p.z;
      o1.x = v.x; o1.y = v.y; o1.z = v.z;
    } else {
      double cx = 0.0, cy = 0.0, cz = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
      if (m != 0.0) {
        cx = xx / m; cy = xy / m; cz = xz / m;
        ux = px / m; uy = py / m; uz = pz / m;
      }
      const double phi = 0.0 - s * clump_phi_scale<T>();  // +0 where nothing was summed
      const double wx = (double)v.x - ux, wy = (double)v.y - uy, wz = (double)v.z - uz;
      const double e = __builtin_fma(0.5, __builtin_fma(wx, wx, __builtin_fma(wy, wy, wz * wz)), phi);
      o0.y = (T)cx; o0.z = (T)cy; o0.w = (T)cz;
      o1.x = (T)ux; o1.y = (T)uy; o1.z = (T)uz;
      o1.w = (T)phi;
      o2.x = (T)e;
    }
  }
  T4* out = f.out + (size_t)kClumpOutRecords * idx;
  out[0] = o0;
  out[1] = o1;
  out[2] = o2;
  f.members[idx] = members;
}

}  // namespace nbx
