// nbx_jerk_kernels.hpp -- the kernels of nbx_jerk, nbx_ensemble_jerk and nbx_ragged_jerk (include/nbx_jerk.h): for every body i
// of a system of n bodies the acceleration and its time derivative,
//     a_i    = sum over j < n of gm_j d / r2^(3/2)
//     adot_i = sum over j < n of gm_j [ u / r2^(3/2) - 3 (d.u) d / r2^(5/2) ],   d = x_j - x_i,  u = v_j - v_i,  r2 = |d|^2 + eps^2
// Instantiated by nbx_jerk.hip alone.
//
//   jerk_kernel<T>            grid (columns, splits), block 256          a context that owns all n bodies
//   ensemble_jerk_kernel<T>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_jerk_kernel<T>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads its
//                             member's {pos_off, vel_off, out_off, n} from the table, evaluates field_shape(n, n) itself and
//                             returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three run jerk_body: 256 threads, two bodies per lane (the i side: the column's own position and velocity records), the
//     j range of the workgroup's split in 256-record tiles staged in LDS -- TWO arrays per tile, the position records and the
//     velocity records of the same j, both read whole (a velocity is loaded only where j < n, zero is staged otherwise: what lies
//     behind a system's last velocity is never read) -- the next tile prefetched into registers.  Columns, splits and tiles per
//     split are field_shape(n, n) (nbx_field_shape.hpp): the rule of the field at caller-supplied points, no new one.
//   jerk_finish_kernel<T>     one thread per body of the call: adds the body's partial records in fp64 in split order, rounds
//                             once to T and writes {ax, ay, az, 0} and {jx, jy, jz, 0}
//
// One pair, in T.  A body keeps six sums over one split, j ascending.
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))          the force kernels' r2
//   ux,uy,uz = v_j - v_i;  rv = fma(dx,ux, fma(dy,uy, dz*uz))
//   fp32:  inv = rsq(r2);  inv2 = inv*inv;  s = (gm*inv)*inv2;  a += d*s (fma)      the operations of the field's acceleration
//          c = (rv*inv2)*(-3)   two separately rounded multiplies;  t_a = fma(c, d_a, u_a);  adot_a += t_a*s (fma)
//          on the lane's two bodies per packed instruction: 3 subtracts (d), 3 fma (r2), 3 multiplies (inv2, the two of s),
//          3 fma (a), 3 subtracts (u), 1 multiply and 2 fma (rv), 2 multiplies (c), 3 fma (t), 3 fma (adot)
//          = 26 packed VALU and 2 v_rsq_f32 per j record (two pairs)
//   fp64:  y = v_rsq_f64(r2);  y2 = y*y;  h = fma(-r2, y2, 1)       the seed and its residual, shared by the cube and 1/r2
//          s    = ((gm*y)*y2) * fma(h, fma(h, 15, 12), 8)           8 gm r2^(-3/2) (1 + O(h^3)), the field's
//          inv2 = fma(y2, fma(h, h, h), y2)                         y2 (1 + h + h^2) = (1/r2) (1 - h^3): second order
//          c, t and the sums as in fp32
// gm is the record's .w = G*m * gm_prescale<T>().  The fp64 prescale, 1/8, meets the 8 folded into the cube's polynomial -- powers
// of two, so every rounding is the one the unscaled operation would make: what leaves jerk_body carries no scale.  Every multiply
// or add that is not part of a written fma goes through mul_rn / add_rn, so no build contracts one.
//
// Nothing is masked.  j == i has d = u = 0: rv = 0, c = 0, t = 0 and both terms are exact zeros.  A position record at or beyond
// n -- the zero padding -- has gm = 0 and a finite r2 >= eps2, hence s = 0: with the zero staged for its velocity t is finite and
// both terms are exact zeros.
//
// Partials: two records of T per (split, body): {ax, ay, az, 0} and {jx, jy, jz, 0}, at 2 * (split * n + body) and the record
// after it of the system's rows.  Written by plain stores, each by one thread.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kJerkBodies = 2;                         // bodies per lane (fp32: one packed pair)
constexpr long long kJerkMaxBodies = kFieldMaxPoints;  // per call (include/nbx_jerk.h, status 4)

// the six sums of one body
template <typename V>
struct JerkSums {
  V ax, ay, az, jx, jy, jz;
};

// one pair of the scalar form (fp64)
__device__ __forceinline__ void jerk_pair(double xj, double yj, double zj, double gmj, double uj, double vj, double wj, double xi,
                                          double yi, double zi, double ui, double vi, double wi, JerkSums<double>& q) {
  const double dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const double r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<double>())));
  const double ux = uj - ui, uy = vj - vi, uz = wj - wi;
  const double rv = fmaT(dx, ux, fmaT(dy, uy, mul_rn(dz, uz)));
  const double y = __builtin_amdgcn_rsq(r2);
  const double y2 = mul_rn(y, y);
  const double h = __builtin_fma(-r2, y2, 1.0);
  const double p = __builtin_fma(h, __builtin_fma(h, 15.0, 12.0), 8.0);  // 8 (1 + 3/2 h + 15/8 h^2): the cube's
  const double s = mul_rn(mul_rn(mul_rn(gmj, y), y2), p);
  const double inv2 = __builtin_fma(y2, __builtin_fma(h, h, h), y2);     // y2 (1 + h + h^2)
  const double c = mul_rn(mul_rn(rv, inv2), -3.0);
  const double tx = fmaT(c, dx, ux), ty = fmaT(c, dy, uy), tz = fmaT(c, dz, uz);
  q.ax = fmaT(dx, s, q.ax);
  q.ay = fmaT(dy, s, q.ay);
  q.az = fmaT(dz, s, q.az);
  q.jx = fmaT(tx, s, q.jx);
  q.jy = fmaT(ty, s, q.jy);
  q.jz = fmaT(tz, s, q.jz);
}

// two bodies per call on the packed-fp32 pipe: r the position record, w the velocity record of one j
__device__ __forceinline__ void jerk_pair2(const float4 r, const float4 w, f32x2 xi, f32x2 yi, f32x2 zi, f32x2 ui, f32x2 vi, f32x2 wi,
                                           JerkSums<f32x2>& q) {
  const f32x2 dx = f32x2{r.x, r.x} - xi, dy = f32x2{r.y, r.y} - yi, dz = f32x2{r.z, r.z} - zi;
  const f32x2 e2 = {softening2<float>(), softening2<float>()};
  f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dx, dx, r2);
  const f32x2 ux = f32x2{w.x, w.x} - ui, uy = f32x2{w.y, w.y} - vi, uz = f32x2{w.z, w.z} - wi;
  f32x2 rv = mul_rn(dz, uz);
  rv = __builtin_elementwise_fma(dy, uy, rv);
  rv = __builtin_elementwise_fma(dx, ux, rv);
  f32x2 inv;
  inv.x = __builtin_amdgcn_rsqf(r2.x);
  inv.y = __builtin_amdgcn_rsqf(r2.y);
  const f32x2 inv2 = mul_rn(inv, inv);
  const f32x2 s = mul_rn(mul_rn(f32x2{r.w, r.w}, inv), inv2);
  const f32x2 c = mul_rn(mul_rn(rv, inv2), f32x2{-3.0f, -3.0f});
  const f32x2 tx = __builtin_elementwise_fma(c, dx, ux), ty = __builtin_elementwise_fma(c, dy, uy), tz = __builtin_elementwise_fma(c, dz, uz);
  q.ax = __builtin_elementwise_fma(dx, s, q.ax);
  q.ay = __builtin_elementwise_fma(dy, s, q.ay);
  q.az = __builtin_elementwise_fma(dz, s, q.az);
  q.jx = __builtin_elementwise_fma(tx, s, q.jx);
  q.jy = __builtin_elementwise_fma(ty, s, q.jy);
  q.jz = __builtin_elementwise_fma(tz, s, q.jz);
}

// What a lane keeps for its two bodies: fp32 packs them, body 0 in .x and body 1 in .y of every value; fp64 holds two scalars.
// No arrays: every value has a name, so every value has a register.
template <typename T> struct JerkLane;
template <> struct JerkLane<float> {
  f32x2 x, y, z, u, v, w;
  JerkSums<f32x2> q;
  __device__ __forceinline__ void load(int b, float4 p, float4 s) {
    if (b == 0) { x.x = p.x; y.x = p.y; z.x = p.z; u.x = s.x; v.x = s.y; w.x = s.z; }
    else { x.y = p.x; y.y = p.y; z.y = p.z; u.y = s.x; v.y = s.y; w.y = s.z; }
  }
  __device__ __forceinline__ void clear() {
    const f32x2 o = {0.0f, 0.0f};
    q.ax = q.ay = q.az = q.jx = q.jy = q.jz = o;
  }
  __device__ __forceinline__ JerkSums<float> sums(int b) const {
    if (b == 0) return JerkSums<float>{q.ax.x, q.ay.x, q.az.x, q.jx.x, q.jy.x, q.jz.x};
    return JerkSums<float>{q.ax.y, q.ay.y, q.az.y, q.jx.y, q.jy.y, q.jz.y};
  }
  __device__ __forceinline__ void tile(const float4* ptile, const float4* vtile) {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) jerk_pair2(ptile[j], whole_record(vtile, j), x, y, z, u, v, w, q);
  }
};
template <> struct JerkLane<double> {
  double x0, y0, z0, u0, v0, w0, x1, y1, z1, u1, v1, w1;
  JerkSums<double> q0, q1;
  __device__ __forceinline__ void load(int b, double4 p, double4 s) {
    if (b == 0) { x0 = p.x; y0 = p.y; z0 = p.z; u0 = s.x; v0 = s.y; w0 = s.z; }
    else { x1 = p.x; y1 = p.y; z1 = p.z; u1 = s.x; v1 = s.y; w1 = s.z; }
  }
  __device__ __forceinline__ void clear() {
    q0.ax = q0.ay = q0.az = q0.jx = q0.jy = q0.jz = 0.0;
    q1 = q0;
  }
  __device__ __forceinline__ JerkSums<double> sums(int b) const { return b == 0 ? q0 : q1; }
  __device__ __forceinline__ void tile(const double4* ptile, const double4* vtile) {
#pragma unroll 2
    for (int j = 0; j < kTile; ++j) {
      const double4 r = ptile[j];
      const double4 s = vtile[j];
      jerk_pair(r.x, r.y, r.z, r.w, s.x, s.y, s.z, x0, y0, z0, u0, v0, w0, q0);
      jerk_pair(r.x, r.y, r.z, r.w, s.x, s.y, s.z, x1, y1, z1, u1, v1, w1, q1);
    }
  }
};

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding) and whose velocity records velm[0 .. n) are read.  Writes, for
// every body below n of the column, records 2 * (split * n + body) and the next of parts.
template <typename T>
__device__ __forceinline__ void jerk_body(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                          const int n, const int tiles_per_split, typename V4<T>::type* __restrict__ parts, const int col,
                                          const int split) {
  using T4 = typename V4<T>::type;
  constexpr int B = kJerkBodies;
  __shared__ T4 ptile[kTile];
  __shared__ T4 vtile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  JerkLane<T> lane;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero, v = zero;
    if (li < n) {
      p = posm[li];
      v = velm[li];
    }
    lane.load(b, p, v);
  }
  lane.clear();
  TileWalk2<T4> walk(posm, velm, n, split, tiles_per_split);
  for (int k = walk.k0; k < walk.k1; ++k) {
    walk.stage(ptile, vtile, k);
    lane.tile(ptile, vtile);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) {
      const JerkSums<T> s = lane.sums(b);
      T4 o0, o1;
      o0.x = s.ax; o0.y = s.ay; o0.z = s.az; o0.w = (T)0;
      o1.x = s.jx; o1.y = s.jy; o1.z = s.jz; o1.w = (T)0;
      T4* row = parts + 2 * ((size_t)split * (size_t)n + (size_t)li);
      row[0] = o0;
      row[1] = o1;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void jerk_kernel(const typename V4<T>::type* __restrict__ posm,
                                                      const typename V4<T>::type* __restrict__ velm, int n, int tiles_per_split,
                                                      typename V4<T>::type* __restrict__ parts) {
  jerk_body<T>(posm, velm, n, tiles_per_split, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as the ensemble's step kernels have it: posm[S][n_alloc + kSgprOverread], velm[S][own_pad];
// parts[count][gridDim.y][n][2].
template <typename T>
struct EnsembleJerkArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* velm;  // member 0's velocities
  typename V4<T>::type* parts;       // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  unsigned vel_stride;               // records between members in velm
  int n, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_jerk_kernel(const EnsembleJerkArgs<T> e) {
  const size_t k = blockIdx.z;
  jerk_body<T>(e.posm + (e.first + k) * e.pos_stride, e.velm + (e.first + k) * e.vel_stride, e.n, e.tiles_per_split,
               e.parts + 2 * k * gridDim.y * (size_t)e.n, blockIdx.x, blockIdx.y);
}

struct JerkMember : VelMember {};

template <typename T>
struct RaggedJerkArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  const JerkMember* table;           // [members]
  typename V4<T>::type* parts;       // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_jerk_kernel(const RaggedJerkArgs<T> r) {
  const MemberGroup<JerkMember> g = member_group(r.table, r.first);
  if (g.elsewhere()) return;
  jerk_body<T>(r.posm + g.mem.pos_off, r.velm + g.mem.vel_off, g.mem.n, g.shape.tiles_per_split, r.parts + 2 * g.rel() * gridDim.y,
               blockIdx.x, blockIdx.y);
}

// Body idx of the call's `total` bodies, its member found by member_at..  The member has field_shape(n, n).splits rows of n
// record pairs; its rows begin at (the bodies of the range before it) * row_splits pairs, row_splits the gridDim.y of the
// pair-work launch..  Writes records 2 * idx and 2 * idx + 1 of out.
template <typename T>
__global__ __launch_bounds__(kBlock) void jerk_finish_kernel(const typename V4<T>::type* __restrict__ parts, const JerkMember* __restrict__ table,
                                                             unsigned first, int count, int n_all, int row_splits, unsigned total,
                                                             typename V4<T>::type* __restrict__ out) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const MemberAt at = member_at(table, first, count, n_all, idx);
  const int n = at.n;
  const size_t rel = at.rel;  // the bodies of the range before the body's member
  const int splits = field_shape(n, n).splits;
  const T4* row = parts + 2 * (rel * (size_t)row_splits + ((size_t)idx - rel));
  double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
  for (int s = 0; s < splits; ++s) {
    const T4 a = row[2 * (size_t)s * (size_t)n], b = row[2 * (size_t)s * (size_t)n + 1];
    ax += (double)a.x; ay += (double)a.y; az += (double)a.z;
    jx += (double)b.x; jy += (double)b.y; jz += (double)b.z;
  }
  T4 o0, o1;
  o0.x = (T)ax; o0.y = (T)ay; o0.z = (T)az; o0.w = (T)0;
  o1.x = (T)jx; o1.y = (T)jy; o1.z = (T)jz; o1.w = (T)0;
  out[2 * (size_t)idx] = o0;
  out[2 * (size_t)idx + 1] = o1;
}

}  // namespace nbx
