// nbx_advance_kernels.hpp -- the kernels of nbx_advance, nbx_ensemble_advance and nbx_ragged_advance (include/nbx_advance.h):
// fourth-order Hermite P(EC) steps whose size every system chooses for itself on the device, a power of two read from the
// system's clock record; three launches a step, nothing read back.  Instantiated by nbx_advance.hip alone.
//
//   advance_kernel<T>            grid (columns, splits), block 256          a context that owns all n bodies, clock record 0
//   ensemble_advance_kernel<T>   grid (columns, splits, members), block 256  member blockIdx.z, clock record blockIdx.z
//   ragged_advance_kernel<T>     grid (largest columns, largest splits of the members, members), block 256: the workgroup reads
//                                its member's {pos_off, vel_off, out_off, n} from the table, evaluates field_shape(n, n) itself
//                                and returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three read the system's clock record first -- one address for the whole workgroup, so scalar loads -- return at once
//     where predict != 0 and the record's t >= t_end (the system is done), and run advance_body with {h, k2, k6, h3} of the
//     record: the fixed stepper's pair work restated -- 256 threads, two bodies per lane, the j range of the workgroup's split in
//     256-record tiles staged in LDS, two arrays per tile (positions, velocities), the next tile prefetched into registers, the
//     predictor fused into the loads, nothing masked, no predicted state written to memory.  predict == 0: the loads alone, the
//     kept records and the clock record's values not used -- the evaluation at the resident state that starts a call without
//     `resume`, which no system skips.
//   advance_finish_kernel<T>     one thread per body of the object: the fixed stepper's finish -- the body's partial records added
//                                in fp64 in split order, rounded once to T (a1, j1), the corrector with k2, k6 of the system's
//                                clock record, x1 and v1 stored in place, {a1, 0}, {j1, 0} kept -- plus the body's candidate s_i
//                                (below), one double at cand[body].  A thread of a done system returns before it reads
//                                anything else.  correct == 0: the kept records and the starting candidate alone.
//   advance_clock_kernel         grid (systems), block 256: a strided minimum over the system's candidates, the 256 minima
//                                reduced through LDS, and thread 0 runs the quantiser and writes the clock record.  A done
//                                system's record is left alone.  start != 0: the record is made from nothing (t = 0).
//
// One pair, in T: the pair of the acceleration's time derivative, restated (advance_pair, advance_pair2): the same operations in
// the same order as the fixed stepper's, so the same bits from the same records.
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))
//   ux,uy,uz = v_j - v_i;  rv = fma(dx,ux, fma(dy,uy, dz*uz))
//   fp32:  inv = rsq(r2);  inv2 = inv*inv;  s = (gm*inv)*inv2;  a += d*s (fma)
//          c = (rv*inv2)*(-3);  t_a = fma(c, d_a, u_a);  adot_a += t_a*s (fma)       26 packed VALU and 2 v_rsq_f32 per j record
//   fp64:  y = v_rsq_f64(r2);  y2 = y*y;  h = fma(-r2, y2, 1)
//          s = ((gm*y)*y2) * fma(h, fma(h, 15, 12), 8);  inv2 = fma(y2, fma(h, h, h), y2);  c, t and the sums as in fp32
//
// Predictor and corrector, per component, every operation a separately rounded fp64 multiply or add (mul_rn / add_rn), innermost
// bracket first; x, v, a0, j0, a1, j1 are T values widened; h, k2, k6, h3 come from the clock record:
//   vp = v + h*(a0 + k2*j0)             xp = x + h*(v + k2*(a0 + h3*j0))            each rounded once to T
//   v1 = v + k2*((a0 + a1) + k6*(j0 - j1))   x1 = x + k2*((v + v1) + k6*(a0 - a1))  the unrounded v1 enters x1; each rounded once
//
// The candidate of a body after a step of h (ih = 1 / h), fp64, mul_rn / add_rn and one correctly rounded sqrt and division each
// where written, per component first:
//   d = a0 - a1;  a2 = (((-6 d) - h*((4 j0) + (2 j1))) * ih) * ih;  a3 = ((((12 d) + (6 h)*(j0 + j1)) * ih) * ih) * ih
//   a2 = a2 + h*a3;  |v|^2 = (vx*vx + vy*vy) + vz*vz;  A = |a1|^2, J = |j1|^2, S = |a2|^2, C = |a3|^2
//   s_i = (sqrt(A*S) + J) / (sqrt(J*C) + S) where the denominator is > 0, else +inf;  at the start: A / J where J > 0, else +inf
//
// The quantiser (advance_choose), integers only: E = the exponent field of eta2 * q minus 1023, k_crit = E >> 1 (the floor of
// E / 2); with k the exponent of the step just taken, k + 1 if k_crit > k and t is a multiple of 2^(k+1), else k if k_crit >= k,
// else k_crit; at the start k_crit; clamped to [k_cap - levels, k_cap].  h = dt_cap * 2^(k - k_cap) and ih = (1 / dt_cap) *
// 2^(k_cap - k), the powers of two made from their bits: exact, no division and no logarithm on the device.
//
// Partials and kept records: the fixed stepper's layout -- two records of T per (split, body) at 2 * (split * n + body) of the
// system's rows, a system's rows beginning at 2 * (the bodies of the systems before it) * gridDim.y; {a0, 0} and {j0, 0} of body
// i at 2 * (vel_off + i) and the record after it.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kAdvanceBodies = 2;                         // bodies per lane (fp32: one packed pair)
constexpr long long kAdvanceMaxBodies = kFieldMaxPoints;  // per object (include/nbx_advance.h, status 7)
constexpr int kAdvanceMaxLevels = 40;

// One system's clock, on the device.  h is a power of two; k2 = h / 2, ih = 1 / h exactly; k6 = h * (1.0 / 6.0) and
// h3 = h * (1.0 / 3.0) are the host's h / 6.0 and h / 3.0 bit for bit (scaling by a power of two commutes with rounding).
struct AdvanceClock {
  double t, h, k2, k6, h3, ih;
  double h_last;           // the step last taken (0: none)
  long long steps;         // taken since the call without resume
  long long floor_steps;   // of those, taken at the floor although the criterion asked for less
  int floor_next;          // the step of size h will be such a step
  int reserved;
};

// the step constants the predictor and the corrector read
struct AdvanceConsts {
  double h, k2, k6, h3;
};

// what every kernel is told about time
struct AdvanceTime {
  const AdvanceClock* clocks;  // [systems]
  double t_end;
};

__device__ __forceinline__ double adv_sub_rn(double x, double y) { return add_rn(x, -y); }

// (x, v) -> (xp, vp) of one body: p the position record (.w = gm, kept), v the velocity record, a and j the kept records
template <typename T>
__device__ __forceinline__ void advance_predict(typename V4<T>::type& p, typename V4<T>::type& v, const typename V4<T>::type a,
                                                const typename V4<T>::type j, const AdvanceConsts k) {
#define NBX_ADVANCE_PREDICT(c)                                                                             \
  {                                                                                                        \
    const double x0 = (double)p.c, v0 = (double)v.c, a0 = (double)a.c, j0 = (double)j.c;                   \
    const double vp = add_rn(v0, mul_rn(k.h, add_rn(a0, mul_rn(k.k2, j0))));                               \
    const double xp = add_rn(x0, mul_rn(k.h, add_rn(v0, mul_rn(k.k2, add_rn(a0, mul_rn(k.h3, j0))))));     \
    p.c = (T)xp;                                                                                           \
    v.c = (T)vp;                                                                                           \
  }
  NBX_ADVANCE_PREDICT(x)
  NBX_ADVANCE_PREDICT(y)
  NBX_ADVANCE_PREDICT(z)
#undef NBX_ADVANCE_PREDICT
}

// the six sums of one body
template <typename V>
struct AdvanceSums {
  V ax, ay, az, jx, jy, jz;
};

// one pair of the scalar form (fp64)
__device__ __forceinline__ void advance_pair(double xj, double yj, double zj, double gmj, double uj, double vj, double wj, double xi,
                                             double yi, double zi, double ui, double vi, double wi, AdvanceSums<double>& q) {
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
__device__ __forceinline__ void advance_pair2(const float4 r, const float4 w, f32x2 xi, f32x2 yi, f32x2 zi, f32x2 ui, f32x2 vi, f32x2 wi,
                                              AdvanceSums<f32x2>& q) {
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
template <typename T> struct AdvanceLane;
template <> struct AdvanceLane<float> {
  f32x2 x, y, z, u, v, w;
  AdvanceSums<f32x2> q;
  __device__ __forceinline__ void load(int b, float4 p, float4 s) {
    if (b == 0) { x.x = p.x; y.x = p.y; z.x = p.z; u.x = s.x; v.x = s.y; w.x = s.z; }
    else { x.y = p.x; y.y = p.y; z.y = p.z; u.y = s.x; v.y = s.y; w.y = s.z; }
  }
  __device__ __forceinline__ void clear() {
    const f32x2 o = {0.0f, 0.0f};
    q.ax = q.ay = q.az = q.jx = q.jy = q.jz = o;
  }
  __device__ __forceinline__ AdvanceSums<float> sums(int b) const {
    if (b == 0) return AdvanceSums<float>{q.ax.x, q.ay.x, q.az.x, q.jx.x, q.jy.x, q.jz.x};
    return AdvanceSums<float>{q.ax.y, q.ay.y, q.az.y, q.jx.y, q.jy.y, q.jz.y};
  }
  __device__ __forceinline__ void tile(const float4* ptile, const float4* vtile) {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) advance_pair2(ptile[j], whole_record(vtile, j), x, y, z, u, v, w, q);
  }
};
template <> struct AdvanceLane<double> {
  double x0, y0, z0, u0, v0, w0, x1, y1, z1, u1, v1, w1;
  AdvanceSums<double> q0, q1;
  __device__ __forceinline__ void load(int b, double4 p, double4 s) {
    if (b == 0) { x0 = p.x; y0 = p.y; z0 = p.z; u0 = s.x; v0 = s.y; w0 = s.z; }
    else { x1 = p.x; y1 = p.y; z1 = p.z; u1 = s.x; v1 = s.y; w1 = s.z; }
  }
  __device__ __forceinline__ void clear() {
    q0.ax = q0.ay = q0.az = q0.jx = q0.jy = q0.jz = 0.0;
    q1 = q0;
  }
  __device__ __forceinline__ AdvanceSums<double> sums(int b) const { return b == 0 ? q0 : q1; }
  __device__ __forceinline__ void tile(const double4* ptile, const double4* vtile) {
#pragma unroll 2
    for (int j = 0; j < kTile; ++j) {
      const double4 r = ptile[j];
      const double4 s = vtile[j];
      advance_pair(r.x, r.y, r.z, r.w, s.x, s.y, s.z, x0, y0, z0, u0, v0, w0, q0);
      advance_pair(r.x, r.y, r.z, r.w, s.x, s.y, s.z, x1, y1, z1, u1, v1, w1, q1);
    }
  }
};

// The four records of one body as they are loaded, and the two that are staged.  Record j of a system of n bodies: the position
// record always (the tail of the position buffer is zero padding), the other three only where j < n.
template <typename T>
struct AdvanceRecords {
  typename V4<T>::type p, v, a, j;
  __device__ __forceinline__ void load(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                       const typename V4<T>::type* __restrict__ keep, const int i, const int n, const bool with_pos,
                                       const int predict) {
    typename V4<T>::type zero;
    zero.x = zero.y = zero.z = zero.w = (T)0;
    p = v = a = j = zero;
    if (with_pos) p = posm[i];
    if (i < n) {
      v = velm[i];
      if (predict) {
        a = keep[2 * (size_t)i];
        j = keep[2 * (size_t)i + 1];
      }
    }
  }
  // p, v become the records the pair work sees
  __device__ __forceinline__ void advance(const int predict, const AdvanceConsts k) {
    if (predict) advance_predict<T>(p, v, a, j, k);
  }
};

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), whose velocity records velm[0 .. n) and kept records
// keep[0 .. 2 n) are read.  Writes, for every body below n of the column, records 2 * (split * n + body) and the next of parts.
template <typename T>
__device__ __forceinline__ void advance_body(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                             const typename V4<T>::type* __restrict__ keep, const int n, const int tiles_per_split,
                                             typename V4<T>::type* __restrict__ parts, const int col, const int split, const int predict,
                                             const AdvanceConsts hc) {
  using T4 = typename V4<T>::type;
  constexpr int B = kAdvanceBodies;
  __shared__ T4 ptile[kTile];
  __shared__ T4 vtile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  AdvanceLane<T> lane;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    AdvanceRecords<T> own;
    own.load(posm, velm, keep, li, n, li < n, predict);
    own.advance(predict, hc);
    lane.load(b, own.p, own.v);
  }
  lane.clear();
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  AdvanceRecords<T> next;
  next.load(posm, velm, keep, k0 * kTile + t, n, k0 < k1, predict);
  for (int k = k0; k < k1; ++k) {
    next.advance(predict, hc);
    __syncthreads();  // every lane is done with the previous tile
    ptile[t] = next.p;
    vtile[t] = next.v;
    __syncthreads();
    if (k + 1 < k1) next.load(posm, velm, keep, (k + 1) * kTile + t, n, true, predict);
    lane.tile(ptile, vtile);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) {
      const AdvanceSums<T> s = lane.sums(b);
      T4 o0, o1;
      o0.x = s.ax; o0.y = s.ay; o0.z = s.az; o0.w = (T)0;
      o1.x = s.jx; o1.y = s.jy; o1.z = s.jz; o1.w = (T)0;
      T4* row = parts + 2 * ((size_t)split * (size_t)n + (size_t)li);
      row[0] = o0;
      row[1] = o1;
    }
  }
}

// The system's clock record as the workgroup's step constants; *done: the system has reached t_end.  One address per workgroup.
__device__ __forceinline__ AdvanceConsts advance_consts(const AdvanceTime tm, const size_t system, bool* done) {
  const AdvanceClock* __restrict__ ck = tm.clocks + system;
  *done = ck->t >= tm.t_end;
  return AdvanceConsts{ck->h, ck->k2, ck->k6, ck->h3};
}

template <typename T>
struct AdvanceArgs {
  const typename V4<T>::type* posm;  // the current records
  const typename V4<T>::type* velm;
  const typename V4<T>::type* keep;  // {a0, 0}, {j0, 0} per velocity record
  typename V4<T>::type* parts;
  int n, tiles_per_split, predict;
  AdvanceTime tm;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void advance_kernel(const AdvanceArgs<T> a) {
  bool done;
  const AdvanceConsts hc = advance_consts(a.tm, 0, &done);
  if (a.predict && done) return;  // the whole workgroup
  advance_body<T>(a.posm, a.velm, a.keep, a.n, a.tiles_per_split, a.parts, blockIdx.x, blockIdx.y, a.predict, hc);
}

// Layout, member-major as the ensemble's step kernels have it: posm[S][n_alloc + kSgprOverread], velm[S][own_pad],
// keep[S][own_pad][2]; parts[S][gridDim.y][n][2].
template <typename T>
struct EnsembleAdvanceArgs {
  AdvanceArgs<T> member0;  // member 0's records and rows
  unsigned pos_stride;     // records between members in posm
  unsigned vel_stride;     // records between members in velm
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_advance_kernel(const EnsembleAdvanceArgs<T> e) {
  const size_t k = blockIdx.z;
  const AdvanceArgs<T>& a = e.member0;
  bool done;
  const AdvanceConsts hc = advance_consts(a.tm, k, &done);
  if (a.predict && done) return;
  advance_body<T>(a.posm + k * e.pos_stride, a.velm + k * e.vel_stride, a.keep + 2 * k * e.vel_stride, a.n, a.tiles_per_split,
                  a.parts + 2 * k * gridDim.y * (size_t)a.n, blockIdx.x, blockIdx.y, a.predict, hc);
}

// the fixed stepper's table (the same layout: whichever call comes first builds it)
struct AdvanceMember : VelMember {};

template <typename T>
struct RaggedAdvanceArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  const typename V4<T>::type* keep;  // the kept records of all members
  const AdvanceMember* table;        // [members]
  typename V4<T>::type* parts;
  int predict;
  AdvanceTime tm;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_advance_kernel(const RaggedAdvanceArgs<T> r) {
  const MemberGroup<AdvanceMember> g = member_group(r.table, 0u);
  if (g.elsewhere()) return;
  const AdvanceMember& mem = g.mem;
  const FieldShape& s = g.shape;
  bool done;
  const AdvanceConsts hc = advance_consts(r.tm, blockIdx.z, &done);
  if (r.predict && done) return;
  advance_body<T>(r.posm + mem.pos_off, r.velm + mem.vel_off, r.keep + 2 * mem.vel_off, mem.n, s.tiles_per_split,
                  r.parts + 2 * (size_t)mem.out_off * gridDim.y, blockIdx.x, blockIdx.y, r.predict, hc);
}

// |v|^2 = (vx*vx + vy*vy) + vz*vz, each operation rounded
__device__ __forceinline__ double advance_norm2(double x, double y, double z) {
  return add_rn(add_rn(mul_rn(x, x), mul_rn(y, y)), mul_rn(z, z));
}

// Body idx of the object's `total` bodies.  table == nullptr: every system has n_all bodies, member idx / n_all at
// pos_stride / vel_stride records from the one before.  Otherwise the member is the last of table[0 .. members) whose out_off is
// not above idx.  The member has field_shape(n, n).splits rows of n record pairs; its rows begin at (the bodies before it) *
// row_splits pairs, row_splits the gridDim.y of the pair-work launch.  The body's candidate goes to cand[idx].
template <typename T>
struct AdvanceFinishArgs {
  const typename V4<T>::type* parts;
  const AdvanceMember* table;
  typename V4<T>::type* posm;  // the current records: x1 is stored here
  typename V4<T>::type* velm;
  typename V4<T>::type* keep;
  double* cand;                // [total]
  unsigned pos_stride, vel_stride;
  int members, n_all, row_splits, correct;
  unsigned total;
  AdvanceTime tm;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void advance_finish_kernel(const AdvanceFinishArgs<T> f) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= f.total) return;
  int n = f.n_all;
  size_t system = 0, rel = 0, pos_off = 0, vel_off = 0;  // the bodies before the body's member; the member's first records
  if (f.table) {
    int lo = 0, hi = f.members - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (f.table[mid].out_off <= idx) lo = mid;
      else hi = mid - 1;
    }
    const AdvanceMember mem = f.table[lo];
    system = (size_t)lo;
    n = mem.n;
    rel = (size_t)mem.out_off;
    pos_off = (size_t)mem.pos_off;
    vel_off = (size_t)mem.vel_off;
  } else {
    system = idx / (unsigned)f.n_all;
    rel = system * (size_t)f.n_all;
    pos_off = system * f.pos_stride;
    vel_off = system * f.vel_stride;
  }
  const AdvanceClock ck = f.tm.clocks[system];
  if (f.correct && ck.t >= f.tm.t_end) return;  // a done system: nothing is written
  const size_t i = (size_t)idx - rel;
  const int splits = field_shape(n, n).splits;
  const T4* row = f.parts + 2 * (rel * (size_t)f.row_splits + i);
  double ax = 0.0, ay = 0.0, az = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
  for (int s = 0; s < splits; ++s) {
    const T4 a = row[2 * (size_t)s * (size_t)n], b = row[2 * (size_t)s * (size_t)n + 1];
    ax += (double)a.x; ay += (double)a.y; az += (double)a.z;
    jx += (double)b.x; jy += (double)b.y; jz += (double)b.z;
  }
  T4 a1, j1;
  a1.x = (T)ax; a1.y = (T)ay; a1.z = (T)az; a1.w = (T)0;
  j1.x = (T)jx; j1.y = (T)jy; j1.z = (T)jz; j1.w = (T)0;
  T4* kept = f.keep + 2 * (vel_off + i);
  const double inf = __builtin_huge_val();
  const double A = advance_norm2((double)a1.x, (double)a1.y, (double)a1.z);
  const double J = advance_norm2((double)j1.x, (double)j1.y, (double)j1.z);
  double s_i = inf;
  if (f.correct) {
    const T4 a0 = kept[0], j0 = kept[1];
    T4 p = f.posm[pos_off + i], v = f.velm[vel_off + i];
    const double h = ck.h, ih = ck.ih, k2 = ck.k2, k6 = ck.k6;
    const double h6 = mul_rn(6.0, h);
    double a2x, a2y, a2z, a3x, a3y, a3z;
#define NBX_ADVANCE_CORRECT(c)                                                                                                   \
  {                                                                                                                              \
    const double x0 = (double)p.c, v0 = (double)v.c;                                                                             \
    const double v1 = add_rn(v0, mul_rn(k2, add_rn(add_rn((double)a0.c, (double)a1.c), mul_rn(k6, adv_sub_rn((double)j0.c, (double)j1.c))))); \
    const double x1 = add_rn(x0, mul_rn(k2, add_rn(add_rn(v0, v1), mul_rn(k6, adv_sub_rn((double)a0.c, (double)a1.c)))));        \
    p.c = (T)x1;                                                                                                                 \
    v.c = (T)v1;                                                                                                                 \
    const double d = adv_sub_rn((double)a0.c, (double)a1.c);                                                                     \
    const double m2 = adv_sub_rn(mul_rn(-6.0, d), mul_rn(h, add_rn(mul_rn(4.0, (double)j0.c), mul_rn(2.0, (double)j1.c))));      \
    const double m3 = add_rn(mul_rn(12.0, d), mul_rn(h6, add_rn((double)j0.c, (double)j1.c)));                                   \
    a3##c = mul_rn(mul_rn(mul_rn(m3, ih), ih), ih);                                                                              \
    a2##c = add_rn(mul_rn(mul_rn(m2, ih), ih), mul_rn(h, a3##c));                                                                \
  }
    NBX_ADVANCE_CORRECT(x)
    NBX_ADVANCE_CORRECT(y)
    NBX_ADVANCE_CORRECT(z)
#undef NBX_ADVANCE_CORRECT
    f.posm[pos_off + i] = p;  // .w, gm, as it was
    f.velm[vel_off + i] = v;  // .w, the mass, as it was
    const double S = advance_norm2(a2x, a2y, a2z), C = advance_norm2(a3x, a3y, a3z);
    const double num = add_rn(__builtin_sqrt(mul_rn(A, S)), J);
    const double den = add_rn(__builtin_sqrt(mul_rn(J, C)), S);
    if (den > 0.0) s_i = num / den;
  } else {
    if (J > 0.0) s_i = A / J;
  }
  kept[0] = a1;
  kept[1] = j1;
  f.cand[idx] = s_i;
}

// 2^d for |d| <= 1022, from its bits
__device__ __forceinline__ double advance_pow2(const int d) { return __longlong_as_double((long long)(d + 1023) << 52); }

// the exponent field of x minus 1023 (x >= 0: no sign to mask)
__device__ __forceinline__ int advance_exponent(const double x) { return (int)((__double_as_longlong(x) >> 52) & 0x7ff) - 1023; }

struct AdvanceClockArgs {
  const double* cand;          // [bodies of the object]
  AdvanceClock* clocks;        // [systems]
  const AdvanceMember* table;  // nullptr: every system has n_all candidates
  int n_all, start;
  double t_end, eta2, dt_cap, inv_cap;  // inv_cap = 1 / dt_cap
  int k_cap, levels;
};

// The exponent of the next step.  start: no step has been taken.  *raised: the floor lifted it.
__device__ __forceinline__ int advance_choose(const double q, const AdvanceClockArgs& a, const int start, const int k, const double t,
                                              const double ih, int* raised) {
  const int k_crit = advance_exponent(mul_rn(a.eta2, q)) >> 1;  // an arithmetic shift: the floor of E / 2
  int next = k_crit;
  if (!start && k_crit >= k) {
    const double u = mul_rn(t, mul_rn(0.5, ih));  // t / 2^(k+1), exact
    next = (k_crit > k && u == __builtin_floor(u)) ? k + 1 : k;
  }
  const int k_floor = a.k_cap - a.levels;
  *raised = next < k_floor;
  return next < k_floor ? k_floor : (next > a.k_cap ? a.k_cap : next);
}

__global__ __launch_bounds__(kBlock) void advance_clock_kernel(const AdvanceClockArgs a) {
  __shared__ double low[kBlock];
  const unsigned system = blockIdx.x;
  AdvanceClock ck = a.clocks[system];
  if (!a.start && ck.t >= a.t_end) return;  // done: the record stays as it is (the whole workgroup)
  size_t off = (size_t)system * (size_t)a.n_all;
  int n = a.n_all;
  if (a.table) {
    off = (size_t)a.table[system].out_off;
    n = a.table[system].n;
  }
  const int t = threadIdx.x;
  double q = __builtin_huge_val();
  for (int i = t; i < n; i += kBlock) {
    const double c = a.cand[off + i];
    if (c < q) q = c;  // a NaN is never selected
  }
  low[t] = q;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (t < s && low[t + s] < low[t]) low[t] = low[t + s];
    __syncthreads();
  }
  if (t != 0) return;
  q = low[0];
  int k = 0;
  if (a.start) {
    ck.t = 0.0;
    ck.h_last = 0.0;
    ck.steps = 0;
    ck.floor_steps = 0;
  } else {
    k = advance_exponent(ck.h);
    ck.t = add_rn(ck.t, ck.h);  // exact: t is a multiple of h and t / h < 2^52
    ck.h_last = ck.h;
    ck.steps += 1;
    ck.floor_steps += ck.floor_next;
  }
  int raised = 0;
  const int next = advance_choose(q, a, a.start, k, ck.t, ck.ih, &raised);
  ck.h = mul_rn(a.dt_cap, advance_pow2(next - a.k_cap));
  ck.ih = mul_rn(a.inv_cap, advance_pow2(a.k_cap - next));
  ck.k2 = mul_rn(ck.h, 0.5);
  ck.k6 = mul_rn(ck.h, 1.0 / 6.0);
  ck.h3 = mul_rn(ck.h, 1.0 / 3.0);
  ck.floor_next = raised;
  ck.reserved = 0;
  a.clocks[system] = ck;
}

}  // namespace nbx
