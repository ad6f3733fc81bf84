// nbx_hermite_kernels.hpp -- the kernels of nbx_hermite_step, nbx_ensemble_hermite_step and nbx_ragged_hermite_step
// (include/nbx_hermite.h): one fourth-order Hermite P(EC) step of every body of every system in two launches, nothing read back.
// Instantiated by nbx_hermite.hip alone.
//
//   hermite_kernel<T>            grid (columns, splits), block 256          a context that owns all n bodies
//   ensemble_hermite_kernel<T>   grid (columns, splits, members), block 256  member blockIdx.z
//   ragged_hermite_kernel<T>     grid (largest columns, largest splits of the members, members), block 256: the workgroup reads
//                                its member's {pos_off, vel_off, out_off, n} from the table, evaluates field_shape(n, n) itself
//                                and returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three run hermite_body: the pair work of the acceleration and its time derivative -- 256 threads, two bodies per lane,
//     the j range of the workgroup's split in 256-record tiles staged in LDS, two arrays per tile (positions, velocities), the next
//     tile prefetched into registers -- at the PREDICTED state.  The predictor is fused into the loads: for every j record of a
//     tile one thread loads the position record, and where j < n the velocity record and the kept {a0, j0} records (zeros
//     otherwise: what lies behind a system's last record of these three is never read), predicts in fp64 and stages
//     {xp, yp, zp, gm} and {up, vp, wp, .}; the lane's own two bodies are predicted by the same function.  Every workgroup
//     predicts with the same operations, so j == i still has d = u = 0 exactly, and nothing is masked.  A padding record
//     predicts to itself: 0 + h * (0 + ...) = 0.  No predicted state is written to memory.  predict == 0: the loads alone, the
//     kept records not read -- the evaluation at the resident state that starts a call without `resume`.
//   hermite_finish_kernel<T>     one thread per body of the object: adds the body's partial records in fp64 in split order and
//                                rounds once to T (a1, j1), corrects, stores x1 into the body's position record and v1 into its
//                                velocity record (.w of both untouched) and {a1, 0}, {j1, 0} into the kept records.  A thread
//                                touches its own body only and the pair launch has finished: the update is in place.
//                                correct == 0: the kept records alone.
//
// One pair, in T, is the pair of the acceleration's time derivative, restated (hermite_pair, hermite_pair2): the same operations
// in the same order, so the same bits from the same records.
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))
//   ux,uy,uz = v_j - v_i;  rv = fma(dx,ux, fma(dy,uy, dz*uz))
//   fp32:  inv = rsq(r2);  inv2 = inv*inv;  s = (gm*inv)*inv2;  a += d*s (fma)
//          c = (rv*inv2)*(-3);  t_a = fma(c, d_a, u_a);  adot_a += t_a*s (fma)       26 packed VALU and 2 v_rsq_f32 per j record
//   fp64:  y = v_rsq_f64(r2);  y2 = y*y;  h = fma(-r2, y2, 1)
//          s = ((gm*y)*y2) * fma(h, fma(h, 15, 12), 8);  inv2 = fma(y2, fma(h, h, h), y2);  c, t and the sums as in fp32
//
// Predictor and corrector, per component, every operation a separately rounded fp64 multiply or add (mul_rn / add_rn: no build
// contracts one), innermost bracket first; x, v, a0, j0, a1, j1 are T values widened; h, k2 = h/2, k6 = h/6, h3 = h/3 come from
// the host:
//   vp = v + h*(a0 + k2*j0)             xp = x + h*(v + k2*(a0 + h3*j0))            each rounded once to T
//   v1 = v + k2*((a0 + a1) + k6*(j0 - j1))   x1 = x + k2*((v + v1) + k6*(a0 - a1))  the unrounded v1 enters x1; each rounded once
//
// Partials: two records of T per (split, body), {ax, ay, az, 0} and {jx, jy, jz, 0}, at 2 * (split * n + body) and the record
// after it of the system's rows; a system's rows begin at 2 * (the bodies of the systems before it) * gridDim.y.  Kept records:
// {a0, 0} and {j0, 0} of body i at 2 * (vel_off + i) and the record after it, vel_off the system's first velocity record.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kHermiteBodies = 2;                         // bodies per lane (fp32: one packed pair)
constexpr long long kHermiteMaxBodies = kFieldMaxPoints;  // per object (include/nbx_hermite.h, status 4)

// the host's constants: h = dt rounded once to T and widened, k2 = h * 0.5, k6 = h / 6.0, h3 = h / 3.0, each computed once in fp64
struct HermiteConsts {
  double h, k2, k6, h3;
};

// x - y, separately rounded: the sign flip is exact
__device__ __forceinline__ double sub_rn(double x, double y) { return add_rn(x, -y); }

// (x, v) -> (xp, vp) of one body: p the position record (.w = gm, kept), v the velocity record, a and j the kept records
template <typename T>
__device__ __forceinline__ void hermite_predict(typename V4<T>::type& p, typename V4<T>::type& v, const typename V4<T>::type a,
                                                const typename V4<T>::type j, const HermiteConsts k) {
#define NBX_HERMITE_PREDICT(c)                                                                             \
  {                                                                                                        \
    const double x0 = (double)p.c, v0 = (double)v.c, a0 = (double)a.c, j0 = (double)j.c;                   \
    const double vp = add_rn(v0, mul_rn(k.h, add_rn(a0, mul_rn(k.k2, j0))));                               \
    const double xp = add_rn(x0, mul_rn(k.h, add_rn(v0, mul_rn(k.k2, add_rn(a0, mul_rn(k.h3, j0))))));     \
    p.c = (T)xp;                                                                                           \
    v.c = (T)vp;                                                                                           \
  }
  NBX_HERMITE_PREDICT(x)
  NBX_HERMITE_PREDICT(y)
  NBX_HERMITE_PREDICT(z)
#undef NBX_HERMITE_PREDICT
}

// the six sums of one body
template <typename V>
struct HermiteSums {
  V ax, ay, az, jx, jy, jz;
};

// one pair of the scalar form (fp64)
__device__ __forceinline__ void hermite_pair(double xj, double yj, double zj, double gmj, double uj, double vj, double wj, double xi,
                                             double yi, double zi, double ui, double vi, double wi, HermiteSums<double>& q) {
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
__device__ __forceinline__ void hermite_pair2(const float4 r, const float4 w, f32x2 xi, f32x2 yi, f32x2 zi, f32x2 ui, f32x2 vi, f32x2 wi,
                                              HermiteSums<f32x2>& q) {
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
template <typename T> struct HermiteLane;
template <> struct HermiteLane<float> {
  f32x2 x, y, z, u, v, w;
  HermiteSums<f32x2> q;
  __device__ __forceinline__ void load(int b, float4 p, float4 s) {
    if (b == 0) { x.x = p.x; y.x = p.y; z.x = p.z; u.x = s.x; v.x = s.y; w.x = s.z; }
    else { x.y = p.x; y.y = p.y; z.y = p.z; u.y = s.x; v.y = s.y; w.y = s.z; }
  }
  __device__ __forceinline__ void clear() {
    const f32x2 o = {0.0f, 0.0f};
    q.ax = q.ay = q.az = q.jx = q.jy = q.jz = o;
  }
  __device__ __forceinline__ HermiteSums<float> sums(int b) const {
    if (b == 0) return HermiteSums<float>{q.ax.x, q.ay.x, q.az.x, q.jx.x, q.jy.x, q.jz.x};
    return HermiteSums<float>{q.ax.y, q.ay.y, q.az.y, q.jx.y, q.jy.y, q.jz.y};
  }
  __device__ __forceinline__ void tile(const float4* ptile, const float4* vtile) {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) hermite_pair2(ptile[j], whole_record(vtile, j), x, y, z, u, v, w, q);
  }
};
template <> struct HermiteLane<double> {
  double x0, y0, z0, u0, v0, w0, x1, y1, z1, u1, v1, w1;
  HermiteSums<double> q0, q1;
  __device__ __forceinline__ void load(int b, double4 p, double4 s) {
    if (b == 0) { x0 = p.x; y0 = p.y; z0 = p.z; u0 = s.x; v0 = s.y; w0 = s.z; }
    else { x1 = p.x; y1 = p.y; z1 = p.z; u1 = s.x; v1 = s.y; w1 = s.z; }
  }
  __device__ __forceinline__ void clear() {
    q0.ax = q0.ay = q0.az = q0.jx = q0.jy = q0.jz = 0.0;
    q1 = q0;
  }
  __device__ __forceinline__ HermiteSums<double> sums(int b) const { return b == 0 ? q0 : q1; }
  __device__ __forceinline__ void tile(const double4* ptile, const double4* vtile) {
#pragma unroll 2
    for (int j = 0; j < kTile; ++j) {
      const double4 r = ptile[j];
      const double4 s = vtile[j];
      hermite_pair(r.x, r.y, r.z, r.w, s.x, s.y, s.z, x0, y0, z0, u0, v0, w0, q0);
      hermite_pair(r.x, r.y, r.z, r.w, s.x, s.y, s.z, x1, y1, z1, u1, v1, w1, q1);
    }
  }
};

// The four records of one body as they are loaded, and the two that are staged.  Record j of a system of n bodies: the position
// record always (the tail of the position buffer is zero padding), the other three only where j < n.
template <typename T>
struct HermiteRecords {
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
  __device__ __forceinline__ void advance(const int predict, const HermiteConsts k) {
    if (predict) hermite_predict<T>(p, v, a, j, k);
  }
};

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), whose velocity records velm[0 .. n) and kept records
// keep[0 .. 2 n) are read.  Writes, for every body below n of the column, records 2 * (split * n + body) and the next of parts.
template <typename T>
__device__ __forceinline__ void hermite_body(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                             const typename V4<T>::type* __restrict__ keep, const int n, const int tiles_per_split,
                                             typename V4<T>::type* __restrict__ parts, const int col, const int split, const int predict,
                                             const HermiteConsts hc) {
  using T4 = typename V4<T>::type;
  constexpr int B = kHermiteBodies;
  __shared__ T4 ptile[kTile];
  __shared__ T4 vtile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  HermiteLane<T> lane;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    HermiteRecords<T> own;
    own.load(posm, velm, keep, li, n, li < n, predict);
    own.advance(predict, hc);
    lane.load(b, own.p, own.v);
  }
  lane.clear();
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  HermiteRecords<T> next;
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
      const HermiteSums<T> s = lane.sums(b);
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
struct HermiteArgs {
  const typename V4<T>::type* posm;  // the current records
  const typename V4<T>::type* velm;
  const typename V4<T>::type* keep;  // {a0, 0}, {j0, 0} per velocity record
  typename V4<T>::type* parts;
  int n, tiles_per_split, predict;
  HermiteConsts hc;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void hermite_kernel(const HermiteArgs<T> a) {
  hermite_body<T>(a.posm, a.velm, a.keep, a.n, a.tiles_per_split, a.parts, blockIdx.x, blockIdx.y, a.predict, a.hc);
}

// Layout, member-major as the ensemble's step kernels have it: posm[S][n_alloc + kSgprOverread], velm[S][own_pad],
// keep[S][own_pad][2]; parts[S][gridDim.y][n][2].
template <typename T>
struct EnsembleHermiteArgs {
  HermiteArgs<T> member0;  // member 0's records and rows
  unsigned pos_stride;     // records between members in posm
  unsigned vel_stride;     // records between members in velm
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_hermite_kernel(const EnsembleHermiteArgs<T> e) {
  const size_t k = blockIdx.z;
  const HermiteArgs<T>& a = e.member0;
  hermite_body<T>(a.posm + k * e.pos_stride, a.velm + k * e.vel_stride, a.keep + 2 * k * e.vel_stride, a.n, a.tiles_per_split,
                  a.parts + 2 * k * gridDim.y * (size_t)a.n, blockIdx.x, blockIdx.y, a.predict, a.hc);
}

struct HermiteMember : VelMember {};

template <typename T>
struct RaggedHermiteArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  const typename V4<T>::type* keep;  // the kept records of all members
  const HermiteMember* table;        // [members]
  typename V4<T>::type* parts;
  int predict;
  HermiteConsts hc;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_hermite_kernel(const RaggedHermiteArgs<T> r) {
  const MemberGroup<HermiteMember> g = member_group(r.table, 0u);
  if (g.elsewhere()) return;
  const HermiteMember& mem = g.mem;
  const FieldShape& s = g.shape;
  hermite_body<T>(r.posm + mem.pos_off, r.velm + mem.vel_off, r.keep + 2 * mem.vel_off, mem.n, s.tiles_per_split,
                  r.parts + 2 * (size_t)mem.out_off * gridDim.y, blockIdx.x, blockIdx.y, r.predict, r.hc);
}

// Body idx of the object's `total` bodies.  table == nullptr: every system has n_all bodies, member idx / n_all at
// pos_stride / vel_stride records from the one before.  Otherwise the member is the last of table[0 .. members) whose out_off is
// not above idx.  The member has field_shape(n, n).splits rows of n record pairs; its rows begin at (the bodies before it) *
// row_splits pairs, row_splits the gridDim.y of the pair-work launch.
template <typename T>
struct HermiteFinishArgs {
  const typename V4<T>::type* parts;
  const HermiteMember* table;
  typename V4<T>::type* posm;  // the current records: x1 is stored here
  typename V4<T>::type* velm;
  typename V4<T>::type* keep;
  unsigned pos_stride, vel_stride;
  int members, n_all, row_splits, correct;
  unsigned total;
  HermiteConsts hc;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void hermite_finish_kernel(const HermiteFinishArgs<T> f) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= f.total) return;
  int n = f.n_all;
  size_t rel = 0, pos_off = 0, vel_off = 0;  // the bodies before the body's member; the member's first records
  if (f.table) {
    int lo = 0, hi = f.members - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (f.table[mid].out_off <= idx) lo = mid;
      else hi = mid - 1;
    }
    const HermiteMember mem = f.table[lo];
    n = mem.n;
    rel = (size_t)mem.out_off;
    pos_off = (size_t)mem.pos_off;
    vel_off = (size_t)mem.vel_off;
  } else {
    const size_t m = idx / (unsigned)f.n_all;
    rel = m * (size_t)f.n_all;
    pos_off = m * f.pos_stride;
    vel_off = m * f.vel_stride;
  }
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
  if (f.correct) {
    const T4 a0 = kept[0], j0 = kept[1];
    T4 p = f.posm[pos_off + i], v = f.velm[vel_off + i];
    const double k2 = f.hc.k2, k6 = f.hc.k6;
#define NBX_HERMITE_CORRECT(c)                                                                                                   \
  {                                                                                                                              \
    const double x0 = (double)p.c, v0 = (double)v.c;                                                                             \
    const double v1 = add_rn(v0, mul_rn(k2, add_rn(add_rn((double)a0.c, (double)a1.c), mul_rn(k6, sub_rn((double)j0.c, (double)j1.c))))); \
    const double x1 = add_rn(x0, mul_rn(k2, add_rn(add_rn(v0, v1), mul_rn(k6, sub_rn((double)a0.c, (double)a1.c)))));            \
    p.c = (T)x1;                                                                                                                 \
    v.c = (T)v1;                                                                                                                 \
  }
    NBX_HERMITE_CORRECT(x)
    NBX_HERMITE_CORRECT(y)
    NBX_HERMITE_CORRECT(z)
#undef NBX_HERMITE_CORRECT
    f.posm[pos_off + i] = p;  // .w, gm, as it was
    f.velm[vel_off + i] = v;  // .w, the mass, as it was
  }
  kept[0] = a1;
  kept[1] = j1;
}

}  // namespace nbx
