// nbx_tidal_kernels.hpp -- the kernels of the six entry points of include/nbx_tidal.h: the tidal tensor of a system of n bodies
//     T_ab(p) = sum over j of G m_j [ 3 d_a d_b r2^(-5/2) - delta_ab r2^(-3/2) ],   d = x_j - p,   r2 = |d|^2 + eps^2
// at m caller-supplied points (points mode: every body counts) or at the bodies themselves (bodies mode: j == i is never formed).
// Instantiated by nbx_tidal.hip alone.
//
//   tidal_kernel<T, BODIES>            grid (columns, splits), block 256          a context (sliced or not: every position is resident)
//   ensemble_tidal_kernel<T, BODIES>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_tidal_kernel<T, BODIES>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads
//                                      its member's {pos_off, out_off, n} from the table, evaluates field_shape itself and returns
//                                      at once where blockIdx.x or blockIdx.y is not one of its member's; no work list
//     All run tidal_body, the shape of field_body (nbx_field_kernels.hpp): 256 threads, two points per lane, the j range of the
//     workgroup's split in 256-record tiles staged in LDS (ONE array, the position records, read whole), the next tile prefetched
//     into registers.  Columns, splits and tiles per split are field_shape(m, n) in points mode and field_shape(n, n) in bodies
//     mode (nbx_field_shape.hpp), a function of the sizes alone.  BODIES: the i side is the column's own position records.
//   tidal_finish_kernel<T>             one thread per point or body of the call: adds its partial records in fp64 in split order,
//                                      forms 3 S_ab - delta_ab Q in fp64 (one fma) and rounds once to T
//
// One pair, in T.  A point keeps seven sums over one split, j ascending: six S_ab = sum (d_a s5) d_b (fma) and Q = sum s3.
//   dx,dy,dz = x_j - p;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))          the force kernels' r2
//   fp32:  inv = rsq(r2);  inv2 = inv*inv;  s3 = (gm*inv)*inv2   (gm_inv_cube);  s5 = s3*inv2
//          u = d*s5;  S_ab += u_a*d_b (fma);  Q += s3
//          on the lane's two points per packed instruction: 3 subtracts, 3 fma (r2), 4 multiplies (inv2, the two of s3, s5),
//          3 multiplies (u), 6 fma (S), 1 add (Q) = 20 packed VALU and 2 v_rsq_f32 per two pairs
//   fp64:  y = v_rsq_f64(r2);  y2 = y*y;  h = fma(-r2, y2, 1)     the seed and its residual, shared by the cube and the fifth power
//          t3 = (gm*y)*y2;  s3 = t3 * fma(h, fma(h, 15, 12), 8)     gm_inv_cube, the same operations
//          s5 = (t3*y2) * fma(h, fma(h, 35, 20), 8)                 8 (1 + 5/2 h + 35/8 h^2); the next term 6.6 h^3 < 2^-65 for
//                                                                   seeds good to 2^-24 (|h| < 2^-23)
// gm is the record's .w = G*m * gm_prescale<T>().  The fp64 prescale, 1/8, meets the 8 folded into both polynomials -- powers of
// two, so every rounding is the one the unscaled operation would make: what leaves tidal_body carries no scale.
//
// A record at or beyond n -- the zero padding -- has gm = 0 and a finite r2 >= eps2: all seven of its terms are exact zeros, no
// mask is needed for it.  The self mask of bodies mode: body l0 + b*256 + t of a column is record t of tile 2*col + b, so only
// those two tiles of a column can hold a lane's own body, and in tile 2*col + b only the lane's point b can meet itself, at
// j == t.  TidalLane<T>::tile<SELF> with SELF = b replaces gm by 0 for that point at that record -- one compare and one select per
// record and lane; s3 = s5 = 0 follow exactly and the seven sums take exact zeros: the self term is never formed.  SELF = -1, every
// other tile and all of points mode, compiles no compare.  The choice is uniform over the workgroup.
//
// Partials: two records of T per (split, point): {Sxx, Sxy, Sxz, Syy} and {Syz, Szz, Q, spare}, at 2 * (split * m + point) and
// the record after it of the system's rows.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two points per lane: the self mask counts on it");

constexpr int kTidalPoints = 2;                              // points per lane (fp32: one packed pair)
constexpr long long kTidalMaxPoints = kFieldMaxPoints / 2;   // per call (include/nbx_tidal.h): two partial records per point

// the seven sums of one point
template <typename V>
struct TidalSums {
  V xx, xy, xz, yy, yz, zz, q;
};

// one pair of the scalar form (fp64)
__device__ __forceinline__ void tidal_pair(double xj, double yj, double zj, double gmj, double xi, double yi, double zi,
                                           TidalSums<double>& s) {
  const double dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const double r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<double>())));
  const double y = __builtin_amdgcn_rsq(r2);
  const double y2 = y * y;
  const double h = __builtin_fma(-r2, y2, 1.0);
  const double t3 = (gmj * y) * y2;
  const double q3 = __builtin_fma(h, __builtin_fma(h, 15.0, 12.0), 8.0);  // 8 (1 + 3/2 h + 15/8 h^2): gm_inv_cube's
  const double q5 = __builtin_fma(h, __builtin_fma(h, 35.0, 20.0), 8.0);  // 8 (1 + 5/2 h + 35/8 h^2)
  const double s3 = t3 * q3;
  const double s5 = (t3 * y2) * q5;
  const double ux = dx * s5, uy = dy * s5, uz = dz * s5;
  s.xx = fmaT(ux, dx, s.xx);
  s.xy = fmaT(ux, dy, s.xy);
  s.xz = fmaT(ux, dz, s.xz);
  s.yy = fmaT(uy, dy, s.yy);
  s.yz = fmaT(uy, dz, s.yz);
  s.zz = fmaT(uz, dz, s.zz);
  s.q = add_rn(s.q, s3);  // s3 is needed rounded for s5: no fma may swallow its last product
}

// two points per call on the packed-fp32 pipe; g: the record's G m for either point (a splat where nothing is masked)
__device__ __forceinline__ void tidal_pair2(float xj, float yj, float zj, f32x2 g, f32x2 xi, f32x2 yi, f32x2 zi, TidalSums<f32x2>& s) {
  const f32x2 dx = f32x2{xj, xj} - xi, dy = f32x2{yj, yj} - yi, dz = f32x2{zj, zj} - zi;
  const f32x2 e2 = {softening2<float>(), softening2<float>()};
  f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dx, dx, r2);
  f32x2 inv;
  inv.x = __builtin_amdgcn_rsqf(r2.x);
  inv.y = __builtin_amdgcn_rsqf(r2.y);
  const f32x2 inv2 = inv * inv;
  const f32x2 s3 = (g * inv) * inv2;
  const f32x2 s5 = s3 * inv2;
  const f32x2 ux = dx * s5, uy = dy * s5, uz = dz * s5;
  s.xx = __builtin_elementwise_fma(ux, dx, s.xx);
  s.xy = __builtin_elementwise_fma(ux, dy, s.xy);
  s.xz = __builtin_elementwise_fma(ux, dz, s.xz);
  s.yy = __builtin_elementwise_fma(uy, dy, s.yy);
  s.yz = __builtin_elementwise_fma(uy, dz, s.yz);
  s.zz = __builtin_elementwise_fma(uz, dz, s.zz);
  s.q = add_rn(s.q, s3);
}

// What a lane keeps for its two points: fp32 packs them, point 0 in .x and point 1 in .y of every value; fp64 holds two scalars.
// No arrays: every value has a name, so every value has a register.
template <typename T> struct TidalLane;
template <> struct TidalLane<float> {
  f32x2 x, y, z;
  TidalSums<f32x2> s;
  __device__ __forceinline__ void load(int b, float4 p) {
    if (b == 0) { x.x = p.x; y.x = p.y; z.x = p.z; }
    else { x.y = p.x; y.y = p.y; z.y = p.z; }
  }
  __device__ __forceinline__ void clear() {
    const f32x2 o = {0.0f, 0.0f};
    s.xx = s.xy = s.xz = s.yy = s.yz = s.zz = s.q = o;
  }
  __device__ __forceinline__ TidalSums<float> sums(int b) const {
    if (b == 0) return TidalSums<float>{s.xx.x, s.xy.x, s.xz.x, s.yy.x, s.yz.x, s.zz.x, s.q.x};
    return TidalSums<float>{s.xx.y, s.xy.y, s.xz.y, s.yy.y, s.yz.y, s.zz.y, s.q.y};
  }
  // SELF >= 0: the tile holds the column's bodies of point SELF, the lane's own at record threadIdx.x; SELF < 0: no mask
  template <int SELF>
  __device__ __forceinline__ void tile(const float4* tile) {
    const int t = threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = tile[j];
      f32x2 g = {r.w, r.w};
      if constexpr (SELF == 0) g.x = j == t ? 0.0f : r.w;
      if constexpr (SELF == 1) g.y = j == t ? 0.0f : r.w;
      tidal_pair2(r.x, r.y, r.z, g, x, y, z, s);
    }
  }
};
template <> struct TidalLane<double> {
  double x0, y0, z0, x1, y1, z1;
  TidalSums<double> s0, s1;
  __device__ __forceinline__ void load(int b, double4 p) {
    if (b == 0) { x0 = p.x; y0 = p.y; z0 = p.z; }
    else { x1 = p.x; y1 = p.y; z1 = p.z; }
  }
  __device__ __forceinline__ void clear() {
    s0.xx = s0.xy = s0.xz = s0.yy = s0.yz = s0.zz = s0.q = 0.0;
    s1 = s0;
  }
  __device__ __forceinline__ TidalSums<double> sums(int b) const { return b == 0 ? s0 : s1; }
  template <int SELF>
  __device__ __forceinline__ void tile(const double4* tile) {
    const int t = threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const double4 r = tile[j];
      double g0 = r.w, g1 = r.w;
      if constexpr (SELF == 0) g0 = j == t ? 0.0 : r.w;
      if constexpr (SELF == 1) g1 = j == t ? 0.0 : r.w;
      tidal_pair(r.x, r.y, r.z, g0, x0, y0, z0, s0);
      tidal_pair(r.x, r.y, r.z, g1, x1, y1, z1, s1);
    }
  }
};

// The work of one workgroup: point column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), at the m points pts[0 .. m) ({x, y, z, anything} records; bodies
// mode: pts == posm and m == n).  Writes, for every point below m of the column, records 2 * (split * m + point) and the next.
template <typename T, bool BODIES>
__device__ __forceinline__ void tidal_body(const typename V4<T>::type* __restrict__ posm, const int n,
                                           const typename V4<T>::type* __restrict__ pts, const int m, const int tiles_per_split,
                                           typename V4<T>::type* __restrict__ parts, const int col, const int split) {
  using T4 = typename V4<T>::type;
  constexpr int B = kTidalPoints;
  static_assert(B == 2, "tile 2 * col + b holds the bodies of point b");
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first point of this workgroup
  const T4 zero = zero_record<T4>();
  TidalLane<T> lane;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < m) p = pts[li];
    lane.load(b, p);
  }
  lane.clear();
  TileWalk<T4> walk(posm, n, split, tiles_per_split);
  for (int k = walk.k0; k < walk.k1; ++k) {
    walk.stage(tile, k);
    if (BODIES && k == B * col) lane.template tile<0>(tile);
    else if (BODIES && k == B * col + 1) lane.template tile<1>(tile);
    else lane.template tile<-1>(tile);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < m) {
      const TidalSums<T> s = lane.sums(b);
      T4 o0, o1;
      o0.x = s.xx; o0.y = s.xy; o0.z = s.xz; o0.w = s.yy;
      o1.x = s.yz; o1.y = s.zz; o1.z = s.q; o1.w = (T)0;
      T4* row = parts + 2 * ((size_t)split * (size_t)m + (size_t)li);
      row[0] = o0;
      row[1] = o1;
    }
  }
}

template <typename T, bool BODIES>
__global__ __launch_bounds__(kBlock) void tidal_kernel(const typename V4<T>::type* __restrict__ posm, int n,
                                                       const typename V4<T>::type* __restrict__ pts, int m, int tiles_per_split,
                                                       typename V4<T>::type* __restrict__ parts) {
  tidal_body<T, BODIES>(posm, n, BODIES ? posm : pts, BODIES ? n : m, tiles_per_split, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread]; pts[count][m]; parts[count][gridDim.y][m][2]
// (bodies mode: m = n, pts unused).
template <typename T>
struct EnsembleTidalArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* pts;   // the points of member `first`
  typename V4<T>::type* parts;       // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  int n, m, tiles_per_split;
};

template <typename T, bool BODIES>
__global__ __launch_bounds__(kBlock) void ensemble_tidal_kernel(const EnsembleTidalArgs<T> e) {
  const size_t k = blockIdx.z;
  const typename V4<T>::type* posm = e.posm + (e.first + k) * e.pos_stride;
  const int m = BODIES ? e.n : e.m;
  tidal_body<T, BODIES>(posm, e.n, BODIES ? posm : e.pts + k * (size_t)m, m, e.tiles_per_split,
                                      e.parts + 2 * k * gridDim.y * (size_t)m, blockIdx.x, blockIdx.y);
}

struct TidalMember : OutMember {};

template <typename T>
struct RaggedTidalArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const TidalMember* table;          // [members]
  const typename V4<T>::type* pts;   // the points of member `first`
  typename V4<T>::type* parts;       // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  int m;                             // points per member (points mode)
};

template <typename T, bool BODIES>
__global__ __launch_bounds__(kBlock) void ragged_tidal_kernel(const RaggedTidalArgs<T> r) {
  const size_t k = blockIdx.z;
  const MemberGroup<TidalMember> g = member_group(r.table, r.first, BODIES ? 0 : r.m);
  if (g.elsewhere()) return;
  const int m = BODIES ? g.mem.n : r.m;
  const typename V4<T>::type* posm = r.posm + g.mem.pos_off;
  const size_t rel = BODIES ? g.rel() : k * (size_t)m;  // the points or bodies of the range before this member
  tidal_body<T, BODIES>(posm, g.mem.n, BODIES ? posm : r.pts + rel, m, g.shape.tiles_per_split, r.parts + 2 * rel * gridDim.y,
                                      blockIdx.x, blockIdx.y);
}

// Point or body idx of the call's `total`..  m > 0, points mode: member idx / m of the range, point idx % m; the member has n
// bodies from the table (a ragged ensemble) or n_all (table == nullptr)..  m == 0, bodies mode: the member found by member_at..  A
// system of `pts` points has field_shape(pts, n).splits rows of pts record pairs; its rows begin at (the points of the range
// before it) * row_splits pairs, row_splits the gridDim.y of the pair-work launch..  Writes records 2 * idx {xx, xy, xz, yy} and
// 2 * idx + 1 {yz, zz, 0, 0} of out.
template <typename T>
__global__ __launch_bounds__(kBlock) void tidal_finish_kernel(const typename V4<T>::type* __restrict__ parts,
                                                              const TidalMember* __restrict__ table, unsigned first, int count, int n_all,
                                                              int m, int row_splits, unsigned total,
                                                              typename V4<T>::type* __restrict__ out) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  int n = n_all, pts = m;
  size_t rel = 0;
  if (m > 0) {
    const unsigned k = idx / (unsigned)m;
    if (table) n = table[first + k].n;
    rel = (size_t)k * (size_t)m;
  } else {
    const MemberAt at = member_at(table, first, count, n_all, idx);
    n = pts = at.n;
    rel = at.rel;
  }
  const int splits = field_shape(pts, n).splits;
  const T4* row = parts + 2 * (rel * (size_t)row_splits + ((size_t)idx - rel));
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0, q = 0.0;
  for (int s = 0; s < splits; ++s) {
    const T4 a = row[2 * (size_t)s * (size_t)pts], b = row[2 * (size_t)s * (size_t)pts + 1];
    xx += (double)a.x; xy += (double)a.y; xz += (double)a.z; yy += (double)a.w;
    yz += (double)b.x; zz += (double)b.y; q += (double)b.z;
  }
  T4 o0, o1;
  o0.x = (T)__builtin_fma(3.0, xx, -q);
  o0.y = (T)(3.0 * xy);
  o0.z = (T)(3.0 * xz);
  o0.w = (T)__builtin_fma(3.0, yy, -q);
  o1.x = (T)(3.0 * yz);
  o1.y = (T)__builtin_fma(3.0, zz, -q);
  o1.z = o1.w = (T)0;
  out[2 * (size_t)idx] = o0;
  out[2 * (size_t)idx + 1] = o1;
}

}  // namespace nbx
