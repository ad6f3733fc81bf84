// nbx_field_kernels.hpp -- the kernels of nbx_field, nbx_ensemble_field and nbx_ragged_field (include/nbx_field.h): at each of
// m caller-supplied points p of a system of n bodies
//     a(p)   =   sum over j < n of G m_j (x_j - p) / (|x_j - p|^2 + eps^2)^(3/2)
//     phi(p) = - sum over j < n of G m_j / sqrt(|x_j - p|^2 + eps^2)
// Instantiated by nbx_field.hip alone.
//
//   field_kernel<T>            grid (columns, splits), block 256          a context (sliced or not: every position is resident)
//   ensemble_field_kernel<T>   grid (columns, splits, count), block 256   member first + blockIdx.z, its points at blockIdx.z * m
//   ragged_field_kernel<T>     grid (columns, largest splits of the range, count), block 256: the workgroup reads its member's
//                              {pos_off, n} from the table, evaluates field_shape(m, n) itself and returns at once where
//                              blockIdx.y is not one of its member's splits; no per-call work list
//     All three run field_body, the shape of ts_body (nbx_timescale_kernels.hpp) with the i side replaced: 256 threads,
//     kFieldPoints<T> = 2 points per lane, the j range of the workgroup's split in 256-record tiles staged in LDS (ONE array, the
//     position records, read whole), the next tile prefetched into registers.  Columns, splits and tiles per split are
//     field_shape's (nbx_field_shape.hpp), a function of (m, n) alone.
//   field_finish_kernel<T>     one thread per point of the call: adds the point's partial records in fp64 in split order, rounds
//                              once to T and writes {ax, ay, az, phi}; phi takes its minus sign here
//
// One pair, in T (fp32: the same operations on the lane's two points per packed instruction -- pair2's 12 packed VALU and
// 2 v_rsq_f32 plus ONE packed fma for phi):
//   dx,dy,dz = x_j - p;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))          the force kernels' r2
//   fp32:  inv = rsq(r2);  s = (gm*inv)*(inv*inv)        gm_inv_cube        a += d*s (fma);   phi += gm*inv (fma)
//   fp64:  y = v_rsq_f64(r2);  y2 = y*y;  h = fma(-r2, y2, 1)     the seed and its residual, shared by the cube and the inverse
//          s = ((gm*y)*y2) * fma(h, fma(h, 15, 12), 8)            gm_inv_cube, the same operations: 8 r2^(-3/2) gm
//          phi += (gm*y) * fma(h, fma(h, 3, 4), 8)    (fma)       8 gm y (1 + h/2 + 3/8 h^2) = 8 gm r2^(-1/2) (1 + O(h^3)), h^3 < 2^-70
// gm is the record's .w = G*m * gm_prescale<T>().  The fp64 prescale, 1/8, meets the 8 folded into both polynomials -- powers of
// two, so every rounding is the one the unscaled operation would make -- and the seed is used as it comes (rsq<double>()'s factor
// 2 is the Newton form's and does not arise): what leaves field_body carries no scale.
//
// Every body counts: a point is not a body, so nothing is masked.  A record at or beyond n -- the zero padding -- has gm = 0 and
// a finite r2 >= eps2: both of its terms are exact zeros.  A point on body i gets d = 0, hence a zero acceleration term, and the
// potential term G m_i / eps.
//
// Partials: parts[member of the range][split][point] records {ax, ay, az, sum gm*inv} of T, a member's rows together (stride
// gridDim.y * m records); a point's four accumulators are T, j ascending within the split.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");

// one pair of the scalar form (fp64, and fp32 where B is odd)
__device__ __forceinline__ void field_pair(float xj, float yj, float zj, float gmj, float xi, float yi, float zi, float& ax, float& ay,
                                           float& az, float& ph) {
  const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const float r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<float>())));
  const float inv = rsq(r2);
  const float inv2 = inv * inv;
  const float s = (gmj * inv) * inv2;
  ax = fmaT(dx, s, ax);
  ay = fmaT(dy, s, ay);
  az = fmaT(dz, s, az);
  ph = fmaT(gmj, inv, ph);
}
__device__ __forceinline__ void field_pair(double xj, double yj, double zj, double gmj, double xi, double yi, double zi, double& ax,
                                           double& ay, double& az, double& ph) {
  const double dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const double r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<double>())));
  const double y = __builtin_amdgcn_rsq(r2);
  const double y2 = y * y;
  const double h = __builtin_fma(-r2, y2, 1.0);
  const double gy = gmj * y;
  const double q = __builtin_fma(h, __builtin_fma(h, 15.0, 12.0), 8.0);  // 8 (1 + 3/2 h + 15/8 h^2): gm_inv_cube's
  const double p = __builtin_fma(h, __builtin_fma(h, 3.0, 4.0), 8.0);    // 8 (1 + 1/2 h +  3/8 h^2)
  const double s = (gy * y2) * q;
  ax = fmaT(dx, s, ax);
  ay = fmaT(dy, s, ay);
  az = fmaT(dz, s, az);
  ph = fmaT(gy, p, ph);
}

// two points per call on the packed-fp32 pipe: pair2 (nbx_pair.hpp) and one packed fma more
__device__ __forceinline__ void field_pair2(float xj, float yj, float zj, float gmj, f32x2 xi, f32x2 yi, f32x2 zi, f32x2& ax, f32x2& ay,
                                            f32x2& az, f32x2& ph) {
  const f32x2 dx = f32x2{xj, xj} - xi, dy = f32x2{yj, yj} - yi, dz = f32x2{zj, zj} - zi;
  const f32x2 e2 = {softening2<float>(), softening2<float>()};
  f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dx, dx, r2);
  f32x2 inv;
  inv.x = __builtin_amdgcn_rsqf(r2.x);
  inv.y = __builtin_amdgcn_rsqf(r2.y);
  const f32x2 inv2 = inv * inv;
  const f32x2 g = {gmj, gmj};
  const f32x2 s = (g * inv) * inv2;
  ax = __builtin_elementwise_fma(dx, s, ax);
  ay = __builtin_elementwise_fma(dy, s, ay);
  az = __builtin_elementwise_fma(dz, s, az);
  ph = __builtin_elementwise_fma(g, inv, ph);
}

// The work of one workgroup: point column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), at the m points pts[0 .. m) ({x, y, z, 0} records).  Writes, for
// every point below m of the column, record split * m + point of parts.
template <typename T, int B>
__device__ __forceinline__ void field_body(const typename V4<T>::type* __restrict__ posm, const int n,
                                           const typename V4<T>::type* __restrict__ pts, const int m, const int tiles_per_split,
                                           typename V4<T>::type* __restrict__ parts, const int col, const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first point of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[B], yi[B], zi[B], ax[B], ay[B], az[B], ph[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < m) p = pts[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ax[b] = ay[b] = az[b] = ph[b] = (T)0;
  }
  TileWalk<T4> walk(posm, n, split, tiles_per_split);
  for (int k = walk.k0; k < walk.k1; ++k) {
    walk.stage(tile, k);
    if constexpr (sizeof(T) == 4 && B % 2 == 0) {
      f32x2 px[B / 2], py[B / 2], pz[B / 2], qx[B / 2], qy[B / 2], qz[B / 2], qp[B / 2];
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
        py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
        pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
        qx[h] = f32x2{ax[2 * h], ax[2 * h + 1]};
        qy[h] = f32x2{ay[2 * h], ay[2 * h + 1]};
        qz[h] = f32x2{az[2 * h], az[2 * h + 1]};
        qp[h] = f32x2{ph[2 * h], ph[2 * h + 1]};
      }
#pragma unroll 4
      for (int j = 0; j < kTile; ++j) {
        const float4 r = tile[j];
#pragma unroll
        for (int h = 0; h < B / 2; ++h) field_pair2(r.x, r.y, r.z, r.w, px[h], py[h], pz[h], qx[h], qy[h], qz[h], qp[h]);
      }
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        ax[2 * h] = qx[h].x; ax[2 * h + 1] = qx[h].y;
        ay[2 * h] = qy[h].x; ay[2 * h + 1] = qy[h].y;
        az[2 * h] = qz[h].x; az[2 * h + 1] = qz[h].y;
        ph[2 * h] = qp[h].x; ph[2 * h + 1] = qp[h].y;
      }
    } else {
#pragma unroll 4
      for (int j = 0; j < kTile; ++j) {
        const T4 r = tile[j];
#pragma unroll
        for (int b = 0; b < B; ++b) field_pair(r.x, r.y, r.z, r.w, xi[b], yi[b], zi[b], ax[b], ay[b], az[b], ph[b]);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < m) {
      T4 o;
      o.x = ax[b]; o.y = ay[b]; o.z = az[b]; o.w = ph[b];
      parts[(size_t)split * (size_t)m + (size_t)li] = o;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void field_kernel(const typename V4<T>::type* __restrict__ posm, int n,
                                                       const typename V4<T>::type* __restrict__ pts, int m, int tiles_per_split,
                                                       typename V4<T>::type* __restrict__ parts) {
  field_body<T, kFieldPoints<T>>(posm, n, pts, m, tiles_per_split, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread]; pts[count][m]; parts[count][gridDim.y][m].
template <typename T>
struct EnsembleFieldArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* pts;   // the points of member `first`
  typename V4<T>::type* parts;       // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  int n, m, tiles_per_split;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ensemble_field_kernel(const EnsembleFieldArgs<T> e) {
  const size_t k = blockIdx.z;
  field_body<T, kFieldPoints<T>>(e.posm + (e.first + k) * e.pos_stride, e.n, e.pts + k * (size_t)e.m, e.m, e.tiles_per_split,
                                 e.parts + k * gridDim.y * (size_t)e.m, blockIdx.x, blockIdx.y);
}

struct FieldMember : PosMember {};

template <typename T>
struct RaggedFieldArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const FieldMember* table;          // [members]
  const typename V4<T>::type* pts;   // the points of member `first`
  typename V4<T>::type* parts;       // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  int m;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void ragged_field_kernel(const RaggedFieldArgs<T> r) {
  const size_t k = blockIdx.z;
  const MemberGroup<FieldMember> g = member_group(r.table, r.first, r.m);
  if ((int)blockIdx.y >= g.shape.splits) return;  // the whole workgroup: this split is another, larger member's
  field_body<T, kFieldPoints<T>>(r.posm + g.mem.pos_off, g.mem.n, r.pts + k * (size_t)r.m, r.m, g.shape.tiles_per_split,
                                 r.parts + k * gridDim.y * (size_t)r.m, blockIdx.x, blockIdx.y);
}

// Point idx of the call's `total` = count * m points: member idx / m of the range, point idx % m.  The member has
// field_shape(m, n).splits rows, n from the table (a ragged ensemble) or n_all (table == nullptr); its rows begin at
// member * row_splits * m, row_splits the gridDim.y of the pair-work launch.
template <typename T>
__global__ __launch_bounds__(kBlock) void field_finish_kernel(const typename V4<T>::type* __restrict__ parts,
                                                              const FieldMember* __restrict__ table, unsigned first, int n_all, int m,
                                                              int row_splits, unsigned total, typename V4<T>::type* __restrict__ out) {
  using T4 = typename V4<T>::type;
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const unsigned k = idx / (unsigned)m, p = idx - k * (unsigned)m;
  const int n = table ? table[first + k].n : n_all;
  const int splits = field_shape(m, n).splits;
  const T4* row = parts + (size_t)k * (size_t)row_splits * (size_t)m + p;
  double ax = 0.0, ay = 0.0, az = 0.0, ph = 0.0;
  for (int s = 0; s < splits; ++s) {
    const T4 v = row[(size_t)s * (size_t)m];
    ax += (double)v.x;
    ay += (double)v.y;
    az += (double)v.z;
    ph += (double)v.w;
  }
  T4 o;
  o.x = (T)ax; o.y = (T)ay; o.z = (T)az; o.w = (T)(-ph);
  out[idx] = o;
}

}  // namespace nbx
