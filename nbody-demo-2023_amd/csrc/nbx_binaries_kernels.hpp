// nbx_binaries_kernels.hpp -- the kernels of nbx_binaries, nbx_ensemble_binaries and nbx_ragged_binaries
// (include/nbx_binaries.h): for every body i of a system of n bodies the partner j < n, j != i with the smallest specific
// two-body energy
//     e(i, j) = |v_j - v_i|^2 / 2 - G (m_i + m_j) / sqrt(|x_j - x_i|^2 + eps^2)
// (the lowest j among equal bit patterns), that e, and the number of partners with e(i, j) < 0.  Instantiated by
// nbx_binaries.hip alone.
//
//   bound_kernel<T, COUNT>            grid (columns, splits), block 256          a context that owns all n bodies
//   ensemble_bound_kernel<T, COUNT>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_bound_kernel<T, COUNT>     grid (largest columns, largest splits of the range, count), block 256: the workgroup reads
//                                     its member's {pos_off, vel_off, out_off, n} from the table, evaluates field_shape(n, n)
//                                     itself and returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three run bound_body: 256 threads, two bodies per lane (the i side: the column's own position and velocity records),
//     the j range of the workgroup's split in 256-record tiles staged in LDS -- TWO arrays per tile, the position records and
//     the velocity records of the same j (a velocity is loaded only where j < n: what lies behind a system's last velocity is
//     never read) -- the next tile prefetched into registers.  Columns, splits and tiles per split are field_shape(n, n)
//     (nbx_field_shape.hpp): a performance choice only, nothing below depends on it.  COUNT: the bound count is asked for; the
//     other form does not compile its compare and add.
//   bound_finish_kernel<T>            one thread per body of the call: walks the body's split records in ascending order, takes
//                                     a split's candidate only on strict <, adds the counts, undoes the scale, writes
//                                     {e, j, count}
//
// One pair, in T (bound_pair; the fp32 tile loop is the same operations on the lane's two bodies per packed instruction: per j
// record 6 packed subtracts, 5 packed fma and 1 packed multiply for r2 and w, 1 packed add for s, 2 v_rsq_f32, 1 packed fma):
//   dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))           the force kernels' r2
//   ux,uy,uz = v_j - v_i;  w  = fma(ux,ux, fma(uy,uy, uz*uz))
//   s = gm_i + gm_j;  inv = rsq(r2);  e2 = fma(-s, inv, w)
//   if (e2 < best) { best = e2; index = j; }         j ascends within a split and the compare is strict: the lowest j wins
//   count += e2 < 0
// e2 is TWICE the header's e = fma(-s, inv, w/2), exactly: both gm enter scaled by bound_gm_scale<T>() -- a power of two, so the
// sum, the product inside the fma and the fma's one rounding are those of the unscaled operands -- which is 2 in fp32 and, since
// the fp64 records carry G*m/8 and rsq<double>() is 2/sqrt, 2 * 8 / 2 = 8 in fp64.  The i side is scaled once per body, the j
// side once per record when its tile is staged; the minimum and the sign do not see a positive scale, and the finish kernel
// halves the winner.  Every multiply or add that is not part of a written fma goes through mul_rn / add_rn, so no build
// contracts one.  j is uniform over the wave, so the index operand of the select is a scalar.
//
// The mask: a pair is dropped EXACTLY where j == i or j >= n -- it is neither a candidate nor counted.  A padding record has a
// position (the origin) and a zero velocity: against a body at rest near the origin it would be an unbound partner of energy
// about 0 and the minimum of a body that is bound to nobody.  Only tiles that meet the workgroup's own bodies or reach past n
// run the masked loop; every other tile runs the loop without the mask compares (bound_tile<..., MASK>).
//
// A minimum with a lowest-index tie-break and an integer sum do not depend on the order they are taken in: the three values are
// the same bits for every launch shape, and a member's are a lone context's.  parts[member of the range][split][body] records
// {e2, j, count}, a member's rows together; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kBoundBodies = 2;                         // bodies per lane (fp32: one packed pair)
constexpr long long kBoundMaxBodies = kFieldMaxPoints;  // per call (include/nbx_binaries.h, status 3)

// what a (split, body) leaves behind (e: the doubled energy), and what the finish kernel writes per body (e: the energy):
// j == -1, e == +inf, count == 0 where the body met no partner
template <typename T>
struct BoundRecord {
  T e;
  int j;
  int count;
};

template <typename T> __device__ __forceinline__ T bound_inf() { return (T)__builtin_huge_valf(); }

// what a record's .w is multiplied by so that fma(-(gm_i + gm_j), rsq(r2), w) is twice the energy: 2 / (gm_prescale * the
// numerator of rsq) -- 2 and 8, powers of two
template <typename T> __host__ __device__ constexpr T bound_gm_scale() { return sizeof(T) == 8 ? (T)8 : (T)2; }

// The pair arithmetic of include/nbx_binaries.h for one pair, in T: twice e(i, j).  gmi, gmj: the records' .w times
// bound_gm_scale<T>().
template <typename T>
__device__ __forceinline__ T bound_pair(T xj, T yj, T zj, T gmj, T uj, T vj, T wj, T xi, T yi, T zi, T gmi, T ui, T vi, T wi) {
  const T dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
  const T ux = uj - ui, uy = vj - vi, uz = wj - wi;
  const T w = fmaT(ux, ux, fmaT(uy, uy, mul_rn(uz, uz)));
  const T s = add_rn(gmi, gmj);
  const T inv = rsq(r2);
  return fmaT(-s, inv, w);
}

// one pair against the running minimum, its index and the count.  MASK: the pair may be the body itself or a record at or
// beyond n (jg: the record's index, uniform over the wave).
template <typename T, bool MASK, bool COUNT>
__device__ __forceinline__ void bound_take(const T e, const int jg, const int n, const int ig, T& best, int& bj, int& cnt) {
  bool lt = e < best;
  bool neg = e < (T)0;
  if constexpr (MASK) {
    const bool ok = jg < n && jg != ig;
    lt = lt && ok;
    neg = neg && ok;
  }
  best = lt ? e : best;
  bj = lt ? jg : bj;
  if constexpr (COUNT) cnt += neg ? 1 : 0;
}

// One LDS tile against the lane's B bodies (j_glob: global index of tile record 0).
template <typename T, int B, bool MASK, bool COUNT>
__device__ __forceinline__ void bound_tile(const typename V4<T>::type* ptile, const typename V4<T>::type* vtile, const int j_glob,
                                           const int n, const T (&xi)[B], const T (&yi)[B], const T (&zi)[B], const T (&gi)[B],
                                           const T (&ui)[B], const T (&vi)[B], const T (&wi)[B], const int (&ig)[B], T (&best)[B],
                                           int (&bj)[B], int (&cnt)[B]) {
  if constexpr (sizeof(T) == 4 && B % 2 == 0) {
    f32x2 px[B / 2], py[B / 2], pz[B / 2], pg[B / 2], pu[B / 2], pv[B / 2], pw[B / 2];
#pragma unroll
    for (int h = 0; h < B / 2; ++h) {
      px[h] = f32x2{xi[2 * h], xi[2 * h + 1]};
      py[h] = f32x2{yi[2 * h], yi[2 * h + 1]};
      pz[h] = f32x2{zi[2 * h], zi[2 * h + 1]};
      pg[h] = f32x2{gi[2 * h], gi[2 * h + 1]};
      pu[h] = f32x2{ui[2 * h], ui[2 * h + 1]};
      pv[h] = f32x2{vi[2 * h], vi[2 * h + 1]};
      pw[h] = f32x2{wi[2 * h], wi[2 * h + 1]};
    }
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const float4 r = ptile[j];
      const float4 s = whole_record(vtile, j);
      const int jg = j_glob + j;
#pragma unroll
      for (int h = 0; h < B / 2; ++h) {
        const f32x2 dx = f32x2{r.x, r.x} - px[h], dy = f32x2{r.y, r.y} - py[h], dz = f32x2{r.z, r.z} - pz[h];
        f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
        r2 = __builtin_elementwise_fma(dy, dy, r2);
        r2 = __builtin_elementwise_fma(dx, dx, r2);
        const f32x2 ux = f32x2{s.x, s.x} - pu[h], uy = f32x2{s.y, s.y} - pv[h], uz = f32x2{s.z, s.z} - pw[h];
        f32x2 w = mul_rn(uz, uz);
        w = __builtin_elementwise_fma(uy, uy, w);
        w = __builtin_elementwise_fma(ux, ux, w);
        const f32x2 sg = add_rn(pg[h], f32x2{r.w, r.w});
        f32x2 inv;
        inv.x = __builtin_amdgcn_rsqf(r2.x);
        inv.y = __builtin_amdgcn_rsqf(r2.y);
        const f32x2 e = __builtin_elementwise_fma(-sg, inv, w);
        bound_take<float, MASK, COUNT>(e.x, jg, n, ig[2 * h], best[2 * h], bj[2 * h], cnt[2 * h]);
        bound_take<float, MASK, COUNT>(e.y, jg, n, ig[2 * h + 1], best[2 * h + 1], bj[2 * h + 1], cnt[2 * h + 1]);
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = ptile[j];
      const typename V4<T>::type s = vtile[j];
      const int jg = j_glob + j;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const T e = bound_pair<T>(r.x, r.y, r.z, r.w, s.x, s.y, s.z, xi[b], yi[b], zi[b], gi[b], ui[b], vi[b], wi[b]);
        bound_take<T, MASK, COUNT>(e, jg, n, ig[b], best[b], bj[b], cnt[b]);
      }
    }
  }
}

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding) and whose velocity records velm[0 .. n) are read.  Writes, for
// every body below n of the column, record split * n + body of parts.
template <typename T, int B, bool COUNT>
__device__ __forceinline__ void bound_body(const typename V4<T>::type* __restrict__ posm, const typename V4<T>::type* __restrict__ velm,
                                           const int n, const int tiles_per_split, BoundRecord<T>* __restrict__ parts, const int col,
                                           const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 ptile[kTile];
  __shared__ T4 vtile[kTile];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * B);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[B], yi[B], zi[B], gi[B], ui[B], vi[B], wi[B], best[B];
  int ig[B], bj[B], cnt[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero, v = zero;
    if (li < n) {
      p = posm[li];
      v = velm[li];
    }
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    gi[b] = mul_rn(p.w, bound_gm_scale<T>());
    ui[b] = v.x; vi[b] = v.y; wi[b] = v.z;
    ig[b] = li;
    best[b] = bound_inf<T>();
    bj[b] = -1;
    cnt[b] = 0;
  }
  const int g_lo = l0, g_hi = min(l0 + kBlock * B, n);  // the workgroup's bodies: a tile that meets them runs the masked loop
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  T4 next_p = zero, next_v = zero;
  if (k0 < k1) {
    const int j = k0 * kTile + t;
    next_p = posm[j];
    if (j < n) next_v = velm[j];
  }
  for (int k = k0; k < k1; ++k) {
    __syncthreads();  // every lane is done with the previous tile
    next_p.w = mul_rn(next_p.w, bound_gm_scale<T>());
    ptile[t] = next_p;
    vtile[t] = next_v;
    __syncthreads();
    if (k + 1 < k1) {
      const int j = (k + 1) * kTile + t;
      next_p = posm[j];
      next_v = zero;
      if (j < n) next_v = velm[j];
    }
    const int j0 = k * kTile;
    if (tile_masked(j0, g_lo, g_hi, n))
      bound_tile<T, B, true, COUNT>(ptile, vtile, j0, n, xi, yi, zi, gi, ui, vi, wi, ig, best, bj, cnt);
    else
      bound_tile<T, B, false, COUNT>(ptile, vtile, j0, n, xi, yi, zi, gi, ui, vi, wi, ig, best, bj, cnt);
  }
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int li = l0 + b * kBlock + t;
    if (li < n) {
      BoundRecord<T> o;
      o.e = best[b]; o.j = bj[b]; o.count = cnt[b];
      parts[(size_t)split * (size_t)n + (size_t)li] = o;
    }
  }
}

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlock) void bound_kernel(const typename V4<T>::type* __restrict__ posm,
                                                       const typename V4<T>::type* __restrict__ velm, int n, int tiles_per_split,
                                                       BoundRecord<T>* __restrict__ parts) {
  bound_body<T, kBoundBodies, COUNT>(posm, velm, n, tiles_per_split, parts, blockIdx.x, blockIdx.y);
}

// Layout, member-major as the ensemble's step kernels have it: posm[S][n_alloc + kSgprOverread], velm[S][own_pad];
// parts[count][gridDim.y][n].
template <typename T>
struct EnsembleBoundArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  const typename V4<T>::type* velm;  // member 0's velocities
  BoundRecord<T>* parts;             // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
  unsigned pos_stride;               // records between members in posm
  unsigned vel_stride;               // records between members in velm
  int n, tiles_per_split;
};

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlock) void ensemble_bound_kernel(const EnsembleBoundArgs<T> e) {
  const size_t k = blockIdx.z;
  bound_body<T, kBoundBodies, COUNT>(e.posm + (e.first + k) * e.pos_stride, e.velm + (e.first + k) * e.vel_stride, e.n, e.tiles_per_split,
                                     e.parts + k * gridDim.y * (size_t)e.n, blockIdx.x, blockIdx.y);
}

struct BoundMember : VelMember {};

template <typename T>
struct RaggedBoundArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const typename V4<T>::type* velm;  // the velocities of all members
  const BoundMember* table;          // [members]
  BoundRecord<T>* parts;             // the partial rows of member `first`
  unsigned first;                    // member of blockIdx.z == 0
};

template <typename T, bool COUNT>
__global__ __launch_bounds__(kBlock) void ragged_bound_kernel(const RaggedBoundArgs<T> r) {
  const MemberGroup<BoundMember> g = member_group(r.table, r.first);
  if (g.elsewhere()) return;
  bound_body<T, kBoundBodies, COUNT>(r.posm + g.mem.pos_off, r.velm + g.mem.vel_off, g.mem.n, g.shape.tiles_per_split,
                                     r.parts + g.rel() * gridDim.y, blockIdx.x, blockIdx.y);
}

// Body idx of the call's `total` bodies, its member found by member_at..  The member has field_shape(n, n).splits rows of n
// records; its rows begin at (the bodies of the range before it) * row_splits, row_splits the gridDim.y of the pair-work
// launch..  The winner's doubled energy is halved: exact, +inf stays +inf.
template <typename T>
__global__ __launch_bounds__(kBlock) void bound_finish_kernel(const BoundRecord<T>* __restrict__ parts, const BoundMember* __restrict__ table,
                                                              unsigned first, int count, int n_all, int row_splits, unsigned total,
                                                              BoundRecord<T>* __restrict__ out) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const MemberAt at = member_at(table, first, count, n_all, idx);
  const int n = at.n;
  const size_t rel = at.rel;  // the bodies of the range before the body's member
  const int splits = field_shape(n, n).splits;
  const BoundRecord<T>* row = parts + rel * (size_t)row_splits + ((size_t)idx - rel);
  BoundRecord<T> o;
  o.e = bound_inf<T>(); o.j = -1; o.count = 0;
  for (int s = 0; s < splits; ++s) {
    const BoundRecord<T> v = row[(size_t)s * (size_t)n];
    if (v.e < o.e) { o.e = v.e; o.j = v.j; }
    o.count += v.count;
  }
  o.e = mul_rn(o.e, (T)0.5);
  out[idx] = o;
}

}  // namespace nbx
