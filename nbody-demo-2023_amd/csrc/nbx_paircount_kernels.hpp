// nbx_paircount_kernels.hpp -- the kernels of nbx_paircount, nbx_ensemble_paircount and nbx_ragged_paircount
// (include/nbx_paircount.h): for a system of n bodies and E radii per pass the number of ORDERED pairs (i, j), j < n, j != i, with
//     r2(i, j) = |x_j - x_i|^2 + eps^2 <= h2[k]
// per workgroup; the finish adds a member's workgroups and halves.  Instantiated by nbx_paircount.hip alone.
//
//   paircount_kernel<T, E, WAVE>            grid (columns, splits), block 256          a context (sliced or not)
//   ensemble_paircount_kernel<T, E, WAVE>   grid (columns, splits, count), block 256   member first + blockIdx.z
//   ragged_paircount_kernel<T, E, WAVE>     grid (largest columns, largest splits of the range, count), block 256: the workgroup
//                                           reads its member's {pos_off, n} from the table, evaluates field_shape(n, n) itself and
//                                           returns at once where blockIdx.x or blockIdx.y is not one of its member's
//     All three run pc_body, which is nb_body's structure (nbx_neighbours_kernels.hpp): 256 threads, two bodies per lane on the
//     i side, the j range of the workgroup's split in 256-record LDS tiles read as whole 16-byte records, the next tile prefetched
//     into registers, a masked and an unmasked tile loop chosen per tile.  Columns, splits and tiles per split are
//     field_shape(n, n): a performance choice only.  E in {4, 8, 16}: the radii of one pass, uniform kernel arguments (scalar
//     operands of the compares); a slot the call does not use carries h2 = -1 and never counts, because r2 >= eps2 > 0.
//   paircount_finish_kernel                 one thread per (member, radius): adds the member's splits x columns records in uint64,
//                                           splits outer, columns inner, both ascending, and shifts right by one
//
// One pair, in T: the neighbours kernels' r2 -- dx,dy,dz = x_j - x_i; r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2))) -- in fp32
// for the lane's two bodies in 3 packed subtracts and 3 packed fma; then per radius one compare against a scalar operand and
// one of two counting schemes (pc_take, WAVE):
//   lane counters (WAVE = false)   cnt[k] += r2 <= h2[k]: a compare and an add-with-carry, 2 VALU; E VGPRs, the lane's two bodies
//                                  share a counter; the lanes are added once, at the end of the workgroup
//   wave counters (WAVE = true)    cnt[k] += popcount(ballot(r2 <= h2[k])): a compare, a scalar bit count and a scalar add,
//                                  1 VALU + 2 SALU; the counters are wave-uniform
// Both are integer sums of the same predicate: the same bits.
//
// The mask: a pair is dropped EXACTLY where j == i, j >= n or i >= n, by a mask on the compare RESULT (with h2 = +inf nothing done
// to the operand would keep such a pair out).  Tiles that meet the workgroup's own bodies or reach past n run the masked loop, and
// so does every tile of a column that reaches past n (its last lanes hold no body); every other tile runs the loop without the
// mask.
//
// Counter widths: a workgroup has 512 bodies and a split at most 2^22 partners (kNbMaxBodies), so a workgroup's count stays below
// 2^31 and every partial fits uint32; the finish adds in uint64.  parts[member of the range][pass][split][column][kPcSlots]
// uint32, written by one thread per workgroup with ordinary stores; no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"
#include "nbx_tilewalk.hpp"

namespace nbx {

static_assert(kFieldBlock == kBlock && kFieldTile == kTile && kTile == kBlock, "field_shape counts in the kernels' own tiles");
static_assert(kFieldColumn == kBlock * 2, "a workgroup column is two bodies per lane");

constexpr int kPcBodies = 2;                        // bodies per lane (fp32: one packed pair)
constexpr int kPcSlots = 16;                        // radii per pass at most, and the uint32 per workgroup record
constexpr int kPcMaxRadii = 256;                    // per call (include/nbx_paircount.h, NBX_PAIRCOUNT_MAX_RADII)
constexpr long long kPcMaxBodies = kFieldMaxPoints;  // per call (include/nbx_paircount.h, status 5)
static_assert((long long)kBlock * kPcBodies * kPcMaxBodies <= (1ll << 31), "a workgroup's count fits uint32");

// the radii of one pass: h2[k] = fma(rT, rT, eps2), or -1 in a slot the call does not use
template <typename T, int E>
struct PcRadii {
  T h2[E];
};

// records per unrolled step of the tile loops: about 32 compares per step whatever E
template <int E> constexpr int kPcUnroll = E >= 16 ? 1 : (E >= 8 ? 2 : 4);

// one pair against the E radii.  MASK: the pair may be the body itself, a record at or beyond n or the row of a lane without a
// body (ok: it is none of these).
template <typename T, int E, bool MASK, bool WAVE>
__device__ __forceinline__ void pc_take(const T r2, const bool ok, const PcRadii<T, E>& h, unsigned (&cnt)[E]) {
  if constexpr (WAVE) {
    unsigned long long okb = 0;
    if constexpr (MASK) okb = __ballot(ok);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      unsigned long long b = __ballot(r2 <= h.h2[k]);
      if constexpr (MASK) b &= okb;
      cnt[k] += (unsigned)__builtin_popcountll(b);
    }
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      bool in = r2 <= h.h2[k];
      if constexpr (MASK) in = in && ok;
      cnt[k] += in ? 1u : 0u;
    }
  }
}

// One LDS tile against the lane's two bodies (j_glob: global index of tile record 0).
template <typename T, int E, bool MASK, bool WAVE>
__device__ __forceinline__ void pc_tile(const typename V4<T>::type* tile, const int j_glob, const int n, const T (&xi)[kPcBodies],
                                        const T (&yi)[kPcBodies], const T (&zi)[kPcBodies], const int (&ig)[kPcBodies],
                                        const PcRadii<T, E>& h, unsigned (&cnt)[E]) {
  if constexpr (sizeof(T) == 4) {
    const f32x2 px = {xi[0], xi[1]}, py = {yi[0], yi[1]}, pz = {zi[0], zi[1]};
    const f32x2 e2 = {softening2<float>(), softening2<float>()};
#pragma unroll kPcUnroll<E>
    for (int j = 0; j < kTile; ++j) {
      const float4 r = whole_record(tile, j);
      const int jg = j_glob + j;
      const f32x2 dx = f32x2{r.x, r.x} - px, dy = f32x2{r.y, r.y} - py, dz = f32x2{r.z, r.z} - pz;
      f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
      r2 = __builtin_elementwise_fma(dy, dy, r2);
      r2 = __builtin_elementwise_fma(dx, dx, r2);
      pc_take<float, E, MASK, WAVE>(r2.x, jg < n && jg != ig[0] && ig[0] < n, h, cnt);
      pc_take<float, E, MASK, WAVE>(r2.y, jg < n && jg != ig[1] && ig[1] < n, h, cnt);
    }
  } else {
#pragma unroll kPcUnroll<E>
    for (int j = 0; j < kTile; ++j) {
      const typename V4<T>::type r = tile[j];
      const int jg = j_glob + j;
#pragma unroll
      for (int b = 0; b < kPcBodies; ++b) {
        const T dx = r.x - xi[b], dy = r.y - yi[b], dz = r.z - zi[b];
        const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
        pc_take<T, E, MASK, WAVE>(r2, jg < n && jg != ig[b] && ig[b] < n, h, cnt);
      }
    }
  }
}

// The work of one workgroup: body column `col`, j split `split`, of a system of n bodies whose position records
// posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding).  Thread 0 writes the workgroup's E counts to out[0 .. E).
template <typename T, int E, bool WAVE>
__device__ __forceinline__ void pc_body(const typename V4<T>::type* __restrict__ posm, const int n, const int tiles_per_split,
                                        const PcRadii<T, E>& h, unsigned* __restrict__ out, const int col, const int split) {
  using T4 = typename V4<T>::type;
  __shared__ T4 tile[kTile];
  __shared__ unsigned red[kBlock / 64][E];
  const int t = threadIdx.x;
  const int l0 = col * (kBlock * kPcBodies);  // first body of this workgroup
  const T4 zero = zero_record<T4>();
  T xi[kPcBodies], yi[kPcBodies], zi[kPcBodies];
  int ig[kPcBodies];
  unsigned cnt[E];
#pragma unroll
  for (int b = 0; b < kPcBodies; ++b) {
    const int li = l0 + b * kBlock + t;
    T4 p = zero;
    if (li < n) p = posm[li];
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ig[b] = li;
  }
#pragma unroll
  for (int k = 0; k < E; ++k) cnt[k] = 0u;
  const int g_lo = l0, g_hi = min(l0 + kBlock * kPcBodies, n);  // the workgroup's bodies: a tile that meets them runs the masked loop
  const bool short_column = l0 + kBlock * kPcBodies > n;        // some lanes hold no body: every tile runs the masked loop
  const int tiles = (n + kTile - 1) / kTile;
  const int k0 = split * tiles_per_split, k1 = min(tiles, k0 + tiles_per_split);
  T4 next = zero;
  if (k0 < k1) next = posm[k0 * kTile + t];
  for (int k = k0; k < k1; ++k) {
    __syncthreads();  // every lane is done with the previous tile
    tile[t] = next;
    __syncthreads();
    if (k + 1 < k1) next = posm[(k + 1) * kTile + t];
    const int j0 = k * kTile;
    if (short_column || (j0 < g_hi && j0 + kTile > g_lo) || j0 + kTile > n)
      pc_tile<T, E, true, WAVE>(tile, j0, n, xi, yi, zi, ig, h, cnt);
    else
      pc_tile<T, E, false, WAVE>(tile, j0, n, xi, yi, zi, ig, h, cnt);
  }
  // once per workgroup: the lanes of a wave (lane counters; wave counters are uniform already), then the four waves through LDS
  if constexpr (!WAVE) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cnt[k] += __shfl_down(cnt[k], off, 64);
    }
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < E; ++k) red[t >> 6][k] = cnt[k];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < E; ++k) out[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// the record of workgroup (x, y) of member z of the launch: parts[z][pass][y][x][kPcSlots], `parts` the member 0 record of this
// pass and member_stride the uint32 between members (passes * gridDim.y * gridDim.x * kPcSlots)
__device__ __forceinline__ unsigned* pc_out(unsigned* parts, const size_t member_stride) {
  return parts + blockIdx.z * member_stride + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kPcSlots;
}

template <typename T, int E, bool WAVE>
__global__ __launch_bounds__(kBlock) void paircount_kernel(const typename V4<T>::type* __restrict__ posm, int n, int tiles_per_split,
                                                           const PcRadii<T, E> h, unsigned* __restrict__ parts) {
  pc_body<T, E, WAVE>(posm, n, tiles_per_split, h, pc_out(parts, 0), blockIdx.x, blockIdx.y);
}

// Layout, member-major as nbx_ensemble_kernels.hpp: posm[S][n_alloc + kSgprOverread].
template <typename T, int E>
struct EnsemblePcArgs {
  const typename V4<T>::type* posm;  // member 0's current records
  unsigned* parts;                   // this pass's records of member `first`
  unsigned long long member_stride;  // uint32 between members in parts
  PcRadii<T, E> h;
  unsigned first;       // member of blockIdx.z == 0
  unsigned pos_stride;  // records between members in posm
  int n, tiles_per_split;
};

template <typename T, int E, bool WAVE>
__global__ __launch_bounds__(kBlock) void ensemble_paircount_kernel(const EnsemblePcArgs<T, E> e) {
  pc_body<T, E, WAVE>(e.posm + (size_t)(e.first + blockIdx.z) * e.pos_stride, e.n, e.tiles_per_split, e.h,
                      pc_out(e.parts, (size_t)e.member_stride), blockIdx.x, blockIdx.y);
}

struct PcMember : PosMember {};

template <typename T, int E>
struct RaggedPcArgs {
  const typename V4<T>::type* posm;  // the current records of all members
  const PcMember* table;             // [members]
  unsigned* parts;                   // this pass's records of member `first`
  unsigned long long member_stride;  // uint32 between members in parts
  PcRadii<T, E> h;
  unsigned first;  // member of blockIdx.z == 0
};

template <typename T, int E, bool WAVE>
__global__ __launch_bounds__(kBlock) void ragged_paircount_kernel(const RaggedPcArgs<T, E> r) {
  const PcMember mem = r.table[r.first + blockIdx.z];
  const FieldShape s = field_shape(mem.n, mem.n);
  if ((int)blockIdx.x >= s.columns || (int)blockIdx.y >= s.splits) return;  // the whole workgroup: another, larger member's
  pc_body<T, E, WAVE>(r.posm + mem.pos_off, mem.n, s.tiles_per_split, r.h, pc_out(r.parts, (size_t)r.member_stride), blockIdx.x, blockIdx.y);
}

// Element idx = member * nradii + k of the call's count * nradii.  table == nullptr: every system has n_all bodies.  Reads the
// records of the member's own field_shape(n, n).splits x columns workgroups -- the only ones written -- in slot k % kPcSlots of
// pass k / kPcSlots; row_splits and row_columns are the gridDim.y and gridDim.x of the pair-work launches.
__global__ __launch_bounds__(kBlock) void paircount_finish_kernel(const unsigned* __restrict__ parts, const PcMember* __restrict__ table,
                                                                  unsigned first, int nradii, int n_all, int passes, int row_splits,
                                                                  int row_columns, unsigned total, unsigned long long* __restrict__ out) {
  const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (idx >= total) return;
  const unsigned m = idx / (unsigned)nradii, k = idx % (unsigned)nradii;
  const int n = table ? table[first + m].n : n_all;
  const FieldShape s = field_shape(n, n);
  const unsigned* rec = parts + ((size_t)m * (size_t)passes + k / kPcSlots) * (size_t)row_splits * (size_t)row_columns * kPcSlots + k % kPcSlots;
  unsigned long long sum = 0;
  for (int y = 0; y < s.splits; ++y)
    for (int x = 0; x < s.columns; ++x) sum += rec[((size_t)y * (size_t)row_columns + (size_t)x) * kPcSlots];
  out[idx] = sum >> 1;  // every unordered pair was met twice, with the same r2 bits
}

}  // namespace nbx
