// nbx_tilewalk.hpp -- the device code that the kernel headers which launch by field_shape (nbx_field_shape.hpp) share: the
// whole-record LDS read, the member entries of a ragged ensemble's tables, the member of a workgroup and of a finished element,
// the rule for which tiles run a masked loop, and the double-buffered walk over the j tiles of a split.  The device-side sibling
// of nbx_analysis.hpp: inline device code only, no kernel, and no call is named -- a unit hands in its own arrays and its own
// per-tile work.
#pragma once
#include "nbx_field_shape.hpp"
#include "nbx_pair.hpp"

namespace nbx {

template <typename T4>
__device__ __forceinline__ T4 zero_record() {
  T4 z;
  z.x = z.y = z.z = z.w = 0;
  return z;
}

// A tile record, read whole.  Where a pair needs three of the record's components alone, the compiler left to itself narrows
// the fp32 read to 12 bytes (ds_read_b96), which occupies the LDS twice as long as the 16-byte read (ds_read_b128): the empty
// statement keeps .w alive and costs no instruction.
__device__ __forceinline__ float4 whole_record(const float4* tile, const int j) {
  const float4 r = tile[j];
  asm volatile("" ::"v"(r.w));
  return r;
}

// One entry per member of a ragged ensemble, built on first use and fixed for the object's life (kernel-argument data: the
// host's ragged_member_table makers fill them).  Three layouts: what a unit reads decides which it takes.
struct PosMember {
  unsigned long long pos_off;  // the member's first record in posm
  int n;
  int reserved;
};
struct OutMember {
  unsigned long long pos_off;  // the member's first record in posm
  unsigned long long out_off;  // the bodies of the members before it: where its results begin in a call that starts at member 0
  int n;
  int reserved;
};
struct VelMember {
  unsigned long long pos_off;  // the member's first record in posm
  unsigned long long vel_off;  // the member's first record in velm
  unsigned long long out_off;  // the bodies of the members before it: where its results begin in a call that starts at member 0
  int n;
  int reserved;
};

// The member a workgroup of a ragged pair-work launch belongs to: member first + blockIdx.z of the table, and the launch shape
// of one system of its size, evaluated here as the host evaluates it.  points: the i side of every member, or 0 where the i side
// is the member's own bodies.
template <typename Member>
struct MemberGroup {
  const Member* range;  // the entry of member `first`
  Member mem;
  FieldShape shape;
  // the whole workgroup returns at once: this column or split is another, larger member's
  __device__ __forceinline__ bool elsewhere() const { return (int)blockIdx.x >= shape.columns || (int)blockIdx.y >= shape.splits; }
  // the bodies of the range before this member (the layouts that hold out_off)
  __device__ __forceinline__ size_t rel() const { return (size_t)(mem.out_off - range->out_off); }
};
template <typename Member>
__device__ __forceinline__ MemberGroup<Member> member_group(const Member* __restrict__ table, const unsigned first, const int points = 0) {
  const Member mem = table[first + blockIdx.z];
  return MemberGroup<Member>{table + first, mem, field_shape(points ? points : mem.n, mem.n)};
}

// The member that holds element idx of a finish launch over the bodies of `count` members.  table == nullptr: every system has
// n_all bodies, member idx / n_all of the range.  Otherwise the member is the last of table[first .. first + count) whose
// out_off, taken from member first, is not above idx.
struct MemberAt {
  int n;       // its bodies
  size_t rel;  // the bodies of the range before it
};
template <typename Member>
__device__ __forceinline__ MemberAt member_at(const Member* __restrict__ table, const unsigned first, const int count, const int n_all,
                                              const unsigned idx) {
  MemberAt at;
  if (table) {
    const unsigned long long base = table[first].out_off;
    int lo = 0, hi = count - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (table[first + mid].out_off - base <= idx) lo = mid;
      else hi = mid - 1;
    }
    at.n = table[first + lo].n;
    at.rel = (size_t)(table[first + lo].out_off - base);
  } else {
    at.n = n_all;
    at.rel = (size_t)(idx / (unsigned)n_all) * (size_t)n_all;
  }
  return at;
}

// Whether the tile that begins at record j0 runs the masked loop: it meets the workgroup's own bodies [g_lo, g_hi) or reaches
// past n.  Every other tile runs the loop without the mask compares.
__device__ __forceinline__ bool tile_masked(const int j0, const int g_lo, const int g_hi, const int n) {
  return (j0 < g_hi && j0 + kTile > g_lo) || j0 + kTile > n;
}

// The j tiles of split `split` of a system of n bodies, double-buffered.  The caller's loop runs k over [k0, k1) and calls
// stage(tile, k) first: tile k is staged in LDS by the 256 threads, one record each, and tile k + 1 is on its way into registers
// while the caller works on the staged one.  posm[0 .. ceil(n / 256) * 256) exist (the tail zero padding), so position records
// are read unguarded.
template <typename T4>
struct TileWalk {
  const T4* __restrict__ posm;
  int k0, k1;
  T4 next;
  __device__ __forceinline__ TileWalk(const T4* __restrict__ posm_, const int n, const int split, const int tiles_per_split) : posm(posm_) {
    const int tiles = (n + kTile - 1) / kTile;
    k0 = split * tiles_per_split;
    k1 = min(tiles, k0 + tiles_per_split);
    const int t = threadIdx.x;
    next = zero_record<T4>();
    if (k0 < k1) next = posm[k0 * kTile + t];
  }
  __device__ __forceinline__ void stage(T4* tile, const int k) {
    const int t = threadIdx.x;
    __syncthreads();  // every lane is done with the previous tile
    tile[t] = next;
    __syncthreads();
    if (k + 1 < k1) next = posm[(k + 1) * kTile + t];
  }
};

// The same walk over two arrays.  velm[0 .. n) alone exist: a velocity record at or beyond n is staged as zeros.
template <typename T4>
struct TileWalk2 {
  const T4* __restrict__ posm;
  const T4* __restrict__ velm;
  int n, k0, k1;
  T4 next_p, next_v;
  __device__ __forceinline__ TileWalk2(const T4* __restrict__ posm_, const T4* __restrict__ velm_, const int n_, const int split,
                                       const int tiles_per_split)
      : posm(posm_), velm(velm_), n(n_) {
    const int t = threadIdx.x;
    const int tiles = (n + kTile - 1) / kTile;
    k0 = split * tiles_per_split;
    k1 = min(tiles, k0 + tiles_per_split);
    next_p = next_v = zero_record<T4>();
    if (k0 < k1) {
      const int j = k0 * kTile + t;
      next_p = posm[j];
      if (j < n) next_v = velm[j];
    }
  }
  __device__ __forceinline__ void stage(T4* ptile, T4* vtile, const int k) {
    const int t = threadIdx.x;
    __syncthreads();  // every lane is done with the previous tile
    ptile[t] = next_p;
    vtile[t] = next_v;
    __syncthreads();
    if (k + 1 < k1) {
      const int j = (k + 1) * kTile + t;
      next_p = posm[j];
      next_v = zero_record<T4>();
      if (j < n) next_v = velm[j];
    }
  }
};

}  // namespace nbx
