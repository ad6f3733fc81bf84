// nbx_jlane.hpp -- the one-launch-per-step kernel body (NBX_KERNEL_JLANE) as device functions, and what it reads its
// arguments from.  Inline code only, so that several translation units can include it: nbx_kernels.hpp wraps the bodies into
// force_jlane_kernel / force_jlane_kernel_f64 (one system per launch, nbx_api.hip), nbx_ensemble_kernels.hpp into
// ensemble_step_kernel / ensemble_step_kernel_f64 (many systems per launch, nbx_ensemble.hip), nbx_ragged_kernels.hpp into
// ragged_step_kernel / ragged_step_kernel_f64 (systems of different size per launch, nbx_ragged.hip).  The workgroup index is an
// argument: a context passes blockIdx.x, an ensemble too -- after it has pointed the arguments at member blockIdx.y -- and a
// ragged ensemble the index its work list gives workgroup blockIdx.x within its member.  nbx_batch_accel_kernels.hpp and
// nbx_kick_kernels.hpp wrap the same bodies for the accelerations and the kicks of the members of either.
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_pair.hpp"  // V4, the pair term, euler_update, block_sum
#include "nbx_plan.hpp"  // kBlock, LOOP_*, kSgprOverread

namespace nbx {

template <typename T>
struct ForceArgs {
  const typename V4<T>::type* posm;  // current positions, n_alloc records
  typename V4<T>::type* accp;        // [gridDim.y][own_pad] partial-acceleration slabs (EPI_SLAB)
  typename V4<T>::type* velm;        // EPI_ROW: owned velocities, updated in place
  typename V4<T>::type* posm_next;   // EPI_ROW: next position buffer (owned slice written)
  double* ke_part;                   // EPI_ROW: one partial per workgroup (blockIdx.x)
  int i_begin, i_count, own_pad;
  int j_per_split;                   // split y covers [y*jps, min((y+1)*jps, n_alloc)); multiple of kTile for the
                                     // LDS source, of 4*kSgprBatch (2*kSgprBatch per wave under WSPLIT) for the SGPR one
  int n_alloc;                       // multiple of kTile
  T dt;
  const typename V4<T>::type* posm_pairs;  // LOOP_ASM with one body per lane: the pair-interleaved copy of posm (pair_transpose_kernel)
  unsigned slice_bit;                // LOOP_ASM_TS: clock bit of the priority slices (kSliceBit unless NBX_SLICE_BIT overrides)
};

// ---------------------------------------------------------------------------------------------
// jlane_step (the body of force_jlane_kernel: NBX_KERNEL_JLANE; fp32, tree order, launch-bound sizes): the roles of i and j swapped.
//   A WAVE owns NB bodies and holds them wave-uniformly (scalar loads -> SGPRs, two bodies per packed op).  Its 64
//   LANES each walk every 64th j record (lane l: j = l, l + 64, ...), one record per lane in VGPRs, requested D records
//   (one trip) ahead with coalesced 1-KiB loads.  Every lane ends with a partial sum for each of the NB bodies; a transpose through LDS
//   (one padded float4 column per body: conflict-free) lets lane t < NB add body t's 64 partials in lane order, and that
//   lane integrates the body at once (same euler_update as everywhere else) and contributes to the wave's energy partial.
// One launch per time step: no partial-acceleration slabs, no integrate kernel, no inter-workgroup hand-off -- which is
// what bounds n <= 16k (a step there was two dependent launches whose fixed costs exceeded the arithmetic: 21 us per
// step for 0.9 us of pair work at n = 2048).  Parallelism is ceil(own / NB) waves, so NB is chosen to give ~1024 waves
// (one per SIMD); the inner loop is the same 12 packed + 2 rsq instructions per two pairs as the other kernels.
// Summation order: j = lane (mod 64) ascending per lane, then lanes 0..63 in order -- a tree, like SGPRW's, so the kernel
// serves the tree-order range only (n <= 131072).  acc_only != 0: store the accelerations to accp instead
// of integrating (nbx_accel).
// ---------------------------------------------------------------------------------------------
#include "nbx_jlane_loop.inc"

// What lane t < NB does with body t's summed acceleration, as a compile-time choice:
//   JLANE_EPI_ARG   what the argument acc_only says -- store it (nbx_accel) or integrate the body (a step); the default, and the
//                   only form the step and accel kernels instantiate
//   JLANE_EPI_KICK  the velocity half of the update alone (include/nbx_kick.h): v += a * a.dt, velm[li] stored, the position
//                   neither advanced nor written, m v^2 of the kicked velocity into the workgroup's ke_part as a step does;
//                   acc_only is not looked at, and neither of the other two epilogues is compiled in
enum : int { JLANE_EPI_ARG = 0, JLANE_EPI_KICK = 1 };

// LOOP_ASM (NB = 2, 4, 8): whole trips of 8 records per lane go through the generated loop, a remainder of four records
// through the compiled one -- the same operations in the same order either way (tests compare the bits).
template <int NB, int D, int LOOP, int EPI = JLANE_EPI_ARG>
__device__ __forceinline__ void jlane_step(const ForceArgs<float>& a, const int acc_only, const unsigned wg) {
  static_assert(NB % 2 == 0 && NB >= 2 && NB <= 16 && D >= 1, "two bodies per packed operation; body state must fit the SGPR file");
  static_assert(LOOP == LOOP_CXX || NB <= 8, "the generated loop exists for 2, 4 and 8 bodies per wave");
  __shared__ float4 red[4][NB][65];  // [wave][body][lane], one float4 of padding per column: lanes t read 1040 B apart
  __shared__ double ksum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(wg * 4 + w);
  const int b0 = wave * NB;

  f32x2 xi[NB / 2], yi[NB / 2], zi[NB / 2], ax[NB / 2], ay[NB / 2], az[NB / 2];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    int li = b0 + b;
    li = li < a.i_count ? li : a.i_count - 1;  // waves / bodies past the end shadow the last owned body
    const float4 p = a.posm[a.i_begin + li];   // wave-uniform index: a scalar load
    xi[b / 2][b & 1] = p.x; yi[b / 2][b & 1] = p.y; zi[b / 2][b & 1] = p.z;
    ax[b / 2][b & 1] = 0.f; ay[b / 2][b & 1] = 0.f; az[b / 2][b & 1] = 0.f;
  }

  // the body lane t < NB will integrate at the end: its position and velocity are requested now, so that the two loads
  // land under the j loop instead of in front of the epilogue (at n = 2048 the whole launch is a few microseconds)
  const int li = b0 + lane;
  const bool mine = lane < NB && li < a.i_count;
  float4 pe = make_float4(0.f, 0.f, 0.f, 0.f), ve = pe;
  if (mine) {
    pe = a.posm[a.i_begin + li];
    ve = a.velm[li];
  }

  // Two register sets of D records ping-pong: the loads of the NEXT D records are issued before the current D are
  // applied, so a request has D x NB/2 x 56 cycles of arithmetic to land under (one wave per SIMD has no other wave to
  // hide an L2 round trip behind).  Requests may run up to D blocks past the end of the array (zero-filled spare records,
  // kSgprOverread); what they return is never applied.
  static_assert(64 * D <= kSgprOverread - 16, "the farthest request is D blocks of 64 records past the array (main loop: ra at k + 2 D <= K; the tail requests rb only when part of it is applied)");
  const float4* pj = a.posm + lane;
  const int K = a.n_alloc >> 6;  // records per lane; n_alloc is a multiple of 256, so K >= 4
  float4 ra[D], rb[D];
  auto request = [&](float4 (&r)[D], int k0) {
#pragma unroll
    for (int d = 0; d < D; ++d) r[d] = pj[(size_t)64 * (k0 + d)];
  };
  // one record on body pairs (p, p + 1), or -- a wave with a single body pair -- two records on that pair: two pinned,
  // interleaved instruction streams either way (pair2_x2)
  auto apply_record = [&](const float4& r) {
    if constexpr (NB >= 4) {
#pragma unroll
      for (int p = 0; p < NB / 2; p += 2)
        pair2_x2<false>(r.x, r.y, r.z, r.w, xi[p], yi[p], zi[p], ax[p], ay[p], az[p], r.x, r.y, r.z, r.w, xi[p + 1], yi[p + 1], zi[p + 1],
                        ax[p + 1], ay[p + 1], az[p + 1]);
    } else {
      pair2(r.x, r.y, r.z, r.w, xi[0], yi[0], zi[0], ax[0], ay[0], az[0]);
    }
  };
  auto apply = [&](const float4 (&r)[D]) {
    if constexpr (NB >= 4) {
#pragma unroll
      for (int d = 0; d < D; ++d) apply_record(r[d]);
    } else {
      static_assert(NB >= 4 || D % 2 == 0, "a single body pair takes its records two at a time");
#pragma unroll
      for (int d = 0; d < D; d += 2)
        pair2_x2<true>(r[d].x, r[d].y, r[d].z, r[d].w, xi[0], yi[0], zi[0], ax[0], ay[0], az[0], r[d + 1].x, r[d + 1].y, r[d + 1].z,
                       r[d + 1].w, xi[0], yi[0], zi[0], ax[0], ay[0], az[0]);
    }
  };
  auto apply_some = [&](const float4 (&r)[D], int count) {  // wave-uniform count in [0, D]
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (d < count) apply_record(r[d]);
  };
  int k = 0;
  if constexpr (LOOP == LOOP_ASM) {
    const int trips = K >> 3;  // K is a multiple of 4: the remainder is 0 or 4 records
    if (trips > 0) {
      if constexpr (NB == 2) jlane_loop_asm_nb2(a.posm, trips, xi, yi, zi, ax, ay, az);
      else if constexpr (NB == 4) jlane_loop_asm_nb4(a.posm, trips, xi, yi, zi, ax, ay, az);
      else jlane_loop_asm_nb8(a.posm, trips, xi, yi, zi, ax, ay, az);
      k = trips << 3;
    }
    if (k < K) request(ra, k);
  } else {
    request(ra, 0);
    for (; k + 2 * D <= K; k += 2 * D) {
      request(rb, k + D);
      apply(ra);
      request(ra, k + 2 * D);
      apply(rb);
    }
  }
  if (k < K) {  // fewer than 2 D records left: ra holds records k .. k + D - 1
    // rb is requested only if any of it will be applied: the farthest request of the whole kernel is then the main loop's
    // ra at k + 2 D <= K, i.e. at most D blocks (64 D records) past the array -- what kSgprOverread reserves
    if (K - k > D) request(rb, k + D);
    apply_some(ra, K - k < D ? K - k : D);
    apply_some(rb, K - k - D > 0 ? K - k - D : 0);
  }

  // lane partials -> LDS columns; lane t < NB adds the 64 partials of body t in lane order
#pragma unroll
  for (int b = 0; b < NB; ++b) red[w][b][lane] = make_float4(ax[b / 2][b & 1], ay[b / 2][b & 1], az[b / 2][b & 1], 0.f);
  __builtin_amdgcn_wave_barrier();  // same wave, in-order LDS queue: the reads below see the writes above
  double ke = 0.0;
  if (mine) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 8
    for (int l = 0; l < 64; ++l) {
      const float4 q = red[w][lane][l];
      sx += q.x; sy += q.y; sz += q.z;
    }
    if constexpr (EPI == JLANE_EPI_KICK) {
      ke = (double)kick_update<float>(sx, sy, sz, a.dt, ve);
      a.velm[li] = ve;
    } else if (acc_only) {
      a.accp[li] = make_float4(sx, sy, sz, 0.f);
    } else {
      ke = (double)euler_update<float>(sx, sy, sz, a.dt, pe, ve);
      a.velm[li] = ve;
      a.posm_next[a.i_begin + li] = pe;
    }
  }
  // one energy partial per workgroup, fixed order (wave shuffle tree, then the four waves)
  const double s = block_sum(ke, ksum);
  if (threadIdx.x == 0 && (EPI == JLANE_EPI_KICK || !acc_only)) a.ke_part[wg] = s;
}

// The fp64 form of jlane_step: same decomposition (a wave owns NB bodies wave-uniformly, its lanes split j, LDS
// transpose, the wave integrates its own bodies), plain fp64 arithmetic (pair<double>: there is no packed fp64), records
// of 32 bytes.  NB <= 8: eight bodies are 48 SGPRs of coordinates.
template <int NB, int D, int EPI = JLANE_EPI_ARG>
__device__ __forceinline__ void jlane_step_f64(const ForceArgs<double>& a, const int acc_only, const unsigned wg) {
  static_assert(NB >= 1 && NB <= 8 && D >= 1 && 64 * D <= kSgprOverread - 16, "body state must fit the SGPR file; the farthest request is D blocks past the array");
  __shared__ double4 red[4][NB][65];  // [wave][body][lane] + one column of padding (2080 B between the lanes that read)
  __shared__ double ksum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(wg * 4 + w);
  const int b0 = wave * NB;
  double xi[NB], yi[NB], zi[NB], ax[NB], ay[NB], az[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    int li = b0 + b;
    li = li < a.i_count ? li : a.i_count - 1;
    const double4 p = a.posm[a.i_begin + li];  // wave-uniform index: scalar loads
    xi[b] = p.x; yi[b] = p.y; zi[b] = p.z;
    ax[b] = ay[b] = az[b] = 0.0;
  }
  const int li = b0 + lane;
  const bool mine = lane < NB && li < a.i_count;
  double4 pe = make_double4(0.0, 0.0, 0.0, 0.0), ve = pe;
  if (mine) {
    pe = a.posm[a.i_begin + li];
    ve = a.velm[li];
  }
  const double4* pj = a.posm + lane;
  const int K = a.n_alloc >> 6;
  double4 ra[D], rb[D];
  auto request = [&](double4 (&r)[D], int k0) {
#pragma unroll
    for (int d = 0; d < D; ++d) r[d] = pj[(size_t)64 * (k0 + d)];
  };
  auto apply_record = [&](const double4& r) {
#pragma unroll
    for (int b = 0; b < NB; ++b) pair<double>(r.x, r.y, r.z, r.w, xi[b], yi[b], zi[b], ax[b], ay[b], az[b]);
  };
  int k = 0;
  request(ra, 0);
  for (; k + 2 * D <= K; k += 2 * D) {
    request(rb, k + D);
#pragma unroll
    for (int d = 0; d < D; ++d) apply_record(ra[d]);
    request(ra, k + 2 * D);
#pragma unroll
    for (int d = 0; d < D; ++d) apply_record(rb[d]);
  }
  if (k < K) {
    if (K - k > D) request(rb, k + D);  // as in the fp32 kernel: never more than D blocks past the array
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (k + d < K) apply_record(ra[d]);
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (k + D + d < K) apply_record(rb[d]);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) red[w][b][lane] = make_double4(ax[b], ay[b], az[b], 0.0);
  __builtin_amdgcn_wave_barrier();
  double ke = 0.0;
  if (mine) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll 8
    for (int l = 0; l < 64; ++l) {
      const double4 q = red[w][lane][l];
      sx += q.x; sy += q.y; sz += q.z;
    }
    if constexpr (EPI == JLANE_EPI_KICK) {
      ke = kick_update<double>(sx, sy, sz, a.dt, ve);
      a.velm[li] = ve;
    } else if (acc_only) {
      a.accp[li] = make_double4(sx, sy, sz, 0.0);
    } else {
      ke = euler_update<double>(sx, sy, sz, a.dt, pe, ve);
      a.velm[li] = ve;
      a.posm_next[a.i_begin + li] = pe;
    }
  }
  const double s = block_sum(ke, ksum);
  if (threadIdx.x == 0 && (EPI == JLANE_EPI_KICK || !acc_only)) a.ke_part[wg] = s;
}

}  // namespace nbx
