// nbx_kernels.hpp -- hand-written HIP kernels for gfx950 (MI355X, CDNA4).
//
// The per-time-step work of the reference's GSimulation::start()
// (ver7/GSimulation.cpp:138-200):
//   force_kernel        all-pairs softened-gravity acceleration   (ver7:141-177)
//   integrate_kernel    v += a*dt; x += v*dt; m*v^2 partial sums  (ver7:178-198)
//   ke_reduce_kernel    ordered final sum of the partials         (ver7:179,200)
//   force_exact_kernel  validation: the reference build's arithmetic, bit for bit
//
// Data layout in HBM (all resident for the lifetime of a context):
//   posm[2][n_alloc]  {x, y, z, G*m}   one 16 B (fp32) / 32 B (fp64) record per body, double
//                     buffered: step s reads posm[cur] (every body, as j) and writes the owned
//                     slice of posm[cur^1]; entries >= n are {0,0,0,0} (zero mass => the pair term
//                     is exactly 0, so tiles need no bounds checks).
//   velm[own]         {vx, vy, vz, m}  owned slice only; velocities never leave their owner.
//   accp[S][own_pad]  {ax, ay, az, -}  partial accelerations when S workgroups split the j range.
//   ke_part[blocks]   fp64 block partials of sum m*v^2, reduced in fixed order (deterministic).
//
// Execution shape: 256-thread workgroups (4 wave64, one per SIMD).  Each lane keeps B i-bodies
// in registers (register blocking: one j record feeds B independent 13-instruction chains, which
// hides the v_rsq_f32 latency and amortises the j fetch).  The j records come either from an LDS
// tile (256 records, double buffered, every lane reads the same address => broadcast
// ds_read_b128, no bank conflicts) or from wave-uniform scalar loads (hand-pipelined
// s_load_dwordx16 into SGPRs: costs neither LDS bandwidth nor VGPRs).  No MFMA: the pair kernel is
// rsqrt/FMA-chain bound and its contraction forms cancel catastrophically in fp32.
//
// Two summation orders (include/nbx.h): REFERENCE = one accumulator per body over all
// j ascending (grid.y = 1; reproduces the reference's rounding noise, which is what parity means at
// n >= 262144), TREE = the four waves of a workgroup and grid.y workgroups each sum a j sub-range and
// the partials are added in fixed order (fastest, closest to an fp64 sum).
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_jlane.hpp"  // ForceArgs; the one-launch kernel body (jlane_step), nbx_jlane_loop.inc
#include "nbx_pair.hpp"  // V4, the pair term, euler_update, block_sum
#include "nbx_plan.hpp"  // kBlock, kTile, the shape enums JSRC_*, MATH_*, LOOP_*, EPI_* (what they mean: there)

namespace nbx {

// records per scalar-load batch of the SGPR source (one s_load_dwordx16 = 64 B); a split's j range
// (a quarter of it under WSPLIT) must be a multiple of this
template <typename T> constexpr int kSgprBatch = 64 / (4 * (int)sizeof(T));

// One 64-byte batch of j records held in 16 SGPRs, loaded by an asm s_load_dwordx16 the compiler cannot
// sink.  load() only requests; wait() is the first point at which the values may be read.
template <typename T> struct SgprBatch;
template <> struct SgprBatch<float> {
  typedef float v16 __attribute__((ext_vector_type(16)));
  v16 r;
  __device__ __forceinline__ void load_first(const void* p) {
    // s_nop: the address may have been produced by v_readfirstlane just before (VALU-written SGPR -> SMEM)
    asm volatile("s_nop 4\n\ts_load_dwordx16 %0, %1, 0x0" : "=s"(r) : "s"(p));
  }
  __device__ __forceinline__ void load(const void* p) { asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(r) : "s"(p)); }
  __device__ __forceinline__ void wait() { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r)); }
  __device__ __forceinline__ float x(int u) const { return r[4 * u]; }
  __device__ __forceinline__ float y(int u) const { return r[4 * u + 1]; }
  __device__ __forceinline__ float z(int u) const { return r[4 * u + 2]; }
  __device__ __forceinline__ float w(int u) const { return r[4 * u + 3]; }
};
template <> struct SgprBatch<double> {
  typedef double v8 __attribute__((ext_vector_type(8)));
  v8 r;
  __device__ __forceinline__ void load_first(const void* p) {
    asm volatile("s_nop 4\n\ts_load_dwordx16 %0, %1, 0x0" : "=s"(r) : "s"(p));
  }
  __device__ __forceinline__ void load(const void* p) { asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(r) : "s"(p)); }
  __device__ __forceinline__ void wait() { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r)); }
  __device__ __forceinline__ double x(int u) const { return r[4 * u]; }
  __device__ __forceinline__ double y(int u) const { return r[4 * u + 1]; }
  __device__ __forceinline__ double z(int u) const { return r[4 * u + 2]; }
  __device__ __forceinline__ double w(int u) const { return r[4 * u + 3]; }
};
// one s_waitcnt for a group of batches: names every destination "+s" so no consumer is scheduled above it
template <typename T, int G>
__device__ __forceinline__ void sgpr_wait(SgprBatch<T> (&b)[G]) {
  if constexpr (G == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b[0].r));
  else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b[0].r), "+s"(b[1].r));
}

// clock bit (s_memrealtime counts 10 ns) that selects the favoured slot parity: slices of 2^16 x 10 ns = 0.66 ms.  Measured
// 2^14 ... 2^19 within 1 % of each other, 2^16-2^17 best; shorter slices lose to the time the unfavoured wave needs to reach
// its next decision, longer ones to the imbalance of the last slice.
constexpr unsigned kSliceBit = 1u << 16;
#include "nbx_sgpr_loop.inc"

// The B i-bodies a lane keeps in registers, and how one j record is applied to them.
template <typename T, int B, int MATH>
struct IBodies {
  T xi[B], yi[B], zi[B], ax[B], ay[B], az[B];
  __device__ __forceinline__ void set(int b, T x, T y, T z) {
    xi[b] = x; yi[b] = y; zi[b] = z;
    ax[b] = ay[b] = az[b] = (T)0;
  }
  __device__ __forceinline__ void apply(T xj, T yj, T zj, T gmj) {
#pragma unroll
    for (int b = 0; b < B; ++b) pair<T>(xj, yj, zj, gmj, xi[b], yi[b], zi[b], ax[b], ay[b], az[b]);
  }
  __device__ __forceinline__ void get(int b, T& x, T& y, T& z) const { x = ax[b]; y = ay[b]; z = az[b]; }
};

template <int B>
struct IBodies<float, B, MATH_PACKED> {
  static_assert(B % 2 == 0, "packed math needs an even number of bodies per lane");
  f32x2 xi[B / 2], yi[B / 2], zi[B / 2], ax[B / 2], ay[B / 2], az[B / 2];
  __device__ __forceinline__ void set(int b, float x, float y, float z) {
    xi[b / 2][b & 1] = x; yi[b / 2][b & 1] = y; zi[b / 2][b & 1] = z;
    ax[b / 2][b & 1] = 0.f; ay[b / 2][b & 1] = 0.f; az[b / 2][b & 1] = 0.f;
  }
  __device__ __forceinline__ void apply(float xj, float yj, float zj, float gmj) {
#pragma unroll
    for (int b = 0; b < B / 2; ++b) pair2(xj, yj, zj, gmj, xi[b], yi[b], zi[b], ax[b], ay[b], az[b]);
  }
  __device__ __forceinline__ void get(int b, float& x, float& y, float& z) const {
    x = ax[b / 2][b & 1]; y = ay[b / 2][b & 1]; z = az[b / 2][b & 1];
  }
  // all records of [first, last) in ascending order through the hand-scheduled loop (LOOP_ASM)
  __device__ __forceinline__ void apply_range_asm(const float4* first, const float4* last) {
    static_assert(B == 2 || B == 4, "the asm loop exists for 2 and 4 bodies per lane");
    if constexpr (B == 2) sgpr_loop_asm_b2(first, last, xi[0], yi[0], zi[0], ax[0], ay[0], az[0]);
    else sgpr_loop_asm_b4(first, last, xi[0], yi[0], zi[0], xi[1], yi[1], zi[1], ax[0], ay[0], az[0], ax[1], ay[1], az[1]);
  }
  // the same with the L2 prefetch (LOOP_ASM_PF)
  __device__ __forceinline__ void apply_range_asm_pf(const float4* first, const float4* last) {
    static_assert(B == 2 || B == 4, "the asm loop exists for 2 and 4 bodies per lane");
    if constexpr (B == 2) sgpr_loop_asm_b2_pf(first, last, xi[0], yi[0], zi[0], ax[0], ay[0], az[0]);
    else sgpr_loop_asm_b4_pf(first, last, xi[0], yi[0], zi[0], xi[1], yi[1], zi[1], ax[0], ay[0], az[0], ax[1], ay[1], az[1]);
  }
  // the same with time-sliced wave priority (LOOP_ASM_TS); slot_bit = slice_bit for waves in odd slots of their SIMD, else 0
  __device__ __forceinline__ void apply_range_asm_ts(const float4* first, const float4* last, unsigned slice_bit, unsigned slot_bit) {
    static_assert(B == 2 || B == 4, "the asm loop exists for 2 and 4 bodies per lane");
    if constexpr (B == 2) sgpr_loop_asm_b2_ts(first, last, slice_bit, slot_bit, xi[0], yi[0], zi[0], ax[0], ay[0], az[0]);
    else sgpr_loop_asm_b4_ts(first, last, slice_bit, slot_bit, xi[0], yi[0], zi[0], xi[1], yi[1], zi[1], ax[0], ay[0], az[0], ax[1], ay[1], az[1]);
  }
};

// ---------------------------------------------------------------------------------------------
// force_kernel: block 256 = 4 wave64.
//   WSPLIT == false: grid (ceil(i_count / (256*B)), S).  Lane t of workgroup bx owns bodies
//     i_begin + bx*256*B + b*256 + t, b = 0..B-1, and every wave walks the whole j range of split y.
//   WSPLIT == true (small n, SGPR source only): grid (ceil(i_count / (64*B)), S).  The four waves own
//     the SAME 64*B bodies (lane l: bx*64*B + b*64 + l) and each walks one quarter of the split's
//     j range; the four partial sums are added in wave order through LDS.  Four times the workgroups
//     for the same number of partial-acceleration slabs.
// ---------------------------------------------------------------------------------------------
template <typename T, int B, int JSRC, int EPI, int MINW, int MATH = MATH_SCALAR, bool WSPLIT = false, int LOOP = LOOP_CXX>
__global__ __launch_bounds__(kBlock, MINW) void force_kernel(const ForceArgs<T> a) {
  using T4 = typename V4<T>::type;
  static_assert(!WSPLIT || (JSRC == JSRC_SGPR && EPI != EPI_ROW), "wave split exists for the SGPR kernel with slabs only");
  static_assert(LOOP == LOOP_CXX || (JSRC == JSRC_SGPR && MATH == MATH_PACKED && sizeof(T) == 4 && (B == 2 || B == 4)) ||
                    (LOOP == LOOP_ASM && JSRC == JSRC_SGPR && MATH == MATH_SCALAR && sizeof(T) == 4 && B == 1 && !WSPLIT),
                "the hand-scheduled loop exists for the packed fp32 SGPR kernels with 2 or 4 bodies per lane, and as the two-records-per-operation loop for 1");
  const int t = threadIdx.x;
  constexpr int kStride = WSPLIT ? 64 : kBlock;  // distance between a lane's consecutive bodies
  const int base = blockIdx.x * (kStride * B) + (WSPLIT ? (t & 63) : t);

  IBodies<T, B, MATH> ib;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    int li = base + b * kStride;
    li = li < a.i_count ? li : a.i_count - 1;  // padded lanes shadow the last owned body
    const T4 p = a.posm[a.i_begin + li];
    ib.set(b, p.x, p.y, p.z);
  }

  int j0 = blockIdx.y * a.j_per_split;
  int j1 = j0 + a.j_per_split;
  j1 = j1 < a.n_alloc ? j1 : a.n_alloc;
  if constexpr (WSPLIT) {
    // wave-uniform quarter of [j0, j1); quarter length is a multiple of the load batch
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int q = a.j_per_split >> 2;
    j0 += wave * q;
    const int e = j0 + q;
    j1 = e < j1 ? e : j1;
  }

  if constexpr (JSRC == JSRC_LDS) {
    __shared__ T4 tile[2][kTile];
    T4 pre = a.posm[j0 + t];
    tile[0][t] = pre;
    __syncthreads();
    int cur = 0;
    for (int jt = j0; jt < j1; jt += kTile) {
      const bool more = jt + kTile < j1;
      if (more) pre = a.posm[jt + kTile + t];  // in flight under the tile's arithmetic
      const T4* tl = tile[cur];
#pragma unroll 8
      for (int jj = 0; jj < kTile; ++jj) {
        const T4 pj = tl[jj];  // same address in every lane: broadcast read
        ib.apply(pj.x, pj.y, pj.z, pj.w);
      }
      if (more) tile[cur ^ 1][t] = pre;
      __syncthreads();  // one barrier per tile: readers of `cur` done, writers of `cur^1` done
      cur ^= 1;
    }
  } else if constexpr (LOOP == LOOP_ASM) {
    // j range = a positive multiple of kSgprAsmTrip<B> records (the host rounds j_per_split to 64, to 256 under WSPLIT where a
    // wave walks a quarter of it; n_alloc is a multiple of 256)
    if constexpr (B == 1) {
      // one body per lane: two consecutive j records per packed operation, out of the pair-interleaved copy (same offsets)
      if (j0 < j1) sgpr_loop_asm_jpair(a.posm_pairs + j0, a.posm_pairs + j1, f32x2{ib.xi[0], ib.yi[0]}, f32x2{ib.zi[0], ib.zi[0]}, ((unsigned)t & (kSgprJpairPrefetchLines - 1u)) * 64u + kSgprJpairPrefetchBytes, ib.ax[0], ib.ay[0], ib.az[0]);
    } else {
      if (j0 < j1) ib.apply_range_asm(a.posm + j0, a.posm + j1);
    }
  } else if constexpr (LOOP == LOOP_ASM_PF) {
    if (j0 < j1) ib.apply_range_asm_pf(a.posm + j0, a.posm + j1);
  } else if constexpr (LOOP == LOOP_ASM_TS) {
    if (j0 < j1) {
      unsigned hwid;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));  // bits 3:0 = the wave's slot on its SIMD
      const unsigned slice = __builtin_amdgcn_readfirstlane(a.slice_bit);
      ib.apply_range_asm_ts(a.posm + j0, a.posm + j1, slice, (hwid & 1u) ? slice : 0u);
      __builtin_amdgcn_s_setprio(0);
    }
  } else {
    // Wave-uniform j index => the records travel by s_load_dwordx16 (64 B = kSgprBatch records) into
    // SGPRs and feed the VALU as scalar operands: no LDS bandwidth, no VGPRs, no barrier.  Two
    // register batches ping-pong: the load of the NEXT batch is issued before the current one is
    // consumed, so the scalar-cache latency sits under ~200 VALU instructions even when a SIMD holds
    // a single wave (small n).  hipcc would sink a plain C++ prefetch back to its use, so the loads
    // are asm statements (guide section 5.7 form (ii): "=s" load, later a wait naming the destination
    // "+s"; SMEM returns out of order, hence lgkmcnt(0)).  The final trip over-reads one batch past
    // the split; the array carries kSgprOverread spare records for the last split.
    constexpr int U = kSgprBatch<T>;
    // G batches travel together.  SMEM returns out of order, so only lgkmcnt(0) is a usable wait: the cover a
    // request gets is the arithmetic of ONE group.  The wave-split kernel runs 8 waves per SIMD and needs <= 80 SGPRs
    // (G = 1); the plain SGPR kernel serves the reference-order shapes, which run 1-2 waves per SIMD when a rank owns
    // few bodies and need the longer cover of G = 2 (8 j records, 64 SGPRs of payload).
    constexpr int G = WSPLIT ? 1 : 2;
    const char* p = reinterpret_cast<const char*>(a.posm + j0);
    if (j0 < j1) {
      SgprBatch<T> ba[G];
      ba[0].load_first(p);
#pragma unroll
      for (int g = 1; g < G; ++g) ba[g].load(p + 64 * g);
      sgpr_wait<T, G>(ba);
      // Invariant at the loop head AND at the back edge: group `ba` has landed.  No asm-loaded value is in flight
      // across the back edge, so a register copy the compiler may insert for the loop-carried value can never read
      // (or be overtaken by) a pending scalar load.  tests/test_isa_audit.py checks the compiled code: nothing touches
      // a batch's SGPRs between its s_load and the next s_waitcnt lgkmcnt(0).
      for (int j = j0; j < j1; j += 2 * G * U) {
        SgprBatch<T> bb[G];
#pragma unroll
        for (int g = 0; g < G; ++g) bb[g].load(p + 64 * (G + g));
        __builtin_amdgcn_sched_barrier(0);  // keep the arithmetic below the requests (no operand ties it)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < U; ++u) ib.apply(ba[g].x(u), ba[g].y(u), ba[g].z(u), ba[g].w(u));
        __builtin_amdgcn_sched_barrier(0);
        sgpr_wait<T, G>(bb);
#pragma unroll
        for (int g = 0; g < G; ++g) ba[g].load(p + 64 * (2 * G + g));  // next trip's first group (over-read on the last trip)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < U; ++u) ib.apply(bb[g].x(u), bb[g].y(u), bb[g].z(u), bb[g].w(u));
        __builtin_amdgcn_sched_barrier(0);
        sgpr_wait<T, G>(ba);
        p += 128 * G;
      }
    }
  }

  if constexpr (EPI == EPI_ROW) {
    __shared__ double ksum[4];
    double ke = 0.0;
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int li = base + b * kBlock;
      if (li < a.i_count) {
        T4 p = a.posm[a.i_begin + li];
        T4 v = a.velm[li];
        T axb, ayb, azb;
        ib.get(b, axb, ayb, azb);
        ke += (double)euler_update<T>(axb, ayb, azb, a.dt, p, v);
        a.velm[li] = v;
        a.posm_next[a.i_begin + li] = p;
      }
    }
    const double s = block_sum(ke, ksum);
    if (t == 0) a.ke_part[blockIdx.x] = s;
    return;
  }

  // ---- this workgroup's partial accelerations -> slab blockIdx.y -------------------------------
  T4* out = a.accp + (size_t)blockIdx.y * a.own_pad;
  if constexpr (WSPLIT) {
    __shared__ T red[3][3][B][64];  // [wave-1][component][body][lane]
    const int lane = t & 63, wave = t >> 6;
    if (wave > 0) {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        T x, y, z;
        ib.get(b, x, y, z);
        red[wave - 1][0][b][lane] = x; red[wave - 1][1][b][lane] = y; red[wave - 1][2][b][lane] = z;
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const int li = base + b * kStride;
        T4 r;
        ib.get(b, r.x, r.y, r.z);
#pragma unroll
        for (int w = 0; w < 3; ++w) { r.x += red[w][0][b][lane]; r.y += red[w][1][b][lane]; r.z += red[w][2][b][lane]; }
        r.w = (T)0;
        if (li < a.i_count) out[li] = r;
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int li = base + b * kBlock;
      if (li < a.i_count) {
        T4 r;
        ib.get(b, r.x, r.y, r.z);
        r.w = (T)0;
        out[li] = r;
      }
    }
  }

}

// ---------------------------------------------------------------------------------------------
// force_jlane_kernel / force_jlane_kernel_f64 (NBX_KERNEL_JLANE): one launch per time step for launch-bound sizes.  The bodies are
// jlane_step / jlane_step_f64 of nbx_jlane.hpp (described there), which the ensemble kernels of nbx_ensemble_kernels.hpp run too.
// ---------------------------------------------------------------------------------------------
template <int NB, int D, int LOOP = LOOP_CXX>
__global__ __launch_bounds__(kBlock, 1) void force_jlane_kernel(const ForceArgs<float> a, const int acc_only) {
  jlane_step<NB, D, LOOP>(a, acc_only, blockIdx.x);
}
template <int NB, int D>
__global__ __launch_bounds__(kBlock, 1) void force_jlane_kernel_f64(const ForceArgs<double> a, const int acc_only) {
  jlane_step_f64<NB, D>(a, acc_only, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// force_exact_kernel (NBX_KERNEL_EXACT): the reference's acceleration loop with the reference's rounding.
// The pinned build of ver7 (g++ -O2, x86-64 baseline) compiles ver7/GSimulation.cpp:153-173 to a scalar,
// strictly sequential loop: r2 = ((dx*dx + dy*dy) + dz*dz) + eps, inv = 1.0f / sqrtf(r2) (IEEE sqrtss, divss),
// term = ((((d*G)*m)*inv)*inv)*inv, sum += term for j = 0..n-1, acc = 0 + sum.  One thread per body does exactly
// that: contraction off, HIP's correctly rounded fp32 sqrt and divide.  Validation path, not a fast path.
// ---------------------------------------------------------------------------------------------
// The reference's loop body, spelled once; the fp-contract pragma is lexical, so the text is instantiated inside
// each pragma's scope below.
#define NBX_EXACT_ROW()                                                            \
  T sx = (T)0, sy = (T)0, sz = (T)0;                                               \
  for (int j = 0; j < n; ++j) {                                                    \
    const T4 pj = posm[j];                                                         \
    const T m = mass[j];                                                           \
    const T dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;                  \
    const T r2 = ((dx * dx + dy * dy) + dz * dz) + eps;                            \
    const T inv = (T)1 / sqrt(r2);                                                 \
    sx = sx + ((((dx * G) * m) * inv) * inv) * inv;                                \
    sy = sy + ((((dy * G) * m) * inv) * inv) * inv;                                \
    sz = sz + ((((dz * G) * m) * inv) * inv) * inv;                                \
  }                                                                                \
  r.x = (T)0 + sx; r.y = (T)0 + sy; r.z = (T)0 + sz;

// CONTRACT = false: contraction off (the pinned reference build).  CONTRACT = true: the same source lines with FMA
// contraction allowed, i.e. another legitimate build of the reference (diagnostic NBX_KERNEL_EXACT_FMA).
template <typename T, bool CONTRACT>
__global__ __launch_bounds__(kBlock) void force_exact_kernel(const typename V4<T>::type* __restrict__ posm,
                                                             const T* __restrict__ mass,
                                                             typename V4<T>::type* __restrict__ accp, int i_begin,
                                                             int i_count, int n) {
  using T4 = typename V4<T>::type;
  const int li = blockIdx.x * kBlock + threadIdx.x;
  if (li >= i_count) return;
  const T4 pi = posm[i_begin + li];
  const T eps = softening2<T>(), G = grav_const<T>();
  T4 r;
  r.w = (T)0;
  if constexpr (CONTRACT) {
#pragma clang fp contract(fast)
    NBX_EXACT_ROW()
  } else {
#pragma clang fp contract(off)
    NBX_EXACT_ROW()
  }
  accp[li] = r;
}
#undef NBX_EXACT_ROW

// ---------------------------------------------------------------------------------------------
// pair_transpose_kernel: the pair-interleaved copy of the record array that sgpr_loop_asm_jpair reads.  Records 2k and 2k+1,
// {x0 y0 z0 w0}{x1 y1 z1 w1}, become {x0 x1 y0 y1}{z0 z1 w0 w1} at the same byte offset: a packed operand is one aligned 64-bit
// register pair, so the two records a packed instruction works on must be neighbours component by component.  One thread per
// pair, 32 B in and 32 B out, once per step in front of the force launch (n = 1M: 32 MiB of L2 / Infinity-Cache traffic, ~10 us
// against a 15 ms step); npairs = n_alloc / 2 (the spare records behind the array stay zero in both layouts).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pair_transpose_kernel(const float4* __restrict__ posm, float4* __restrict__ pairs, int npairs) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= npairs) return;
  const float4 a = posm[2 * k], b = posm[2 * k + 1];
  pairs[2 * k] = make_float4(a.x, b.x, a.y, b.y);
  pairs[2 * k + 1] = make_float4(a.z, b.z, a.w, b.w);
}

// ---------------------------------------------------------------------------------------------
// integrate_kernel: one body per thread; sums the S partial accelerations in split order.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void integrate_kernel(const typename V4<T>::type* __restrict__ posm_cur,
                                                           typename V4<T>::type* __restrict__ posm_next,
                                                           typename V4<T>::type* __restrict__ velm,
                                                           const typename V4<T>::type* __restrict__ accp,
                                                           int nsplit, int own_pad, int i_begin, int i_count,
                                                           T dt, double* __restrict__ ke_part) {
  using T4 = typename V4<T>::type;
  __shared__ double ksum[4];
  const int li = blockIdx.x * kBlock + threadIdx.x;
  double ke = 0.0;
  if (li < i_count) {
    T ax = (T)0, ay = (T)0, az = (T)0;
    for (int s = 0; s < nsplit; ++s) {
      const T4 q = accp[(size_t)s * own_pad + li];
      ax += q.x; ay += q.y; az += q.z;
    }
    T4 p = posm_cur[i_begin + li];
    T4 v = velm[li];
    ke = (double)euler_update<T>(ax, ay, az, dt, p, v);
    velm[li] = v;
    posm_next[i_begin + li] = p;
  }
  const double s = block_sum(ke, ksum);
  if (threadIdx.x == 0) ke_part[blockIdx.x] = s;
}

// One workgroup; thread t sums partials t, t+256, ... then the block tree: fixed order.
__global__ __launch_bounds__(kBlock) void ke_reduce_kernel(const double* __restrict__ ke_part, int nparts,
                                                           double* __restrict__ out) {
  __shared__ double ksum[4];
  double v = 0.0;
  for (int k = threadIdx.x; k < nparts; k += kBlock) v += ke_part[k];
  const double s = block_sum(v, ksum);
  if (threadIdx.x == 0) *out = s;
}

}  // namespace nbx
