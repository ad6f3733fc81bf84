// nbx_pair.hpp -- the arithmetic every gfx950 kernel of libnbx.so shares: launch constants, record types, the physical
// constants, the pair term and its packed forms, the reference-rounded Euler update and the fixed-order workgroup sum.
// Inline code only, so that more than one translation unit can include it (nbx_kernels.hpp for the step kernels of
// nbx_api.hip, nbx_diag_kernels.hpp for the diagnostics of nbx_diag.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "nbx_plan.hpp"  // kBlock, kTile

namespace nbx {

template <typename T> struct V4;
template <> struct V4<float> { using type = float4; };
template <> struct V4<double> { using type = double4; };

// ver7/GSimulation.cpp:126-127; the fp64 variant widens the float literals.
template <typename T> __host__ __device__ constexpr T softening2() { return (T)1.e-3f; }
template <typename T> __host__ __device__ constexpr T grav_const() { return (T)6.67259e-11f; }

// c/sqrt(x) with c = rsq_scale<T>().  fp32: the raw v_rsq_f32, c = 1 (<= 1 ulp; r2 >= 1e-3 so no
// denormal/zero handling is needed -- the ocml rsqrtf wrapper would add scaling code per pair).
// fp64: v_rsq_f64 is a ~2^-26 seed (measured 1.2e-8 on the accelerations); ONE Newton step
// y' = y/2 * (3 - x*y*y) takes it to 3/2 e^2 of the seed's error e (measured 4.6e-15 on accelerations, 2.8e-15 on a
// 500-step kenergy trace; the potential of nbx_diag uses it, the pair term has gm_inv_cube below).  The step's factor
// 1/2 is not applied here: the
// function returns 2/sqrt(x) and the records carry G*m/8 instead (exact power-of-two scaling,
// gm_prescale<double>()), which saves one multiply per pair: 3 VALU for the step instead of 4.
template <typename T> __host__ __device__ constexpr T gm_prescale() { return sizeof(T) == 8 ? (T)0.125 : (T)1; }
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ double rsq(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double t = x * y;
  const double u = __builtin_fma(-t, y, 3.0);
  return y * u;
}

// gmj * r2^-3/2 with gmj the record's .w (G*m_j * gm_prescale<T>()).  fp32: (gmj * inv) * inv^2 with the raw v_rsq_f32.
// fp64: the Newton step of rsq() above leaves 3/2 e^2 of the seed's error e on 1/sqrt, three times that on the cube -- and e
// reaches 2^-25 at some arguments, i.e. up to 40 units of 2^-53 on a pair term (tests/test_step_probe_gpu.py saw exactly that on
// bodies whose acceleration is one dominant term).  So the cube is corrected directly, to second order in the seed's residual
// h = 1 - x y^2 = 1 - (1 + e)^2:  x^-3/2 = y^3 (1 - h)^-3/2 = y^3 (1 + 3/2 h + 15/8 h^2 + O(h^3)), h^3 < 2^-70.  y^2 serves both
// the residual and the cube, the x8 of the prescale is folded into the polynomial: 7 VALU where the Newton form took 6, and
// about 5 units of rounding whatever the seed does.
__device__ __forceinline__ float gm_inv_cube(float gmj, float r2) {
  const float inv = rsq(r2);
  const float inv2 = inv * inv;
  return (gmj * inv) * inv2;
}
__device__ __forceinline__ double gm_inv_cube(double gmj, double r2) {
  const double y = __builtin_amdgcn_rsq(r2);
  const double y2 = y * y;
  const double h = __builtin_fma(-r2, y2, 1.0);
  const double q = __builtin_fma(h, __builtin_fma(h, 15.0, 12.0), 8.0);  // 8 (1 + 3/2 h + 15/8 h^2)
  return ((gmj * y) * y2) * q;
}

__device__ __forceinline__ float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }

// One pair: 3 sub, 3 FMA (r^2 + eps^2), 1 rsq, 3 mul (G*m_j * inv^3; fp64: 7, gm_inv_cube), 3 FMA (accumulate)
// = 12 VALU + 1 transcendental = the 20 "algorithmic" flops of DESIGN.md.
// gmj is the record's .w = G*m_j * gm_prescale<T>().
template <typename T>
__device__ __forceinline__ void pair(T xj, T yj, T zj, T gmj, T xi, T yi, T zi, T& ax, T& ay, T& az) {
  const T dx = xj - xi, dy = yj - yi, dz = zj - zi;
  const T r2 = fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())));
  const T s = gm_inv_cube(gmj, r2);
  ax = fmaT(dx, s, ax);
  ay = fmaT(dy, s, ay);
  az = fmaT(dz, s, az);
}

// Two i-bodies per call on the packed-fp32 pipe (v_pk_add/mul/fma_f32): the j record is a
// scalar splat (op_sel), the i-bodies live in even-aligned register pairs.  12 packed VALU +
// 2 v_rsq_f32 per TWO pairs.  A/B'd against the scalar form in tools/kbench.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pair2(float xj, float yj, float zj, float gmj, f32x2 xi, f32x2 yi, f32x2 zi,
                                      f32x2& ax, f32x2& ay, f32x2& az) {
  const f32x2 dx = f32x2{xj, xj} - xi, dy = f32x2{yj, yj} - yi, dz = f32x2{zj, zj} - zi;
  const f32x2 e2 = {softening2<float>(), softening2<float>()};
  f32x2 r2 = __builtin_elementwise_fma(dz, dz, e2);
  r2 = __builtin_elementwise_fma(dy, dy, r2);
  r2 = __builtin_elementwise_fma(dx, dx, r2);
  f32x2 inv;
  inv.x = __builtin_amdgcn_rsqf(r2.x);
  inv.y = __builtin_amdgcn_rsqf(r2.y);
  const f32x2 inv2 = inv * inv;
  const f32x2 s = (f32x2{gmj, gmj} * inv) * inv2;
  ax = __builtin_elementwise_fma(dx, s, ax);
  ay = __builtin_elementwise_fma(dy, s, ay);
  az = __builtin_elementwise_fma(dz, s, az);
}

// pair2() twice, with the two instruction streams interleaved and pinned: (record a on bodies A) and (record b on bodies
// B), instruction k of the one followed by instruction k of the other, a scheduling barrier after each such couple.  Every
// result is consumed two or more instructions after it is produced, which is what the gfx940-family VALU needs (one wait
// state after a transcendental or packed result) -- hipcc left to itself schedules one 14-instruction chain at a time and
// pads it with ~1.4 s_nop per pair2 (15 % of the issue slots of the jlane loop).  Operations, association and, per
// accumulator, the order of additions are exactly pair2's.  SAME_ACC: A and B are the same bodies and share accumulators
// (two j records on one body pair): record a's terms are added before record b's.
template <bool SAME_ACC>
__device__ __forceinline__ void pair2_x2(float xa, float ya, float za, float gma, f32x2 xiA, f32x2 yiA, f32x2 ziA, f32x2& axA,
                                         f32x2& ayA, f32x2& azA, float xb, float yb, float zb, float gmb, f32x2 xiB, f32x2 yiB,
                                         f32x2 ziB, f32x2& axB, f32x2& ayB, f32x2& azB) {
#define NBX_PIN() __builtin_amdgcn_sched_barrier(0)
  const f32x2 e2 = {softening2<float>(), softening2<float>()};
  const f32x2 dxa = f32x2{xa, xa} - xiA, dxb = f32x2{xb, xb} - xiB; NBX_PIN();
  const f32x2 dya = f32x2{ya, ya} - yiA, dyb = f32x2{yb, yb} - yiB; NBX_PIN();
  const f32x2 dza = f32x2{za, za} - ziA, dzb = f32x2{zb, zb} - ziB; NBX_PIN();
  f32x2 ra = __builtin_elementwise_fma(dza, dza, e2), rb = __builtin_elementwise_fma(dzb, dzb, e2); NBX_PIN();
  ra = __builtin_elementwise_fma(dya, dya, ra); rb = __builtin_elementwise_fma(dyb, dyb, rb); NBX_PIN();
  ra = __builtin_elementwise_fma(dxa, dxa, ra); rb = __builtin_elementwise_fma(dxb, dxb, rb); NBX_PIN();
  f32x2 ia, ib;
  ia.x = __builtin_amdgcn_rsqf(ra.x); ib.x = __builtin_amdgcn_rsqf(rb.x); NBX_PIN();
  ia.y = __builtin_amdgcn_rsqf(ra.y); ib.y = __builtin_amdgcn_rsqf(rb.y); NBX_PIN();
  const f32x2 qa = ia * ia, qb = ib * ib; NBX_PIN();
  f32x2 sa = f32x2{gma, gma} * ia, sb = f32x2{gmb, gmb} * ib; NBX_PIN();
  sa = sa * qa; sb = sb * qb; NBX_PIN();
  if constexpr (SAME_ACC) {  // one set of accumulators: a's three updates, then b's (each waits three instructions for its input)
    axA = __builtin_elementwise_fma(dxa, sa, axA); ayA = __builtin_elementwise_fma(dya, sa, ayA); NBX_PIN();
    azA = __builtin_elementwise_fma(dza, sa, azA); axA = __builtin_elementwise_fma(dxb, sb, axA); NBX_PIN();
    ayA = __builtin_elementwise_fma(dyb, sb, ayA); azA = __builtin_elementwise_fma(dzb, sb, azA); NBX_PIN();
  } else {
    axA = __builtin_elementwise_fma(dxa, sa, axA); axB = __builtin_elementwise_fma(dxb, sb, axB); NBX_PIN();
    ayA = __builtin_elementwise_fma(dya, sa, ayA); ayB = __builtin_elementwise_fma(dyb, sb, ayB); NBX_PIN();
    azA = __builtin_elementwise_fma(dza, sa, azA); azB = __builtin_elementwise_fma(dzb, sb, azB); NBX_PIN();
  }
#undef NBX_PIN
}

// Separately rounded multiply and add, so the O(n) update rounds exactly like the reference's x86-64 baseline
// build (no FMA instruction there).  HIP's __fmul_rn / __fadd_rn are plain `*` / `+` and hipcc's
// default -ffp-contract=fast fuses them (seen in the ISA, caught by the NBX_KERNEL_EXACT bit-equality tests), hence
// the pragma: it clears the contract flag on exactly these operations and survives inlining.
template <typename T> __device__ __forceinline__ T mul_rn(T a, T b) {
#pragma clang fp contract(off)
  return a * b;
}
template <typename T> __device__ __forceinline__ T add_rn(T a, T b) {
#pragma clang fp contract(off)
  return a + b;
}

// Sum of one double per thread over the 256-thread workgroup, fixed order: wave64 shuffle tree,
// then the four wave sums through LDS.  Result valid in thread 0.
__device__ __forceinline__ double block_sum(double v, double* lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds4[wave] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) r = ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
  return r;
}

// ver7/GSimulation.cpp:181-197 for one body; returns m*(vx^2+vy^2+vz^2) (the reference's term,
// evaluated in T with the reference's association).
template <typename T>
__device__ __forceinline__ T euler_update(T ax, T ay, T az, T dt, typename V4<T>::type& p,
                                          typename V4<T>::type& v) {
  v.x = add_rn(v.x, mul_rn(ax, dt));
  v.y = add_rn(v.y, mul_rn(ay, dt));
  v.z = add_rn(v.z, mul_rn(az, dt));
  p.x = add_rn(p.x, mul_rn(v.x, dt));
  p.y = add_rn(p.y, mul_rn(v.y, dt));
  p.z = add_rn(p.z, mul_rn(v.z, dt));
  const T v2 = add_rn(add_rn(mul_rn(v.x, v.x), mul_rn(v.y, v.y)), mul_rn(v.z, v.z));
  return mul_rn(v.w, v2);
}

// The velocity half of euler_update alone (include/nbx_kick.h): v += a*h with the same separately rounded operations, the
// position untouched; returns the same term, m*(vx^2+vy^2+vz^2), of the kicked velocity.
template <typename T>
__device__ __forceinline__ T kick_update(T ax, T ay, T az, T h, typename V4<T>::type& v) {
  v.x = add_rn(v.x, mul_rn(ax, h));
  v.y = add_rn(v.y, mul_rn(ay, h));
  v.z = add_rn(v.z, mul_rn(az, h));
  const T v2 = add_rn(add_rn(mul_rn(v.x, v.x), mul_rn(v.y, v.y)), mul_rn(v.z, v.z));
  return mul_rn(v.w, v2);
}

}  // namespace nbx
