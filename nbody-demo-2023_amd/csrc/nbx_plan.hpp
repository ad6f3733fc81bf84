// nbx_plan.hpp -- which force kernel a context runs and with what launch shape: the policy of nbx_create, host-only.
// Standard library, include/nbx.h and nbx_diag_shape.hpp (which includes nothing) only: no HIP call, no environment, no nbx_ctx, so that g++ compiles it without ROCm
// (tests/test_launch_plan.py drives it with every nbx_opts).  kInstances is the one list of compiled force-kernel instances:
// nbx_api.hip instantiates exactly those and launches the ones plan_launch names.  plan_ensemble and plan_ragged (below) are
// the policies of nbx_ensemble_create and nbx_ragged_create, over kEnsembleInstances; plan_ragged_diag is the work list of
// nbx_ragged_diagnostics.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../../include/nbx.h"
#include "nbx_diag_shape.hpp"  // diag_splits: the shape rule of the diagnostics, read by plan_ragged_diag (host-only as well)

namespace nbx_detail {
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
}  // namespace nbx_detail

namespace nbx {
using nbx_detail::ceil_div;
using nbx_detail::round_up;

constexpr int kBlock = 256;  // threads per workgroup
constexpr int kTile = 256;   // j records per LDS tile (BASELINE.json configs[1]: "LDS j-tile=256")
// j-range granule of the plain SGPR kernel: whole trips of every hand-scheduled loop (nbx_api.hip checks it against kSgprAsmTrip<>)
constexpr int kSgprGran = 256;
// spare records behind posm[n_alloc), zero-filled: the pipelined scalar loop requests one batch (16 records at most) past
// the end, the jlane kernel one trip of its widest prefetch (8 blocks of 64 records); nothing read there is ever applied
// (here and not with the kernels: plan_ensemble bounds the record index of an ensemble, whose members each carry the spare records)
constexpr int kSgprOverread = 16 + 8 * 64;

enum : int { JSRC_LDS = 1, JSRC_SGPR = 2 };
enum : int { MATH_SCALAR = 0, MATH_PACKED = 1 };
// How the SGPR kernel's j loop is scheduled: LOOP_CXX = hipcc schedules force_kernel's C++ loop; LOOP_ASM = the hand-scheduled
// gfx950 loop of nbx_sgpr_loop.inc (packed fp32, B = 2 or 4, no wave split): same operations in the same order, hence
// the same bits (tests compare the two), but no s_mov splats, one pointer update per trip and 8-byte aligned VOP3P code:
// worth 13 % when a SIMD holds a single wave, where every scalar instruction costs a full 4-cycle issue slot.
// With ONE body per lane LOOP_ASM is the two-j-records-per-packed-operation loop (sgpr_loop_asm_jpair): slices that leave less than
// one wave per SIMD at two bodies per lane (<= 65536 owned bodies) get twice the waves at 76 cycles per two pairs instead of 2 x 56;
// it reads the pair-interleaved copy of the records that pair_transpose_kernel rebuilds every step.
// LOOP_ASM_TS = the same loop with time-sliced wave priority, for shapes that put two waves on a SIMD for the whole launch
// (reference order, grid.y == 1, 257..512 workgroups on 256 CUs): this chip issues the waves of a SIMD in strict age order,
// so without it they run one after the other -- the older one leaves the loop at 0.50 of the kernel time -- and the younger
// one has nobody to fill its issue bubbles (tools/wave_fair.hip).  +4.5 % at n = 262144; nothing to gain
// with one wave per SIMD (-0.6 %: the six scalar instructions) or with three and more (profiles/r02_time_sliced_ab.txt).
// LOOP_ASM_PF = the same loop plus one L2-prefetch load per trip, for launches that leave ONE wave per SIMD (grid.x <= CUs, e.g. a rank
// that owns 131072 of 1M bodies): there the arithmetic of one ring group (512 cycles) is all the cover a scalar load gets, every wave of
// an XCD asks for the same line at about the same time, and what they all wait for is the first requester's Infinity-Cache round trip
// (~545 cycles).  +3.5 % at one wave per SIMD, -0.4 ... -1.4 % with two or more (profiles/r04_b2_prefetch_ab.txt).
enum : int { LOOP_CXX = 0, LOOP_ASM = 1, LOOP_ASM_TS = 2, LOOP_ASM_PF = 3 };
// What a workgroup does with its accelerations:
//   EPI_SLAB  write them to its split's slab (the separate integrate_kernel, or nbx_accel, consumes the slabs)
//   EPI_ROW   single split (gridDim.y == 1): integrate its bodies directly, no slab
// (Round 1 also had a "last arriver integrates" epilogue for split shapes -- agent-scope release / ticket / acquire.  It was
// bit-equal but slower than the extra launch at every size, and force_jlane_kernel now gives launch-bound sizes
// their single launch per step without any inter-workgroup hand-off; it was removed.)
enum : int { EPI_SLAB = 0, EPI_ROW = 1 };

// NBX_ORDER_AUTO: fp32 sums of more terms than this use the reference's order.  131072 x 500 steps agrees with the
// reference to 2e-5 in tree order (profiles/r01_validate_orders_n131072_s500.log); 262144 x 200 does not (1.3e-3).
constexpr int kTreeOrderMaxN = 131072;
// NBX_KERNEL_AUTO, tree order: contexts that own at most this many bodies step with ONE launch (force_jlane_kernel)
// (12288: 41 us against SGPRW's 48.  Round 3, profiles/r03_band_sweep.txt: between 12288 and 16384 the wave-split kernel falls back
// to two bodies per lane and, at sizes whose splits are not whole tiles, to the compiled loop -- 40-45 % -- while the one-launch kernel
// with 8 bodies per wave is 6-15 % ahead: 13000 50.3 vs 53.2 us, 15000 58.0 vs 65.6, 16000 62.8 vs 72.3.)  16384 ITSELF is excluded:
// there the two tie within 2 %, and SGPRW's summation tree (S = 32) is the one whose chaotic n = 16384 x 500 run -- BASELINE
// configs[1] -- stays inside the 1e-4 gate at every printed step (profiles/r02_config1_by_kernel.txt, r03_config1_by_shape.txt).
constexpr int kJlaneMaxOwn = 16383;
// Tree order, wave-split kernel: contexts that own up to this many bodies keep round 1's split rule (S = 32 at 16384).  Fewer
// splits are 5 % faster there (profiles/r03_band_sweep.txt: S = 4 or 8), but BASELINE.json configs[1] -- n = 16384 x 500 steps, 450 of
// them after the bounce -- is decided at the reference's own noise level, and of S = 2, 4, 8, 16, 32 only the tree of S = 32
// lands inside 1e-4 at every printed row (7.7e-5; the others 1.05e-4 ... 1.43e-4, two builds of the reference itself 1.3e-4:
// profiles/r03_config1_by_shape.txt).  tests/test_parity_gpu.py::test_config1_launch_shape_is_frozen pins it.
constexpr int kRound1SplitMaxOwn = 16384;
constexpr int kJlaneMaxOwnF64 = 12288;  // fp64 form: 92 us against 97 at 12288, SGPRW ahead at 16384 (profiles/r02_jlane_f64_ab.txt)

// One compiled force-kernel instance: its template arguments.  INST_FORCE = force_kernel<T, B, jsrc, epi, 1, math, ws, loop>;
// INST_JLANE = force_jlane_kernel<B, D, loop> (fp32) or force_jlane_kernel_f64<B, D> (B = bodies per wave); INST_EXACT =
// force_exact_kernel<T, B == 1> (B = 1: FMA contraction, NBX_KERNEL_EXACT_FMA).  Fields a kernel does not take are 0.
enum : int { INST_FORCE = 0, INST_JLANE = 1, INST_EXACT = 2 };
struct Instance {
  int kind, precision, B, jsrc, epi, math;
  bool ws;
  int loop;
};
constexpr bool operator==(const Instance& a, const Instance& b) {
  return a.kind == b.kind && a.precision == b.precision && a.B == b.B && a.jsrc == b.jsrc && a.epi == b.epi && a.math == b.math &&
         a.ws == b.ws && a.loop == b.loop;
}
namespace instance_list {  // {kind, precision, B, jsrc, epi, math, ws, loop}
constexpr int F = INST_FORCE, J = INST_JLANE, X = INST_EXACT, S_ = JSRC_SGPR, L_ = JSRC_LDS, R_ = EPI_ROW, Z_ = EPI_SLAB, SC = MATH_SCALAR,
              PK = MATH_PACKED, CXX = LOOP_CXX, ASM = LOOP_ASM, TS = LOOP_ASM_TS, PF = LOOP_ASM_PF;
constexpr Instance kInstances[] = {
    // compiled loop: fp32 one body per lane, fp64 1, 2 and 4 (scalar math); fp32 2, 4 and (no wave split) 8 on the packed pipe
    {F, 32, 1, S_, Z_, SC, true, CXX}, {F, 32, 1, S_, R_, SC, false, CXX}, {F, 32, 1, S_, Z_, SC, false, CXX}, {F, 32, 1, L_, R_, SC, false, CXX}, {F, 32, 1, L_, Z_, SC, false, CXX},
    {F, 64, 1, S_, Z_, SC, true, CXX}, {F, 64, 1, S_, R_, SC, false, CXX}, {F, 64, 1, S_, Z_, SC, false, CXX}, {F, 64, 1, L_, R_, SC, false, CXX}, {F, 64, 1, L_, Z_, SC, false, CXX},
    {F, 64, 2, S_, Z_, SC, true, CXX}, {F, 64, 2, S_, R_, SC, false, CXX}, {F, 64, 2, S_, Z_, SC, false, CXX}, {F, 64, 2, L_, R_, SC, false, CXX}, {F, 64, 2, L_, Z_, SC, false, CXX},
    {F, 64, 4, S_, Z_, SC, true, CXX}, {F, 64, 4, S_, R_, SC, false, CXX}, {F, 64, 4, S_, Z_, SC, false, CXX}, {F, 64, 4, L_, R_, SC, false, CXX}, {F, 64, 4, L_, Z_, SC, false, CXX},
    {F, 32, 2, S_, Z_, PK, true, CXX}, {F, 32, 2, S_, R_, PK, false, CXX}, {F, 32, 2, S_, Z_, PK, false, CXX}, {F, 32, 2, L_, R_, PK, false, CXX}, {F, 32, 2, L_, Z_, PK, false, CXX},
    {F, 32, 4, S_, Z_, PK, true, CXX}, {F, 32, 4, S_, R_, PK, false, CXX}, {F, 32, 4, S_, Z_, PK, false, CXX}, {F, 32, 4, L_, R_, PK, false, CXX}, {F, 32, 4, L_, Z_, PK, false, CXX},
    {F, 32, 8, S_, R_, PK, false, CXX}, {F, 32, 8, S_, Z_, PK, false, CXX}, {F, 32, 8, L_, R_, PK, false, CXX}, {F, 32, 8, L_, Z_, PK, false, CXX},
    // hand-scheduled loops (fp32, SGPR source): two j records per operation for one body per lane, 2 and 4 bodies per lane with and
    // without the wave split; time-sliced priority and L2 prefetch for the single-row kernel
    {F, 32, 1, S_, R_, SC, false, ASM}, {F, 32, 1, S_, Z_, SC, false, ASM},
    {F, 32, 2, S_, Z_, PK, true, ASM}, {F, 32, 2, S_, R_, PK, false, ASM}, {F, 32, 2, S_, Z_, PK, false, ASM},
    {F, 32, 4, S_, Z_, PK, true, ASM}, {F, 32, 4, S_, R_, PK, false, ASM}, {F, 32, 4, S_, Z_, PK, false, ASM},
    {F, 32, 2, S_, R_, PK, false, TS}, {F, 32, 4, S_, R_, PK, false, TS}, {F, 32, 2, S_, R_, PK, false, PF}, {F, 32, 4, S_, R_, PK, false, PF},
    // one launch per step: fp32 2, 4, 8 (generated loop or compiled) and 16 bodies per wave, fp64 2, 4, 8
    {J, 32, 2, 0, 0, 0, false, ASM}, {J, 32, 2, 0, 0, 0, false, CXX}, {J, 32, 4, 0, 0, 0, false, ASM}, {J, 32, 4, 0, 0, 0, false, CXX},
    {J, 32, 8, 0, 0, 0, false, ASM}, {J, 32, 8, 0, 0, 0, false, CXX}, {J, 32, 16, 0, 0, 0, false, CXX},
    {J, 64, 2, 0, 0, 0, false, CXX}, {J, 64, 4, 0, 0, 0, false, CXX}, {J, 64, 8, 0, 0, 0, false, CXX},
    // the reference's arithmetic (validation)
    {X, 32, 0, 0, 0, 0, false, CXX}, {X, 32, 1, 0, 0, 0, false, CXX}, {X, 64, 0, 0, 0, 0, false, CXX}, {X, 64, 1, 0, 0, 0, false, CXX},
};
}  // namespace instance_list
using instance_list::kInstances;
constexpr int kInstanceCount = (int)(sizeof(kInstances) / sizeof(kInstances[0]));
// position of k in kInstances, -1 if it is not compiled
constexpr int instance_index(const Instance& k) {
  for (int i = 0; i < kInstanceCount; ++i)
    if (kInstances[i] == k) return i;
  return -1;
}

// A context's launch plan (nbx_create; nbx_stats reports it).
struct Plan {
  int variant = NBX_KERNEL_LDS, order = NBX_ORDER_TREE;
  int B = 1, S = 1, jps = 0;  // bodies per lane (per wave: JLANE), j-splits, j records per split
  int math = MATH_SCALAR, epi = EPI_SLAB, loop = LOOP_CXX;
  int grid_x = 0, grid_y = 1;
  bool use_graph = false;  // nbx_step replays multi-step windows from a hipGraph
  bool pairs = false;      // one body per lane + hand-scheduled loop: the pair-interleaved copy of the records is rebuilt every step
  Instance step{}, accel{};  // the step kernel, and nbx_accel's form of it (accelerations into the slabs, nothing integrated)
};

// The instance a plan launches with inner loop `loop`.  nbx_accel's slab form of a single-row context: the plain hand-scheduled loop.
inline Instance plan_instance(const Plan& p, int precision, bool accel, int loop) {
  if (p.variant == NBX_KERNEL_EXACT || p.variant == NBX_KERNEL_EXACT_FMA)
    return {INST_EXACT, precision, p.variant == NBX_KERNEL_EXACT_FMA ? 1 : 0, 0, 0, 0, false, loop};
  if (p.variant == NBX_KERNEL_JLANE) return {INST_JLANE, precision, p.B, 0, 0, 0, false, loop};
  if (accel && (loop == LOOP_ASM_TS || loop == LOOP_ASM_PF)) loop = LOOP_ASM;
  return {INST_FORCE, precision, p.B, p.variant == NBX_KERNEL_LDS ? JSRC_LDS : JSRC_SGPR, accel ? EPI_SLAB : p.epi, p.math,
          p.variant == NBX_KERNEL_SGPRW, loop};
}

// Bodies per lane of the reference-order kernel (one chain per owned body, S = 1).  Its run time is quantised: the
// ceil(own / (256 B)) workgroups are spread over the CUs, and a launch takes as long as the fullest CU, which holds
// r = ceil(workgroups / CUs) of them.  Measured on MI355X at n = 1048576 with the hand-scheduled loop for B = 2 and 4
// (profiles/r02_reference_order_thresholds.txt), ms for r = 1, 2, 3, ...: B = 1, compiled loop: 31.0, 48.6, 70.3, 91, 112 (plain VALU ops);
// B = 2: 31.5 (30.0 with the L2 prefetch and the 256-record trips of LOOP_ASM_PF, round 4), 59.6, 88.5, 118;  B = 4: 59.3, 117.4, 175.6, 234.6 -- linear in r after
// the first workgroup.  With two workgroups on the fullest CU the time-sliced loop applies (LOOP_ASM_TS): B = 2, r = 2 then costs 58.0
// (profiles/r02_time_sliced_ab.txt: 57.98 ms for 262144 of 1M bodies), B = 4, r = 2 117.0.  Round 4: one body per lane with the
// two-j-records-per-operation loop (sgpr_loop_asm_jpair, `jpair`): 17.9 for r = 1 (65536 of 1M bodies: 48.8 % of the roofline against 28.4 %
// for the compiled loop and 27.8 % for B = 2 on half the CUs), 34.3 for r = 2 (profiles/r04_jpair_ab.txt) -- so it takes every slice of up to
// 256 x CUs = 65536 bodies, and B = 2 keeps 65537 ... 131072.  Pick the B with the smallest estimate; ties go to the larger B (fewer
// workgroups stream the j records).  Only the ratios matter, so the table serves every n.
inline int reference_order_bodies_per_lane(int own, int cus, int max_b, bool jpair, double* cost_out = nullptr) {
  struct Cost { int b; double first, next, two; };
  static const Cost kCost[] = {{1, 31.0, 20.2, 0.0}, {2, 30.0, 29.25, 58.0}, {4, 59.8, 58.2, 117.0}};
  static const Cost kJpair = {1, 17.9, 16.4, 0.0};  // one body per lane, two j records per packed operation
  int best = 1;
  double best_t = 0.0;
  for (const auto& k0 : kCost) {
    const auto& k = (k0.b == 1 && jpair) ? kJpair : k0;
    if (k.b > max_b) continue;
    const int wgs = ceil_div(own, kBlock * k.b);
    const int r = std::max(1, ceil_div(wgs, std::max(1, cus)));
    const double t = (r == 2 && k.two > 0.0) ? k.two : k.first + k.next * (r - 1);
    if (best_t == 0.0 || t <= best_t * 1.01) { best = k.b; best_t = std::min(t, best_t == 0.0 ? t : best_t); }
  }
  // Where two bodies per lane load every CU evenly too (twice the workgroups, all CUs with the same count), they win over four
  // by 2.5 % at 262144 owned bodies and tie from 524288 up (the younger wave of a SIMD fills the older one's issue bubbles;
  // profiles/r02_loop_ab_asm_vs_cxx.txt, same process on two boxes): take them.
  if (best == 4 && max_b >= 2 && ceil_div(own, kBlock * 2) % std::max(1, cus) == 0) best = 2;
  if (cost_out) *cost_out = best_t;
  return best;
}

// What one force launch of this plan would cost, in relative units, if the context owned `own` bodies instead: the cost table of
// reference_order_bodies_per_lane in reference order (a step function of `own`: the launch lasts as long as its fullest CU), and `own`
// itself in tree order, where j-splits keep the time close to proportional.  The tuner of nbx_group_retune uses the RATIO of two such
// values to predict what a move of the shares would do before it makes it (nbx_detail::model_force_cost).
inline double force_cost(const Plan& p, int precision, int cus, int own) {
  if (own <= 0) return 0.0;
  if (p.order != NBX_ORDER_REFERENCE) return (double)own;
  const bool jpair = precision == 32 && p.variant == NBX_KERNEL_SGPR;
  double t = 0.0;
  (void)reference_order_bodies_per_lane(own, cus > 0 ? cus : 256, precision == 32 ? 8 : 4, jpair, &t);
  return t;
}

// j-splits of the wave-split kernel with the hand-scheduled loop (round 3, profiles/r03_band_sweep.txt).  Round 1's rule -- 32
// workgroups per CU, i.e. S = 32 up to n = 65536 -- suited the compiler-scheduled loop, which needed eight waves per SIMD to
// hide its own bubbles.  The hand-scheduled loop is at its rate with two, and every extra split costs a slab write, a slab
// read by integrate_kernel and a shorter j loop per wave.  The launch lasts as long as the fullest CU: ceil(bi S / CUs)
// workgroups of 1/S of the j range each.  Take the S (power of two) that minimises that product; among equals the smallest
// S that still gives every CU two workgroups.  Measured optimum at every size tried: 24576 -> 8 (+2.6 % over S = 32),
// 32768 -> 4 (+1.9 %), 49152 -> 4 (+1.2 %), 65536 -> 2 (+1.2 %); three workgroups on half the CUs (24576 with S = 4) is 20 % slower.
inline int balanced_j_split(int bi, int cus, int max_s) {
  double best_cost = 0.0;
  for (int S = 1; S <= max_s; S *= 2) {
    const double cost = (double)ceil_div(bi * S, cus) / S;
    if (best_cost == 0.0 || cost < best_cost) best_cost = cost;
  }
  int pick = 0, largest = 1;
  for (int S = 1; S <= max_s; S *= 2) {
    if ((double)ceil_div(bi * S, cus) / S > best_cost * 1.0001) continue;
    largest = S;
    if (!pick && bi * S >= 2 * cus) pick = S;
  }
  return pick ? pick : largest;
}

// Bodies per wave of the one-launch kernel (force_jlane_kernel; ensemble_step_kernel with `members` systems of `own` bodies in one
// launch).  A launch lasts as long as the fullest SIMD: ceil(waves / SIMDs) rounds of NB bodies each, times what a body-round costs
// with that NB; the waves of all members count, each member having ceil(own / NB) of its own.  Measured per body-round and per j
// record, relative to NB = 8 (profiles/r03_jlane_band.txt: the same ratios at 12288, 13000 and 16383 bodies): 2 bodies per wave 1.29
// (every wave streams all j records and transposes through LDS for two bodies only), 4 -> 1.06, 8 -> 1.00 (the generated loop),
// 16 -> 1.06 (compiled loop only).  Smallest product wins, ties to the larger NB.  One system: 2048 -> 2, 4096 -> 4, 8192 -> 8,
// 12288 -> 4 (three full rounds), 13000 ... 16383 -> 8 -- the measured optimum at each.  Round 2 counted body-rounds alone, which
// sent 13000 and 14336 to NB = 2 (56.6 us against 50.1 with 8).
// fp64 (no generated loop, other ratios not measured): body-rounds alone, ties to the larger NB, as in round 2.
// Ensembles (members > 1; profiles/ensemble_sweep.json, which records the time of every NB next to the one taken here): where 16
// bodies per wave still give every SIMD a wave, they beat 8 at every cell measured -- 0.92 of its time at n = 2048 x 16 members,
// 0.95 at 2048 x 64, 0.97-0.98 at 4096 x 4 / 16 / 64, 0.98-0.99 at 8192 x 4 / 16 / 64: a wave's fixed cost (64 LDS reads per body column,
// the epilogue) is spread over twice the bodies and half as many waves stream a member's j records, which weighs most where the j
// loop is short -- so their weight there is 0.97.  With fewer waves than SIMDs 16 lose as the table says (2048 x 4: 1.41 of 8's
// time), and a lone system keeps the table it was measured with (16383 bodies: 8 per wave).
// (`waves_of(nb)` = the launch's waves with nb bodies each: members x ceil(own / nb) for a context or an ensemble, the sum of
// ceil(n_k / nb) over the members of a ragged ensemble -- one rule for all three)
template <typename WavesOf>
inline int jlane_bodies_per_wave_of(WavesOf&& waves_of, int members, int precision, int cus, int max_nb = 16) {
  max_nb = std::min(max_nb, precision == 32 ? 16 : 8);  // fp64 bodies take two SGPRs per coordinate
  int NB = 2;
  long long best = 0;
  for (int nb = 2; nb <= max_nb; nb *= 2) {
    const long long waves = waves_of(nb), simds = (long long)cus * 4;
    long long weight = precision != 32 ? 100 : (nb == 2 ? 129 : nb == 8 ? 100 : 106);
    if (precision == 32 && nb == 16 && members > 1 && waves >= simds) weight = 97;
    const long long cost = ((waves + simds - 1) / simds) * nb * weight;
    if (best == 0 || cost <= best) { best = cost; NB = nb; }
  }
  return NB;
}
inline int jlane_bodies_per_wave(int own, int members, int precision, int cus, int max_nb = 16) {
  return jlane_bodies_per_wave_of([=](int nb) { return (long long)members * ceil_div(own, nb); }, members, precision, cus, max_nb);
}
// NBX_LOOP_AUTO, jlane kernel with a generated loop for its NB: the generated loop keeps four records per set in flight; with few
// bodies per wave that is too little arithmetic to cover an L2 round trip when a SIMD holds a single wave, and the compiled loop
// (eight records per set) is 3-4 % ahead there (profiles/r02_jlane_ab.txt).  Auto takes the generated loop where it measured
// faster: 8 bodies per wave, or 4 with more than one wave per SIMD.  `waves` = the launch's (all members of an ensemble).
inline bool jlane_auto_takes_generated_loop(int NB, long long waves, int cus) { return NB == 8 || (NB == 4 && waves > (long long)cus * 4); }
// prefetch depth D of the compiled loop / tail: records per register set (the generated loop exists for NB <= 8)
constexpr int jlane_depth(int precision, int NB) { return precision == 32 ? (NB <= 4 ? 8 : 4) : (NB == 2 ? 8 : 4); }

// What the shape rules read: the context as nbx_create resolved it (n_alloc rounded to the tile, i_count of a whole run = n), the
// device's CU count (<= 0: taken as 256) and whether the context owns its stream (a caller's stream is not captured for replay).
struct PlanInput { int n, n_alloc, i_count, precision, cus; bool own_stream; };

// Launch shape.  Measured with tools/kbench on MI355X (profiles/r01_kbench_*): the force kernel is
// VALU-issue bound and wants all 8 wave slots of every SIMD filled, i.e. >= 8192 workgroups of 256
// threads (32 per CU).  Fastest shape from n = 2k to 1M: j records in SGPRs, the four waves of a
// workgroup sharing 64*B bodies and splitting the j range (NBX_KERNEL_SGPRW), B = 4 bodies per lane
// (two packed register pairs; B = 2 for short i ranges), plus S j-range splits across workgroups:
// 58-60 % of the fp32 roofline at n >= 64k, 52 % at 16k, vs 52 % / 36 % for B = 8 / LDS tile.
inline void auto_shape(Plan* c, const PlanInput& in, const nbx_opts& o) {
  const int cus = in.cus > 0 ? in.cus : 256;
  const int target_wgs = cus * 32;
  int variant = o.kernel_variant;
  if (variant == NBX_KERNEL_EXACT || variant == NBX_KERNEL_EXACT_FMA) {  // one thread per body, no blocking, no splits, separate integrate kernel
    c->B = 1; c->S = 1; c->jps = in.n_alloc; c->math = MATH_SCALAR; c->variant = variant; c->epi = EPI_SLAB;
    c->order = NBX_ORDER_REFERENCE;  // one accumulator per body, j ascending: it IS the reference's loop
    c->grid_x = ceil_div(in.i_count, kBlock); c->grid_y = 1;
    return;
  }
  // Summation order (include/nbx.h).  The reference adds a body's n terms one after the other into one fp32
  // accumulator; from n = 262144 that sum carries ~1e-5 of rounding noise per step which heats the system (kenergy
  // +5e-4..1e-3 against an fp64 run; 1.6e-5 over 500 steps at n = 131072).  A tree of partial sums does not reproduce
  // that, a single accumulator per body in the same j order does (to 5e-5 / 5e-7, tools/validate_big.py) -- at the
  // price of one chain per owned body.  The noise is a property of the LENGTH of the sum, i.e. of n, not of how many
  // bodies this context owns: every rank of a sharded run takes the same decision.
  int order = o.summation_order;
  if (order != NBX_ORDER_REFERENCE && order != NBX_ORDER_TREE) {
    const bool shape_given = o.j_split > 0 || variant == NBX_KERNEL_SGPRW || variant == NBX_KERNEL_JLANE;  // tree-only shapes
    if (o.j_split == 1 && variant != NBX_KERNEL_SGPRW) order = NBX_ORDER_REFERENCE;
    // fp64 keeps the tree: its summation noise (~1e-13) is far below the 1e-10 fp64 gate in either order
    else order = (!shape_given && in.precision == 32 && in.n > kTreeOrderMaxN) ? NBX_ORDER_REFERENCE : NBX_ORDER_TREE;
  }
  c->order = order;
  if (order == NBX_ORDER_REFERENCE) {
    if (variant != NBX_KERNEL_LDS && variant != NBX_KERNEL_SGPR) variant = NBX_KERNEL_SGPR;
    int B = o.bodies_per_lane;
    const int maxBr = in.precision == 32 ? 8 : 4;
    if (B != 1 && B != 2 && B != 4 && B != 8) B = 0;
    if (B > maxBr) B = maxBr;
    // fp32, plain SGPR kernel, hand-scheduled loops allowed: one body per lane means sgpr_loop_asm_jpair
    const bool jpair = in.precision == 32 && variant == NBX_KERNEL_SGPR && o.inner_loop != NBX_LOOP_CXX;
    if (B == 0) B = reference_order_bodies_per_lane(in.i_count, cus, maxBr, jpair);
    c->B = B; c->S = 1; c->jps = in.n_alloc; c->variant = variant;
    c->math = (in.precision == 32 && B >= 2) ? MATH_PACKED : MATH_SCALAR;
    c->epi = o.fused_epilogue == 2 ? EPI_SLAB : EPI_ROW;
    c->grid_x = ceil_div(in.i_count, kBlock * B); c->grid_y = 1;
    return;
  }
  // Launch-bound sizes (fp32): one launch per step with the lanes of a wave splitting j (force_jlane_kernel).  Bodies per
  // wave: the power of two that gives about one wave per SIMD (1024 waves), between 2 and 16.
  const int max_nb = in.precision == 32 ? 16 : 8;  // fp64 bodies take two SGPRs per coordinate
  const bool jlane_auto = variant == NBX_KERNEL_AUTO && o.j_split <= 0 && o.bodies_per_lane == 0 && o.fused_epilogue != 2 &&
                          in.i_count <= (in.precision == 32 ? kJlaneMaxOwn : kJlaneMaxOwnF64);
  if (variant == NBX_KERNEL_JLANE || jlane_auto) {
    int NB = o.bodies_per_lane;
    if ((NB != 2 && NB != 4 && NB != 8 && NB != 16) || NB > max_nb) NB = jlane_bodies_per_wave(in.i_count, 1, in.precision, cus);
    c->B = NB; c->S = 1; c->jps = in.n_alloc; c->math = in.precision == 32 ? MATH_PACKED : MATH_SCALAR; c->variant = NBX_KERNEL_JLANE; c->epi = EPI_ROW;
    c->grid_x = ceil_div(ceil_div(in.i_count, NB), 4); c->grid_y = 1;
    return;
  }
  if (variant != NBX_KERNEL_LDS && variant != NBX_KERNEL_SGPR && variant != NBX_KERNEL_SGPRW) variant = NBX_KERNEL_SGPRW;
  const int maxB = (in.precision == 32 && variant != NBX_KERNEL_SGPRW) ? 8 : 4;
  int B = o.bodies_per_lane;
  if (B != 1 && B != 2 && B != 4 && B != 8) B = 0;
  if (B > maxB) B = maxB;
  if (B == 0) B = in.i_count >= 16384 ? 4 : 2;
  const int iblk = (variant == NBX_KERNEL_SGPRW ? 64 : kBlock) * B;  // bodies per workgroup
  // j-range granularity of one split: a whole LDS tile / two pipelined SGPR batches (per wave)
  // (the hand-scheduled loop of the plain SGPR kernel walks whole trips of up to 64 records)
  // (round 3: where the balanced split rule applies -- few, long splits -- a split is a whole number of 256-record tiles, so
  // that every wave's quarter is whole trips of the hand-scheduled loop whatever n is: n = 50000 used to get 32 splits of 1568
  // records and, with them, the compiler-scheduled loop)
  // Only where tree order is what AUTO takes (n <= 131072).  Above that it runs on request alone -- asked for because it is closer to the
  // true sum than the reference's single chain -- and the number of chains is what buys that: n = 262144 keeps its 8 x 4, 1M its 2 x 4.
  const bool balanced = o.j_split <= 0 && in.precision == 32 && variant == NBX_KERNEL_SGPRW && in.i_count > kRound1SplitMaxOwn && in.n <= kTreeOrderMaxN;
  const int gran = variant == NBX_KERNEL_LDS ? kTile : (variant == NBX_KERNEL_SGPR ? kSgprGran : (balanced ? 256 : 32));
  const int max_split = std::max(1, in.n_alloc / gran);
  int S = o.j_split;
  if (S <= 0) {
    const int bi = ceil_div(in.i_count, iblk);
    if (balanced) S = balanced_j_split(bi, cus, std::min(32, max_split));
    else S = std::min(32, ceil_div(target_wgs, bi));
    // the S partial-acceleration slabs are written and re-read every step: keep them <= 256 MiB
    const size_t own_pad = (size_t)round_up(in.i_count, kBlock), rec = in.precision == 32 ? 16 : 32;
    while (S > 1 && (size_t)S * own_pad * rec > ((size_t)256 << 20)) S /= 2;
  }
  S = std::max(1, std::min(S, max_split));
  int jps = round_up(ceil_div(in.n_alloc, S), gran);
  S = ceil_div(in.n_alloc, jps);  // drop empty tail splits
  c->B = B;
  c->S = S;
  c->jps = jps;
  c->math = (in.precision == 32 && B >= 2) ? MATH_PACKED : MATH_SCALAR;
  c->variant = variant;
  // fused_epilogue: 0 auto, 1 on, 2 off.  A single split integrates directly (EPI_ROW); shapes with j-splits always
  // use the separate integrate kernel (one launch per step for small n is NBX_KERNEL_JLANE's job).
  if (o.fused_epilogue == 2) c->epi = EPI_SLAB;
  else if (S == 1 && variant != NBX_KERNEL_SGPRW) c->epi = EPI_ROW;
  else c->epi = EPI_SLAB;
  c->grid_x = ceil_div(in.i_count, iblk); c->grid_y = S;
}

// nbx_create's launch plan: auto_shape, then the inner loop and graph replay.  NBX_OK, or NBX_ERR_ARG with the text of
// nbx_last_error() in *msg.
inline int plan_launch(const PlanInput& in, const nbx_opts& o, Plan* p, const char** msg) {
  auto fail = [msg](const char* text) { *msg = text; return NBX_ERR_ARG; };
  const int cus = in.cus > 0 ? in.cus : 256;
  *p = Plan{};
  auto_shape(p, in, o);
  if (o.inner_loop != NBX_LOOP_AUTO && o.inner_loop != NBX_LOOP_CXX && o.inner_loop != NBX_LOOP_ASM && o.inner_loop != NBX_LOOP_ASM_TS &&
      o.inner_loop != NBX_LOOP_ASM_PF)
    return fail("nbx_create: inner_loop must be NBX_LOOP_AUTO, NBX_LOOP_CXX, NBX_LOOP_ASM, NBX_LOOP_ASM_TS or NBX_LOOP_ASM_PF");
  // the hand-scheduled loop: where an instance with it is compiled and every wave's j range is whole trips of it (a quarter of a
  // split under the wave split: 256-record splits)
  const bool asm_loop_compiled = instance_index(plan_instance(*p, in.precision, false, LOOP_ASM)) >= 0 &&
                                 (p->variant == NBX_KERNEL_JLANE || p->jps % kSgprGran == 0);
  p->loop = (o.inner_loop != NBX_LOOP_CXX && asm_loop_compiled) ? LOOP_ASM : LOOP_CXX;
  if ((o.inner_loop == NBX_LOOP_ASM || o.inner_loop == NBX_LOOP_ASM_TS || o.inner_loop == NBX_LOOP_ASM_PF) && p->loop != LOOP_ASM)
    return fail("nbx_create: no hand-scheduled loop for this shape (needs fp32; kernel_variant SGPR with 1, 2 or 4 bodies per lane, SGPRW with j_per_split a multiple of 256 and 2 or 4 bodies per lane, or JLANE with 2, 4 or 8 bodies per wave)");
  // Time-sliced wave priority (LOOP_ASM_TS) exists for the row-epilogue SGPR kernel: one workgroup row, every wave resident
  // from the first cycle to the last.  Auto takes it when the fullest CU holds exactly two workgroups, i.e. two waves per
  // SIMD: measured +4.5 % at 512 workgroups, +2.7 % at 384, -0.6 % with one wave per SIMD (nobody to alternate with, six
  // more scalar instructions per trip) and -0.6 ... +0.3 % with three, four or eight (profiles/r02_time_sliced_ab.txt).
  {
    const bool ts_shape = p->loop == LOOP_ASM && p->variant == NBX_KERNEL_SGPR && p->epi == EPI_ROW && p->B >= 2;
    if (o.inner_loop == NBX_LOOP_ASM_TS && !ts_shape)
      return fail("nbx_create: NBX_LOOP_ASM_TS needs the single-row SGPR kernel (reference summation order or j_split 1, fp32, 2 or 4 bodies per lane)");
    const bool two_per_simd = p->grid_x > cus && p->grid_x <= 2 * cus;
    if (ts_shape && (o.inner_loop == NBX_LOOP_ASM_TS || (o.inner_loop == NBX_LOOP_AUTO && two_per_simd))) p->loop = LOOP_ASM_TS;
    // L2 prefetch (LOOP_ASM_PF): the same kernels when the launch leaves one wave per SIMD -- a rank that owns 131072 of 1M bodies:
    // +3.5 %; with two or more waves per SIMD the other waves are the cover and it costs 0.4-1.4 % (profiles/r04_b2_prefetch_ab.txt)
    if (o.inner_loop == NBX_LOOP_ASM_PF && !ts_shape)
      return fail("nbx_create: NBX_LOOP_ASM_PF needs the single-row SGPR kernel (reference summation order or j_split 1, fp32, 2 or 4 bodies per lane)");
    if (ts_shape && (o.inner_loop == NBX_LOOP_ASM_PF || (o.inner_loop == NBX_LOOP_AUTO && p->grid_x <= cus))) p->loop = LOOP_ASM_PF;
  }
  if (o.inner_loop == NBX_LOOP_AUTO && p->variant == NBX_KERNEL_JLANE && p->loop == LOOP_ASM &&
      !jlane_auto_takes_generated_loop(p->B, ceil_div(in.i_count, p->B), cus))
    p->loop = LOOP_CXX;
  // use_graph: 0 auto (launch-bound sizes only: < ~0.3 ms of pair work per step), 1 on, 2 off;
  // capture needs a stream of our own
  p->use_graph = in.own_stream && (o.use_graph == 1 || (o.use_graph == 0 && (double)in.i_count * (double)in.n < 1.5e9));
  p->pairs = p->loop == LOOP_ASM && p->B == 1;  // sgpr_loop_asm_jpair
  p->step = plan_instance(*p, in.precision, false, p->loop);
  p->accel = plan_instance(*p, in.precision, true, p->loop);
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Ensembles (include/nbx_ensemble.h): `members` independent systems of n bodies advanced by one launch per step, grid
// (workgroups per member, members).  Every member runs the jlane kernel body exactly as a context of that NB and loop does.
// ---------------------------------------------------------------------------------------------------------------------------
// The step-kernel instances nbx_ensemble.hip and nbx_ragged.hip compile: the jlane rows of kInstances in their order, so that a
// member can run every shape a jlane context can, and no other.
constexpr int kEnsembleInstanceCount = [] {
  int rows = 0;
  for (const Instance& k : kInstances) rows += k.kind == INST_JLANE;
  return rows;
}();
constexpr auto kEnsembleInstances = [] {
  std::array<Instance, kEnsembleInstanceCount> rows{};
  int at = 0;
  for (const Instance& k : kInstances)
    if (k.kind == INST_JLANE) rows[at++] = k;
  return rows;
}();
constexpr int ensemble_instance_index(const Instance& k) {
  for (int i = 0; i < kEnsembleInstanceCount; ++i)
    if (kEnsembleInstances[i] == k) return i;
  return -1;
}

constexpr int kEnsembleMaxMembers = 65535;  // gridDim.y

struct EnsemblePlan {
  int n_alloc = 0;        // records per member (n rounded up to the tile), followed by kSgprOverread spare records
  int NB = 0, loop = LOOP_CXX, D = 0;
  int grid_x = 0, grid_y = 0;  // workgroups per member (what a context of this NB launches), members
  Instance step{};
};

// Bodies per wave, inner loop and kernel instance of a launch whose members all run the jlane kernel body: the rule plan_ensemble
// and plan_ragged share -- jlane_bodies_per_wave_of with the waves of all members counted, then the loop as for a context.
// `waves_of(nb)` = the launch's waves with nb bodies each; `fn` = the entry point the texts name.  Fills p->NB, loop, D and step.
template <typename P, typename WavesOf>
inline int plan_wave_shape(WavesOf&& waves_of, int members, int precision, int cus, const nbx_opts& o, const char* fn, P* p, const char** msg) {
  auto fail = [fn, msg](const char* text) {
    static thread_local char buf[160];
    std::snprintf(buf, sizeof buf, "%s: %s", fn, text);
    *msg = buf;
    return NBX_ERR_ARG;
  };
  const int max_nb = precision == 32 ? 16 : 8;
  int NB = o.bodies_per_lane;
  if (NB != 0 && ((NB != 2 && NB != 4 && NB != 8 && NB != 16) || NB > max_nb))
    return fail("bodies_per_lane must be 0 (auto), 2, 4, 8 or -- fp32 only -- 16 bodies per wave");
  if (o.inner_loop != NBX_LOOP_AUTO && o.inner_loop != NBX_LOOP_CXX && o.inner_loop != NBX_LOOP_ASM)
    return fail("inner_loop must be NBX_LOOP_AUTO, NBX_LOOP_CXX or NBX_LOOP_ASM");
  // the hand-scheduled loop asked for by name: the choice is among the shapes that have one (fp32: up to 8 bodies per wave)
  if (NB == 0) NB = jlane_bodies_per_wave_of(waves_of, members, precision, cus, o.inner_loop == NBX_LOOP_ASM && precision == 32 ? 8 : 16);
  const bool asm_loop_compiled = ensemble_instance_index({INST_JLANE, precision, NB, 0, 0, 0, false, LOOP_ASM}) >= 0;
  int loop = (o.inner_loop != NBX_LOOP_CXX && asm_loop_compiled) ? LOOP_ASM : LOOP_CXX;
  if (o.inner_loop == NBX_LOOP_ASM && loop != LOOP_ASM)
    return fail("no hand-scheduled loop for this shape (needs fp32 and 2, 4 or 8 bodies per wave)");
  if (o.inner_loop == NBX_LOOP_AUTO && loop == LOOP_ASM && !jlane_auto_takes_generated_loop(NB, waves_of(NB), cus)) loop = LOOP_CXX;
  p->NB = NB; p->loop = loop; p->D = jlane_depth(precision, NB);
  p->step = {INST_JLANE, precision, NB, 0, 0, 0, false, loop};
  return NBX_OK;
}

// nbx_ensemble_create's plan.  NBX_OK, or NBX_ERR_ARG with the text of nbx_last_error() in *msg (which may point into a
// thread-local buffer).  Reads of `o`: bodies_per_lane, inner_loop and the fields an ensemble cannot honour (which must be at
// their defaults).
inline int plan_ensemble(int n, int precision, int members, int cus, const nbx_opts& o, EnsemblePlan* p, const char** msg) {
  auto fail = [msg](const char* text) { *msg = text; return NBX_ERR_ARG; };
  *p = EnsemblePlan{};
  if (cus <= 0) cus = 256;
  if (precision != 32 && precision != 64) return fail("nbx_ensemble_create: precision must be 32 or 64");
  if (n < 1) return fail("nbx_ensemble_create: n must be > 0");
  if (n > (precision == 32 ? kJlaneMaxOwn : kJlaneMaxOwnF64))
    return fail("nbx_ensemble_create: n is beyond the one-launch kernel's range (fp32: 16383, fp64: 12288 bodies); a system of that size fills the card on its own: use nbx_create");
  if (members < 1 || members > kEnsembleMaxMembers) return fail("nbx_ensemble_create: members must be in [1, 65535] (one grid row per member)");
  const int n_alloc = round_up(n, kTile);
  // (cannot be reached with today's limits -- 65535 x (16384 + 528) records; it is what the host's int offsets rest on if they move)
  if ((long long)members * (n_alloc + kSgprOverread) > 0x7fffffffLL)
    return fail("nbx_ensemble_create: members x (records per member + spare records) must fit 31 bits of record index");
  if (o.kernel_variant != NBX_KERNEL_AUTO && o.kernel_variant != NBX_KERNEL_JLANE)
    return fail("nbx_ensemble_create: kernel_variant must be NBX_KERNEL_AUTO or NBX_KERNEL_JLANE (an ensemble steps with the one-launch kernel body)");
  if (o.summation_order != NBX_ORDER_AUTO && o.summation_order != NBX_ORDER_TREE)
    return fail("nbx_ensemble_create: summation_order must be NBX_ORDER_AUTO or NBX_ORDER_TREE (the one-launch kernel sums in tree order)");
  if (o.j_split > 1) return fail("nbx_ensemble_create: j_split must be 0 or 1 (a member's j range is not split over workgroups)");
  if (o.i_begin != 0 || o.i_count != 0) return fail("nbx_ensemble_create: i_begin and i_count must be 0 (an ensemble is not sharded; run one ensemble per GPU)");
  if (o.external_stream != 0) return fail("nbx_ensemble_create: external_stream must be 0 (an ensemble steps on a stream of its own)");
  const int rc = plan_wave_shape([=](int nb) { return (long long)members * ceil_div(n, nb); }, members, precision, cus, o, "nbx_ensemble_create", p, msg);
  if (rc) return rc;
  p->n_alloc = n_alloc;
  p->grid_x = ceil_div(ceil_div(n, p->NB), 4); p->grid_y = members;
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Ragged ensembles (include/nbx_ragged.h): members of DIFFERENT size advanced by one launch per step.  The launch is a 1-D grid
// whose workgroup blockIdx.x reads one RaggedWork descriptor -- which member it serves, which workgroup of that member it is and
// where the member lives -- and runs the jlane kernel body on it, exactly as a context of n_k bodies with that NB and loop does.
// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup's descriptor, as it lies on the device: 32 bytes, self-contained (one dependent scalar fetch per workgroup).
struct RaggedWork {
  unsigned pos_off;  // first record of the member in posm / posm_next
  unsigned vel_off;  // first record of the member in velm
  unsigned ke_off;   // first energy partial of the member in ke_part
  unsigned wg;       // which workgroup of the member this is: [0, grid_k)
  int n, n_alloc;    // the member's bodies, and its records (n rounded up to the tile; kSgprOverread spare records follow)
  unsigned member;   // for the reader of a dump; the kernel does not need it
  unsigned reserved;
};
static_assert(sizeof(RaggedWork) == 32, "a descriptor is at most one 8-dword scalar load, and the table index is a shift");
struct RaggedMember {
  unsigned pos_off, vel_off, ke_off;
  int grid, n, n_alloc;  // grid: workgroups (= energy partials) of the member
};

struct RaggedPlan {
  int members = 0, precision = 32;
  int NB = 0, loop = LOOP_CXX, D = 0;
  int W = 0;                              // workgroups of the launch: the sum of the members' grids
  long long pos_records = 0;              // sum of n_alloc_k + kSgprOverread
  long long vel_records = 0;              // sum of n_alloc_k
  long long ke_parts = 0;                 // = W
  long long bodies_total = 0;
  int n_min = 0, n_max = 0;
  double pairs_per_step = 0.0;            // sum of n_k^2
  Instance step{};
  std::vector<RaggedMember> member;       // by member index
  std::vector<RaggedWork> work;           // by blockIdx.x: longest member first
};

// nbx_ragged_create's plan.  NBX_OK, or NBX_ERR_ARG with the text of nbx_last_error() in *msg (which may point into a
// thread-local buffer where the text names a member).  Reads of `o`: as plan_ensemble.
inline int plan_ragged(const int* n, int members, int precision, int cus, const nbx_opts& o, RaggedPlan* p, const char** msg) {
  auto fail = [msg](const char* text) { *msg = text; return NBX_ERR_ARG; };
  *p = RaggedPlan{};
  if (cus <= 0) cus = 256;
  if (precision != 32 && precision != 64) return fail("nbx_ragged_create: precision must be 32 or 64");
  if (members < 1 || members > kEnsembleMaxMembers) return fail("nbx_ragged_create: members must be in [1, 65535]");
  if (!n) return fail("nbx_ragged_create: n is NULL (the members' sizes)");
  const int n_limit = precision == 32 ? kJlaneMaxOwn : kJlaneMaxOwnF64;
  long long pos_records = 0;
  for (int k = 0; k < members; ++k) {
    if (n[k] < 1 || n[k] > n_limit) {
      static thread_local char text[256];
      std::snprintf(text, sizeof text,
                    n[k] < 1 ? "nbx_ragged_create: n[%d] = %d: every member's n must be > 0"
                             : "nbx_ragged_create: n[%d] = %d is beyond the one-launch kernel's range (fp32: 16383, fp64: 12288 bodies); a system of that size fills the card on its own: use nbx_create",
                    k, n[k]);
      return fail(text);
    }
    pos_records += round_up(n[k], kTile) + kSgprOverread;
  }
  // (cannot be reached with today's limits; it is what the 32-bit record offsets of RaggedWork rest on if they move)
  if (pos_records > 0x7fffffffLL) return fail("nbx_ragged_create: the members' records and spare records together must fit 31 bits of record index");
  if (o.kernel_variant != NBX_KERNEL_AUTO && o.kernel_variant != NBX_KERNEL_JLANE)
    return fail("nbx_ragged_create: kernel_variant must be NBX_KERNEL_AUTO or NBX_KERNEL_JLANE (a member steps with the one-launch kernel body)");
  if (o.summation_order != NBX_ORDER_AUTO && o.summation_order != NBX_ORDER_TREE)
    return fail("nbx_ragged_create: summation_order must be NBX_ORDER_AUTO or NBX_ORDER_TREE (the one-launch kernel sums in tree order)");
  if (o.j_split > 1) return fail("nbx_ragged_create: j_split must be 0 or 1 (a member's j range is not split over workgroups)");
  if (o.i_begin != 0 || o.i_count != 0) return fail("nbx_ragged_create: i_begin and i_count must be 0 (a ragged ensemble is not sharded; run one per GPU)");
  if (o.external_stream != 0) return fail("nbx_ragged_create: external_stream must be 0 (a ragged ensemble steps on a stream of its own)");
  // One NB and one loop for the whole launch (NB is a template argument): jlane_bodies_per_wave's rule with the waves of all
  // members counted.  That members differ in j length does not enter -- nobody has measured whether it matters;
  // scripts/ragged_sweep.py records the time of every NB next to the one taken here.
  auto waves_of = [n, members](int nb) {
    long long w = 0;
    for (int k = 0; k < members; ++k) w += ceil_div(n[k], nb);
    return w;
  };
  const int rc = plan_wave_shape(waves_of, members, precision, cus, o, "nbx_ragged_create", p, msg);
  if (rc) return rc;
  const int NB = p->NB;
  p->members = members; p->precision = precision;
  // members one behind the other, in member order
  p->member.resize((size_t)members);
  p->n_min = p->n_max = n[0];
  long long pos = 0, vel = 0, ke = 0;
  for (int k = 0; k < members; ++k) {
    RaggedMember& m = p->member[(size_t)k];
    m.n = n[k]; m.n_alloc = round_up(n[k], kTile); m.grid = ceil_div(ceil_div(n[k], NB), 4);
    m.pos_off = (unsigned)pos; m.vel_off = (unsigned)vel; m.ke_off = (unsigned)ke;
    pos += m.n_alloc + kSgprOverread; vel += m.n_alloc; ke += m.grid;
    p->n_min = std::min(p->n_min, n[k]); p->n_max = std::max(p->n_max, n[k]);
    p->bodies_total += n[k];
    p->pairs_per_step += (double)n[k] * (double)n[k];
  }
  p->pos_records = pos; p->vel_records = vel; p->ke_parts = ke; p->W = (int)ke;
  // Work order: the dispatcher hands out workgroups in index order, so the members with the longest j loop come first and
  // never form the launch's tail (longest first; ties to the lower member index).  The member index a user sees is unaffected.
  std::vector<int> order((size_t)members);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [p](int a, int b) { return p->member[(size_t)a].n_alloc > p->member[(size_t)b].n_alloc; });
  p->work.reserve((size_t)p->W);
  for (int k : order) {
    const RaggedMember& m = p->member[(size_t)k];
    for (int wg = 0; wg < m.grid; ++wg) p->work.push_back({m.pos_off, m.vel_off, m.ke_off, (unsigned)wg, m.n, m.n_alloc, (unsigned)k, 0u});
  }
  return NBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Accelerations of the members of a ragged ensemble (include/nbx_batch_accel.h): one launch over a 1-D grid whose workgroup
// blockIdx.x reads one RaggedWork descriptor, as the step does, from a list in MEMBER order, where the step's is longest-first.
// With member order the workgroups of members [first, first + count) are the contiguous slice work_begin[first] ..
// work_begin[first + count) of the list, so no call builds or uploads a list.  The descriptors are plan_ragged's own -- the
// member's offsets from its member table, wg = 0 .. grid_k - 1 in order -- so a member runs the workgroups its step runs.
// Nobody has measured whether longest-first within a range would be faster; a range is usually a few members.
// ---------------------------------------------------------------------------------------------------------------------------
struct RaggedAccelPlan {
  std::vector<unsigned> work_begin;  // [members + 1]: prefix sum of the members' workgroups (RaggedMember::grid)
  std::vector<RaggedWork> work;      // [W], member order; within a member by wg
};

inline void plan_ragged_accel(const RaggedPlan& rp, RaggedAccelPlan* a) {
  *a = RaggedAccelPlan{};
  const size_t members = rp.member.size();
  a->work_begin.assign(members + 1, 0u);
  a->work.reserve((size_t)rp.W);
  for (size_t k = 0; k < members; ++k) {
    const RaggedMember& m = rp.member[k];
    a->work_begin[k] = (unsigned)a->work.size();
    for (int wg = 0; wg < m.grid; ++wg) a->work.push_back({m.pos_off, m.vel_off, m.ke_off, (unsigned)wg, m.n, m.n_alloc, (unsigned)k, 0u});
  }
  a->work_begin[members] = (unsigned)a->work.size();  // = rp.W
}

// ---------------------------------------------------------------------------------------------------------------------------
// Diagnostics of the members of a ragged ensemble (include/nbx_ragged_diag.h): one pair-work launch over a 1-D grid whose
// workgroup blockIdx.x reads one RaggedDiagWork descriptor and runs diag_body (nbx_diag_body.hpp) on it, one reduce launch over
// the members asked for.  Member k's shape is exactly what enqueue_diag_t (nbx_diag.hip) gives a context of n_k bodies that owns
// all of them: cols_k = ceil(n_k / (256 kDiagBodies)), (splits_k, per_k) = diag_splits(cols_k, ceil(n_k / 256)), rows_k =
// cols_k splits_k partial rows -- diag_splits itself (nbx_diag_shape.hpp), not a restatement of it.
// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup's descriptor, as it lies on the device: 32 bytes, self-contained for the reason RaggedWork is (one dependent
// scalar fetch at a wave-uniform index).  The workgroup writes partial row row_off + split * cols + col, as diag_body counts rows.
struct RaggedDiagWork {
  unsigned pos_off;  // first record of the member in posm
  unsigned vel_off;  // first record of the member in velm
  unsigned row_off;  // first partial row of the member
  int n;             // the member's bodies
  int col, split;    // this workgroup: body column [0, cols), j split [0, splits)
  int cols;          // the member's body columns
  int tiles_per_split;
};
static_assert(sizeof(RaggedDiagWork) == 32, "a descriptor is at most one 8-dword scalar load, and the table index is a shift");
struct RaggedDiagRows { unsigned row_off; int rows; };  // member k's partial rows [row_off, row_off + rows): what the reduce reads
struct RaggedDiagShape { int cols, tiles, splits, tiles_per_split, rows; };

struct RaggedDiagPlan {
  long long total_rows = 0;                // partial rows of all members
  long long total_groups = 0;              // workgroups of a launch over all members: one per row
  std::vector<RaggedDiagShape> shape;      // by member index
  std::vector<RaggedDiagRows> rows;        // by member index
  std::vector<unsigned> work_begin;        // [members + 1]: prefix sum of the members' rows = of their workgroups
  std::vector<RaggedDiagWork> work;        // member order; within a member by split, then by column
};

// The work list is in MEMBER order, where plan_ragged's is longest-first.  Under the ragged size limits (n <= 16383, so cols <= 32)
// the kDiagTargetGroups bound of diag_splits never binds (it asks for 1024 / 32 = 32 splits at least, tiles / 4 <= 16 allow fewer),
// and tiles_per_split <= 7 for every member: with fewer than 8 tiles there is one split of at most 7 tiles; from 8 tiles up
// s = floor(tiles / 4) >= 2 and ceil(tiles / s) <= 7 (tiles = 4 s + r, r <= 3: 4 + ceil(r / s) <= 6; 7 occurs at tiles = 7
// alone).  So every workgroup of the launch sums between 1 and 7 tiles for 512 bodies: there is no long tail to schedule
// around.  With member order a range [first, first + count) of members is a contiguous slice of the list -- work_begin[first] ..
// work_begin[first + count) -- so no call builds or uploads a list.  Nobody has measured whether another order is faster.
inline void plan_ragged_diag(const RaggedPlan& rp, int precision, RaggedDiagPlan* d) {
  *d = RaggedDiagPlan{};
  const int B = precision == 32 ? kDiagBodies<float> : kDiagBodies<double>;
  const size_t members = rp.member.size();
  d->shape.resize(members);
  d->rows.resize(members);
  d->work_begin.assign(members + 1, 0u);
  long long rows = 0;
  for (size_t k = 0; k < members; ++k) {
    const RaggedMember& m = rp.member[k];
    RaggedDiagShape& s = d->shape[k];
    s.cols = ceil_div(m.n, kBlock * B);
    s.tiles = ceil_div(m.n, kTile);
    diag_splits(s.cols, s.tiles, &s.splits, &s.tiles_per_split);
    s.rows = s.cols * s.splits;
    d->rows[k] = {(unsigned)rows, s.rows};
    d->work_begin[k] = (unsigned)rows;
    rows += s.rows;  // 65535 members x 512 rows at most: 25 bits
  }
  d->work_begin[members] = (unsigned)rows;
  d->total_rows = d->total_groups = rows;
  d->work.reserve((size_t)rows);
  for (size_t k = 0; k < members; ++k) {
    const RaggedMember& m = rp.member[k];
    const RaggedDiagShape& s = d->shape[k];
    for (int split = 0; split < s.splits; ++split)
      for (int col = 0; col < s.cols; ++col)
        d->work.push_back({m.pos_off, m.vel_off, d->rows[k].row_off, m.n, col, split, s.cols, s.tiles_per_split});
  }
}

}  // namespace nbx
