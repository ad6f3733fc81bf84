/*
 * nbx_advance.h -- adaptive power-of-two time steps chosen on the device: fourth-order Hermite P(EC) steps of every body of a
 * context, of every member of an ensemble or of every member of a ragged ensemble, each system with a clock and a step of its
 * own, three launches a step, nothing read back; and one query call that reads the clocks.  Kept apart from the other headers,
 * whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text
 * via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: the Hermite stepper takes one dt per call for every body of every member.  In a small system a single close encounter
 * decides whether a fixed dt is far too large or a thousand times too small, so a user who wants an adaptive step must
 * synchronise, read a value back and call again with a new dt, once per step -- and in an ensemble the tightest member sets the
 * step of every other one.  That per-step read-back is the host-bound pattern every batch call here was written to remove.  A
 * fourth-order Hermite scheme already holds what the standard step criterion needs: from (a0, j0) and (a1, j1) it forms the
 * second and third derivatives of the acceleration at no extra pair work.  Here every system chooses its own step on the device,
 * eta is the accuracy knob and nobody has to guess a dt.
 *
 * Definition: a system is a context, or one member of a batch object.  Each system has a clock record on the device: {t, h, k2,
 * k6, h3, ih, h_last, steps, floor_steps} and whether the step of h will be a floor step.  One step of a system is the Hermite
 * stepper's P(EC) step
 *   predict    vp = v + h a0 + h^2/2 j0          xp = x + h v + h^2/2 a0 + h^3/6 j0
 *   evaluate   a1, j1 = the acceleration and its time derivative of the state (xp, vp), masses as uploaded
 *   correct    v1 = v + h/2 (a0 + a1) + h^2/12 (j0 - j1)        x1 = x + h/2 (v + v1) + h^2/12 (a0 - a1)
 * with h read from that system's clock record instead of an argument; then t += h, and the next h is chosen (the criterion and
 * the quantiser below).  h is always a power of two.
 *
 * Arithmetic: T is the object's precision.  The predictor, the pair work, the split sums and the corrector are exactly the
 * Hermite stepper's formulas and rounding: separately rounded fp64 operations (mul_rn / add_rn), one rounding to T.  Since h is a
 * power of two, (T)h == h, k2 = h * 0.5 and ih = 1 / h are exact, and k6 = h * (1.0 / 6.0) and h3 = h * (1.0 / 3.0) equal the
 * host's h / 6.0 and h / 3.0 bit for bit, because scaling by a power of two commutes with rounding.  An adaptive step of size h
 * therefore leaves the bits that the Hermite stepper's fixed step of dt = h leaves.
 *   The criterion is evaluated per body in the finish kernel, in fp64, from the T values widened; every operation is mul_rn or
 * add_rn, innermost bracket first, per component:
 *     d = a0 - a1
 *     a2 = (((-6 d) - h*((4 j0) + (2 j1))) * ih) * ih
 *     a3 = ((((12 d) + (6 h)*(j0 + j1)) * ih) * ih) * ih
 *     a2 = a2 + h*a3                                  (a2 at the end of the step)
 *     |v|^2 = (vx*vx + vy*vy) + vz*vz                 A = |a1|^2, J = |j1|^2, S = |a2|^2, C = |a3|^2
 *     s_i = (sqrt(A*S) + J) / (sqrt(J*C) + S)         where the denominator is > 0, else +inf
 * After the evaluation that starts a call without resume there is no previous step: there s_i = A / J where J > 0, else +inf.
 * The per-system minimum is q = min_i s_i; a NaN candidate is never selected (compared with < against a running minimum that
 * starts at +inf).  Aarseth's eta parameter is eta^2 here: the suggested step is eta * sqrt(q).  The fp64 sqrt and / of the device
 * are the correctly rounded ones.
 *   The quantiser uses integers only.  eta2 = eta * eta is computed once on the host.  k_crit = floor(E / 2) with E the
 * unbiased binary exponent of eta2 * q (its exponent field minus 1023: +inf gives 1024, zero -1023), so that 2^k_crit is the
 * largest power of two whose square is <= eta2 * q.  dt_cap = 2^k_cap, k_floor = k_cap - levels.  With k the exponent of the step
 * just taken the next exponent is k + 1 if k_crit > k and t is a multiple of 2^(k+1) -- t * (0.5 * ih) == floor(t * (0.5 * ih))
 * --, k if k_crit >= k and the first case does not apply, k_crit otherwise; at the start, k_crit.  The result is clamped to
 * [k_floor, k_cap]; a step where the clamp raised it counts in floor_steps once it is taken.  Because t_end is a whole multiple
 * of dt_cap, t is always a multiple of h, t += h is exact, no step overshoots and every system lands on t_end exactly.  No sqrt
 * of h and no logarithm is ever taken; the chosen step depends on the last bit of s only at an exact power-of-four boundary.
 *
 * Launch shape: a step is exactly three launches and there are no atomics.  (1) The pair kernel, in three forms (context,
 * ensemble, ragged) with the Hermite stepper's grids and its shape rule evaluated at (n, n): the same two LDS tiles, 8 KiB in
 * fp32 and 16 KiB in fp64, the same pair loop -- in fp32, per j record, 26 packed VALU and 2 v_rsq_f32, nothing unpacked, no
 * fp64 -- and no scratch; the only addition is a wave-uniform load of the system's clock record before the body.  (2) The finish
 * kernel, one thread per body: the Hermite stepper's finish plus the candidate s_i, written as one double per body to a
 * candidate buffer.  (3) The clock kernel, one workgroup of 256 per system: a strided minimum over the system's candidates
 * through LDS, then one thread runs the quantiser and writes the clock record.  Every kernel receives t_end and treats a system
 * whose t >= t_end as done: its pair-work workgroups return at once, its finish threads write nothing and the clock kernel leaves
 * its record alone.  done is computed and not stored, so a later call with a larger t_end carries on.  A call without resume
 * enqueues 3 launches for the starting evaluation plus 3 * max_steps, a call with resume 3 * max_steps: the host cannot know
 * when a system is done, so all of them are always enqueued.  The intended use is advance(max_steps = a few dozen), then the
 * clock call, repeated until every member is done.
 *
 * Contracts: the same state and arguments give the same bits on every call.  A system that took the steps h_1, h_2, ... is bit
 * for bit where the Hermite stepper's fixed steps of dt = h_1, h_2, ..., each resumed after the first, leave it.  Calls (max_steps
 * = a, resume = 0) then (max_steps = b, resume = 1) are (max_steps = a + b, resume = 0) bit for bit, clocks included.  A member
 * of an ensemble or a ragged ensemble ends bit for bit where a lone context holding its state ends, with the same clock.
 *
 * Semantics: all members of a batch object advance, each by its own steps.  The advance calls are asynchronous on the object's
 * stream: they never read back and never synchronise.  resume makes the promise of the Hermite stepper's resume and is checked
 * the same way: steps_done, the current position buffer, and no kinetic-energy partials.  An advance call takes the kept records
 * over: the fixed stepper's resume is refused after it, and an advance resume is refused after a fixed-step call.  dt_cap and
 * levels must equal the previous call's on resume; eta may change and takes effect at the next choice; t_end may grow.  A call
 * without resume starts every clock at t = 0 and, also with max_steps == 0, evaluates and sets the clocks, so that dt_next can be
 * asked for before the first step.  The clock calls are ordered on the stream, synchronise once and read back once.
 *
 * State afterwards: as the Hermite stepper leaves it -- untouched are steps_done (these steps are not counted), which position
 * buffer is current, every *_timed / *_ms_total field, the cached graphs, every analysis call's scratch and the resident
 * tracers, which do not move; the kinetic-energy partials belong to no state afterwards, as after an upload.
 *
 * Status of the advance calls, in this order, all before the first HIP call but the last:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    t_end, dt_cap or eta is not finite, or is <= 0 (eta: also where eta * eta leaves the range of a double)
 *   NBX_ERR_ARG    dt_cap is not a power of two, or not a normal value of T
 *   NBX_ERR_ARG    levels is outside [0, 40]
 *   NBX_ERR_ARG    t_end is not a whole multiple of dt_cap, or t_end / (dt_cap * 2^-levels) > 2^52
 *   NBX_ERR_ARG    max_steps < 0
 *   NBX_ERR_ARG    the bodies of the object -- n, members * n, or the total of the members -- exceed 2^22 = 4194304
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit, or does not own all n bodies
 *   NBX_ERR_STATE  resume cannot be honoured (see above)
 *   NBX_OK         max_steps == 0 and resume != 0: nothing is launched, nothing changes
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Status of the clock calls: NBX_ERR_ARG for a NULL handle, a NULL out, a member range outside the object or a struct_size that
 * is neither 0 nor this library's; NBX_ERR_STATE where the object is not uploaded, has a local step pending or is a slice, or
 * where no advance call has been made on it; all before the first HIP call.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows T, gives
 * unspecified values for every body and for the clock of that system, and of that system alone: the other systems' t, dt_last,
 * dt_next, steps and floor_steps are what they are without it.
 *
 * Deliberately not here: a step per body (block steps: this is the shared-step half of that); P(EC)^n; groups; a member range
 * (all members advance); tracers moving with the scheme; hipGraph replay; a command-line word or an environment knob in nbody.x.
 */
#ifndef NBX_ADVANCE_H
#define NBX_ADVANCE_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_clock_t {
  int32_t struct_size;   /* 0 accepted, set on return */
  int32_t n;
  double  t;             /* the system's time: 0 at a call without resume, a sum of the steps taken */
  double  dt_last;       /* the step last taken (0: none yet) */
  double  dt_next;       /* the step the next one will take */
  int64_t steps;         /* steps taken since the call without resume */
  int64_t floor_steps;   /* of those, steps taken at the floor although the criterion asked for less */
  int32_t done;          /* t >= the t_end of the last call */
  int32_t reserved;
} nbx_clock_t;

int nbx_advance(nbx_ctx* c, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume);
int nbx_ensemble_advance(nbx_ensemble* e, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume);
int nbx_ragged_advance(nbx_ragged* r, double t_end, double dt_cap, int32_t levels, double eta, int32_t max_steps, int32_t resume);

int nbx_clock(nbx_ctx* c, nbx_clock_t* out);
int nbx_ensemble_clock(nbx_ensemble* e, int32_t first, int32_t count, nbx_clock_t* out);
int nbx_ragged_clock(nbx_ragged* r, int32_t first, int32_t count, nbx_clock_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NBX_ADVANCE_H */
