/*
 * nbx_hermite.h -- a device-resident fourth-order Hermite stepper: P(EC) steps of every body of a context, of every member of an
 * ensemble or of every member of a ragged ensemble, two launches a step, nothing read back.  Kept apart from the other headers,
 * whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text
 * via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: the library's resident integrators are the reference's semi-implicit Euler step and the leapfrog the kick calls make of
 * it -- second order at best.  The jerk call gives a and adot on the device, and a fourth-order Hermite predictor-corrector
 * needs nothing else; but integrated from outside the library every step pays one O(n) upload, one O(n) read-back and one
 * stream synchronisation: the host-bound pattern every batch call here was written to remove.  A collisional N-body user asks
 * for this integrator first.
 *
 * Definition: one step of size h takes (x, v) and the kept (a0, j0) -- acceleration and its time derivative at (x, v) -- to
 *   predict    vp = v + h a0 + h^2/2 j0          xp = x + h v + h^2/2 a0 + h^3/6 j0
 *   evaluate   a1, j1 = the acceleration and its time derivative of the state (xp, vp), masses as uploaded
 *   correct    v1 = v + h/2 (a0 + a1) + h^2/12 (j0 - j1)        x1 = x + h/2 (v + v1) + h^2/12 (a0 - a1)
 * and (a1, j1) become (a0, j0) of the next step: P(EC), one evaluation a step, no second one at the corrected state.
 *
 * Arithmetic: T is the object's precision.  h is dt rounded once to T and widened to double; the host computes k2 = h * 0.5,
 * k6 = h / 6.0 and h3 = h / 3.0 once in fp64.  x, v, a0, j0, a1, j1 are T values, widened.  Every operation below is a
 * separately rounded fp64 multiply or add (mul_rn / add_rn: no build contracts one), innermost bracket first, per component:
 *     vp = v + h*(a0 + k2*j0)                      xp = x + h*(v + k2*(a0 + h3*j0))            each rounded once to T
 *     v1 = v + k2*((a0 + a1) + k6*(j0 - j1))       x1 = x + k2*((v + v1) + k6*(a0 - a1))
 * The unrounded fp64 v1 enters the formula for x1; x1 and v1 are then rounded once to T and stored.  a1, j1 are the bits the
 * jerk call returns for the state (xp, vp): the same pair function restated, the same shape rule evaluated at (n, n), j ascending
 * within a split, the splits added in fp64 in split order, one rounding to T.  numpy's separately rounded fp64 operations on
 * T-valued arrays reproduce all of it bit for bit.
 *
 * Starting values and resume: with resume == 0 the call first evaluates a0, j0 at the resident state, by the same two launches
 * without prediction or correction.  With resume != 0 it reuses what the previous Hermite call on this object left: the caller
 * promises that no upload, step, kick, commit or local step came between (analysis calls in between are fine: they write
 * buffers of their own).  The library refuses where it can see the promise broken: there was no previous Hermite call, or
 * steps_done or the current position buffer is not what that call left, or kinetic-energy partials exist (a step or a kick
 * wrote them; a Hermite call leaves none).  An upload that leaves all three alone is beyond what the library sees.
 *
 * Launch shape: a step is exactly two launches.  (1) A pair-work kernel with the predictor fused into its loads, in three forms
 * with the grids of the jerk call's three kernels.  For every j record of a tile one thread of the workgroup loads the position
 * record, loads the velocity record and the kept a0 and j0 records only where j < n (zeros otherwise), predicts, and stages the
 * predicted {xp, yp, zp, gm} and the predicted velocity in the two LDS tiles; the lane's own two bodies are predicted the same
 * way.  Every workgroup predicts with the same operations, so j == i still gives d = u = 0 exactly and nothing is masked.  No
 * predicted state is ever written to memory.  The pair loop is the jerk call's: in fp32, per j record, 26 packed VALU and 2
 * v_rsq_f32, nothing unpacked, the fp64 predictor outside it; two LDS tiles, 8 KiB in fp32 and 16 KiB in fp64; no scratch.
 * (2) A finish kernel with the corrector fused in, one thread per body: it adds the splits, corrects, stores x1 into the
 * current position record with .w (gm) untouched, v1 into the velocity record with .w (the mass) untouched, and a1, j1 into the
 * kept records.  The update is in place and safe: a thread touches its own body only, and the pair launch has finished.
 * Padding records stay zero.  resume == 0 costs 2 + 2 * nsteps launches, resume != 0 costs 2 * nsteps.  No atomics.
 *
 * Contracts: the same state, dt, nsteps and resume give the same bits on every call.  The state after nbx_hermite_step(dt, 1,
 * 0) is bit for bit what this round trip of public calls leaves: the jerk call, the predictor above on the host, an upload of
 * the predicted state with the same masses, the jerk call, the corrector above on the host, an upload.  A resumed call continues
 * that round trip carried on with a1, j1: steps (dt, a, 0) then (dt, b, 1) are steps (dt, a + b, 0) bit for bit; without resume
 * they are not, for a fresh evaluation at the corrected state is a different quantity from a1, j1 at the predicted one.  A
 * member of an ensemble or a ragged ensemble ends bit for bit where a lone context holding its state ends, wherever the member
 * sits and whatever the context's options.
 *
 * Semantics: all members of a batch object step, as in a step call.  The call is asynchronous on the object's stream: it never
 * reads back and never synchronises.  Any finite dt is accepted, zero and negative values included.
 *
 * State afterwards: untouched are steps_done (these steps are not counted), which position buffer is current, every *_timed /
 * *_ms_total field (no Hermite launch is timed), the cached graphs, every analysis call's scratch and the resident tracers --
 * tracers do not move with a Hermite step: they stay where they were.  The kinetic-energy partials belong to no state
 * afterwards, as after an upload: a step call of no steps reports 0 until a step or a kick has run.  The diagnostics see the new
 * state.  A following step call produces the bits it would produce from an upload of the downloaded state.
 *
 * Status, in this order, all before the first HIP call but the last:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    dt is not finite (as a double, or once rounded to T)
 *   NBX_ERR_ARG    nsteps < 0
 *   NBX_ERR_ARG    the bodies of the object -- n, members * n, or the total of the members -- exceed 2^22 = 4194304, which keeps
 *                  the row indices of the partials in 32 bits
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_ERR_STATE  a context does not own all n bodies (the velocities of the others are not resident)
 *   NBX_ERR_STATE  resume cannot be honoured (see above)
 *   NBX_OK         nsteps == 0: nothing is launched, nothing changes
 *   NBX_ERR_ALLOC  the buffers did not fit
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite gives unspecified values for every body
 * of that system, and of that system alone.
 *
 * Deliberately not here: groups; a member range (all members step); a time step per member or per body (block steps);
 * kenergy_out (ask the diagnostics); P(EC)^n; tracers moving with the scheme; hipGraph replay; a command-line word or an
 * environment knob in nbody.x.
 */
#ifndef NBX_HERMITE_H
#define NBX_HERMITE_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_hermite_step(nbx_ctx* c, double dt, int32_t nsteps, int32_t resume);
int nbx_ensemble_hermite_step(nbx_ensemble* e, double dt, int32_t nsteps, int32_t resume);
int nbx_ragged_hermite_step(nbx_ragged* r, double dt, int32_t nsteps, int32_t resume);

#ifdef __cplusplus
}
#endif
#endif /* NBX_HERMITE_H */
