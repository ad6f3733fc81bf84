/*
 * nbx_kick.h -- a velocity-only half step for every kind of object: v += a(x) * h at the current positions, the positions
 * untouched.  Kept apart from nbx.h, nbx_ensemble.h and nbx_ragged.h, whose symbol sets and structs stay as they are
 * (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via nbx_last_error(), one host thread drives
 * an object at a time.
 *
 * Why: every step call performs the reference's update v += a(x) * dt; x += v * dt.  Read as leapfrog, the stored velocities
 * sit half a step away from the stored positions: kenergy + potential of the diagnostics calls carries an O(dt) term that
 * belongs to the read-out and not to the trajectory, and dt < 0 does not retrace a forward step.  The sequence
 *     kick(-dt / 2);  step(dt) x N;  kick(+dt / 2)
 * is kick-drift-kick leapfrog: second order, time reversible, and its N steps are the existing step launches bit for bit.
 * Outside the library the same takes an accel call, a download, a host update and an upload, which starts the object over.
 *
 * Velocity arithmetic: for every owned body and each component c, v.c = add_rn(v.c, mul_rn(a.c, h)) -- the velocity half of a
 * step's update, multiply and add rounded separately (not fused).
 *
 * The acceleration: a is bit for bit what the object's accel call (nbx_accel, nbx_ensemble_accel, nbx_ragged_accel) returns at
 * that moment.
 *
 * The kick size: h is rounded to the object's precision once.  Any finite h is accepted, zero and negative values included;
 * h == 0 leaves every velocity comparing equal to before.  A NaN or an infinity is NBX_ERR_ARG ("h is not finite").
 *
 * What is untouched: positions, which of the two position buffers is current, steps_done, launches_timed /
 * force_launches_timed and the *_ms_total fields (no launch of a kick is timed), and the state of graph replay.  Steps issued
 * after a kick produce the bits they would produce from an upload of the kicked state.
 *
 * Kinetic energy: the kick leaves the kinetic-energy partials describing the KICKED velocities -- the terms m * (vx^2 + vy^2 +
 * vz^2) a step computes, through the reduce a step uses.  kenergy_out receives 0.5 * sum m v^2, for an ensemble or a ragged
 * ensemble one value per member; a following step call with nsteps == 0 reports the same bits.  The call is asynchronous on the
 * object's stream unless kenergy_out != NULL; with it, one reduce launch and one synchronisation, as a step call.
 *
 * Launch shape: an ensemble or a ragged ensemble is kicked by ONE launch over its step's own grid (a ragged ensemble: its
 * step's own work list) -- the step's kernel body with an epilogue that updates the velocity alone.  A context, whatever its
 * kernel variant and summation order, is kicked by two: the acc-only force launch of nbx_accel, then one launch that adds the
 * j-split slabs in nbx_accel's order and updates the velocities.  Nothing is read back.
 *
 * Groups: every rank kicks its owned slice; positions do not move, so nothing is exchanged, and with kenergy_out == NULL the
 * call is not a collective.  With kenergy_out != NULL the ranks' partial sums are added exactly as nbx_group_step adds them; for
 * a one-process-per-GPU group that is a collective every rank must call, bounded by the watchdog (nbx_collective_timeout).
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    h is not finite
 *   NBX_ERR_STATE  the object has not been uploaded; for an ensemble or a ragged ensemble: any member has not been (the text
 *                  names the first such member)
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 * Every one of these checks comes before the first HIP call.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows the object's
 * precision, gives unspecified values for every body of that system, and of that system alone: the other members of an
 * ensemble or a ragged ensemble are kicked to the bits they are kicked to without it.
 *
 * Deliberately not here: a kick size per member; a member range (all members are kicked, as a step call steps all of them); a
 * drift-only call; a command-line word or an environment knob in nbody.x (its output is the reference's); hipGraph replay of
 * kicks.
 */
#ifndef NBX_KICK_H
#define NBX_KICK_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_kick(nbx_ctx* c, double h, double* kenergy_out /* or NULL */);
int nbx_ensemble_kick(nbx_ensemble* e, double h, double* kenergy_out /* [members] or NULL */);
int nbx_ragged_kick(nbx_ragged* r, double h, double* kenergy_out /* [members] or NULL */);
int nbx_group_kick(nbx_group* g, double h, double* kenergy_out /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_KICK_H */
