/*
 * nbx_ragged.h -- ragged ensembles of libnbx.so: independent systems ("members") of DIFFERENT size, all advanced by ONE
 * kernel launch per time step.  Kept apart from nbx.h and nbx_ensemble.h, whose symbol sets and structs are part of the ABI
 * as they stand (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via nbx_last_error(), no
 * exception crosses the boundary, one host thread drives a ragged ensemble at a time.
 *
 * Why: nbx_ensemble serves many systems of ONE size.  A mixed population (clusters of 300, 1000, 2048, 5000 bodies) had to
 * choose between one context per system (launch bound), one ensemble per distinct size (the launch gaps back, and nothing
 * gained where all sizes differ) and padding every member to the largest n with zero-mass bodies (n_max^2 pair work per
 * member).  Here the launch is a 1-D grid over a work list: every workgroup looks up which member it serves and which
 * workgroup of that member it is, so each member costs its own n_k^2.
 *
 * What a member computes: member k computes exactly what an nbx_ctx of n_k bodies computes with kernel_variant =
 * NBX_KERNEL_JLANE and the bodies_per_lane / inner_loop that nbx_ragged_stats reports -- the same kernel body over the same
 * workgroups, so positions, velocities and kinetic energy are the same bits.  One bodies_per_lane and one inner_loop serve
 * all members of a launch.  Members do not interact and do not depend on their neighbours or on the order of the work list.
 *
 * Host arrays are the members' SoA arrays laid end to end without padding, in the ensemble's precision (float for 32,
 * double for 64): for a call on members [first, first + count), member first + k occupies
 * [n[first] + ... + n[first + k - 1], ... + n[first + k]).
 *
 * Launches are plain launches on a non-blocking stream the ragged ensemble owns, one per step (plus one reduce launch where
 * the kinetic energy is asked for); no graph capture.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows the
 * ensemble's precision, gives unspecified values for every body of that member, and of that member alone: the other members'
 * positions, velocities and kinetic energies are the bits they are without it, whatever their sizes and places.
 *
 * Deliberately not here: a time step per member; the diagnostics of nbx_diag.h for ragged members; sharding over GPUs (run
 * one ragged ensemble per GPU); nbx_accel (nbx_batch_accel.h has it); the reference summation order and the exact (validation) kernel; hipGraph replay;
 * a command-line word in nbody.x (its argv is the reference's).  Velocity-only half steps, which make the steps of every member
 * kick-drift-kick leapfrog, are in nbx_kick.h.
 */
#ifndef NBX_RAGGED_H
#define NBX_RAGGED_H

#include "nbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_ragged nbx_ragged;

typedef struct nbx_ragged_stats_t {
  int32_t struct_size;          /* = sizeof(nbx_ragged_stats_t); 0 is accepted as "this version".  Set on return */
  int32_t members, precision;
  int32_t n_min, n_max;         /* the smallest and the largest member */
  int32_t bodies_total;         /* sum of n[k] */
  int32_t bodies_per_lane, inner_loop; /* what the planner took for the whole launch: bodies per wave, and NBX_LOOP_CXX or NBX_LOOP_ASM */
  int32_t grid_x, block;        /* workgroups of one step launch (the sum of the members' workgroups), threads per workgroup */
  int32_t cu_count;
  int32_t reserved;             /* 0 */
  double  pairs_per_step;       /* sum of n[k]^2 */
  int64_t steps_done, launches_timed;
  double  step_ms_total;        /* HIP-event time of those launches (nbx_ragged_profile on) */
} nbx_ragged_stats_t;

/*
 * A ragged ensemble of `members` systems, member k of n[k] bodies, at `precision` (32 | 64).  1 <= members <= 65535;
 * 1 <= n[k] <= 16383 (fp64: 12288) -- the range of the one-launch kernel; a larger system fills the card on its own: use
 * nbx_create; the error text names the offending member.  The members' records (n[k] rounded up to 256, plus 528 spare records
 * each) must together fit 31 bits.  n is read during the call only.
 * opts (nullable): as for nbx_ensemble_create -- device, bodies_per_lane (0 = auto, 2, 4, 8, fp32 also 16: bodies per wave)
 * and inner_loop (NBX_LOOP_AUTO, NBX_LOOP_CXX, NBX_LOOP_ASM) are honoured; kernel_variant must be NBX_KERNEL_AUTO or
 * NBX_KERNEL_JLANE, summation_order NBX_ORDER_AUTO or NBX_ORDER_TREE, j_split <= 1, i_begin == i_count == 0,
 * external_stream == 0; anything else is NBX_ERR_ARG naming the field.  The remaining fields are ignored.  Every argument is
 * checked before the first HIP call; without a device valid arguments give NBX_ERR_DEVICE.
 * With all n[k] equal the planner takes what nbx_ensemble_create takes for that n and that many members.
 */
int nbx_ragged_create(nbx_ragged** out, int32_t members, const int32_t* n /* [members] */, int32_t precision, const nbx_opts* opts);
void nbx_ragged_destroy(nbx_ragged* r); /* NULL-safe */

/*
 * Host -> device for members [first, first + count).  Packs {x, y, z, G*m} and {vx, vy, vz, m} with the same G and the same
 * arithmetic as nbx_upload.  Members may arrive in several calls, in any order; a member uploaded again starts over from the
 * new state.  NBX_ERR_ARG if the range leaves [0, members) or an array is NULL.
 */
int nbx_ragged_upload(nbx_ragged* r, int32_t first, int32_t count, const void* pos_x, const void* pos_y, const void* pos_z,
                      const void* vel_x, const void* vel_y, const void* vel_z, const void* mass);

/*
 * nsteps time steps of every member, one launch each.  Asynchronous unless kenergy_out != NULL: then one reduce launch follows
 * the last step, the call synchronises and stores 0.5 * sum m v^2 of member m after the last step in kenergy_out[m].  With
 * nsteps == 0 it reports the energies the last step left (zeros if no step has run), as nbx_step does.
 * NBX_ERR_STATE until every member has been uploaded.
 * dt is the time step of every member and of all nsteps steps, as nbx_step takes it: any finite value, zero and negative values
 * included, converted to the ragged ensemble's precision by round-to-nearest.  NBX_ERR_ARG ("dt is not finite") for a NaN or an
 * infinity, here and in nbx_ragged_step_trace, before the members' uploads are looked at.
 */
int nbx_ragged_step(nbx_ragged* r, double dt, int32_t nsteps, double* kenergy_out /* [members] or NULL */);

/* As nbx_ragged_step, with the energies after EVERY step: ke_trace[s * members + m]; synchronises. */
int nbx_ragged_step_trace(nbx_ragged* r, double dt, int32_t nsteps, double* ke_trace /* [nsteps][members] */);

/* Device -> host for members [first, first + count): current positions and velocities.  Any pointer may be NULL to skip that
 * array.  Synchronises. */
int nbx_ragged_download(nbx_ragged* r, int32_t first, int32_t count, void* pos_x, void* pos_y, void* pos_z, void* vel_x,
                        void* vel_y, void* vel_z);

int nbx_ragged_sync(nbx_ragged* r);

/* Per-launch HIP-event timing of the step kernel (on the ragged ensemble's stream), reported by nbx_ragged_stats. */
int nbx_ragged_profile(nbx_ragged* r, int32_t enable);
int nbx_ragged_stats(nbx_ragged* r, nbx_ragged_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NBX_RAGGED_H */
