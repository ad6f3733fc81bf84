/*
 * nbx_ensemble.h -- ensembles of libnbx.so: S independent systems ("members") of n bodies each, all advanced by ONE kernel
 * launch per time step.  Kept apart from nbx.h, whose symbol set and structs are part of the ABI as it stands
 * (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via nbx_last_error(), no exception crosses
 * the boundary, one host thread drives an ensemble at a time.
 *
 * Why: a system of a few thousand bodies is launch bound -- one context leaves most of the card idle and pays the fixed cost
 * of a launch every step.  Such systems are run many at a time (the same system from perturbed initial conditions, or many
 * different small ones); an ensemble gives the pair work of all members to one launch, grid (workgroups per member, S).
 *
 * What a member computes: exactly what an nbx_ctx of n bodies computes with kernel_variant = NBX_KERNEL_JLANE and the
 * bodies_per_lane / inner_loop that nbx_ensemble_stats reports -- the same kernel body over the same workgroups, so positions,
 * velocities and kinetic energy are the same bits.  Members do not interact and do not depend on their neighbours.
 *
 * Host arrays are member-major SoA: `count * n` elements of the ensemble's precision (float for 32, double for 64), member
 * first + k at [k * n, (k + 1) * n) -- the reference's ParticleSoA arrays (ver7/Particle.hpp:43-58) of `count` systems laid end
 * to end.
 *
 * Launches are plain launches on a non-blocking stream the ensemble owns, one per step (plus one reduce launch where the
 * kinetic energy is asked for): issuing a launch costs the host 3-4 us, and an ensemble worth creating has more pair work per
 * step than that.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows the
 * ensemble's precision, gives unspecified values for every body of that member, and of that member alone: the other members'
 * positions, velocities and kinetic energies are the bits they are without it.
 *
 * Deliberately not here: members of different n (nbx_ragged.h has them); sharding one ensemble over GPUs (run one ensemble per GPU); nbx_accel for
 * ensembles (nbx_batch_accel.h has it); the reference summation order and the exact (validation) kernel; hipGraph replay; a command-line word in nbody.x
 * (its argv is the reference's).  The diagnostics of nbx_diag.h for the members of an ensemble are in nbx_ensemble_diag.h.
 * Velocity-only half steps, which make the steps of every member kick-drift-kick leapfrog, are in nbx_kick.h.
 */
#ifndef NBX_ENSEMBLE_H
#define NBX_ENSEMBLE_H

#include "nbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_ensemble nbx_ensemble;

typedef struct nbx_ensemble_stats_t {
  int32_t struct_size;          /* = sizeof(nbx_ensemble_stats_t); 0 is accepted as "this version".  Set on return */
  int32_t n, n_alloc, members, precision;
  int32_t bodies_per_lane, inner_loop; /* what the planner took: bodies per wave, and NBX_LOOP_CXX or NBX_LOOP_ASM */
  int32_t grid_x, grid_y, block, cu_count;
  int64_t steps_done, launches_timed;
  double  step_ms_total;        /* HIP-event time of those launches (nbx_ensemble_profile on) */
} nbx_ensemble_stats_t;

/*
 * An ensemble of `members` systems of n bodies at `precision` (32 | 64).  1 <= n <= 16383 (fp64: 12288) -- the range of the
 * one-launch kernel; a larger system fills the card on its own: use nbx_create.  1 <= members <= 65535, and
 * members * (n rounded up to 256 + 528 spare records) must fit 31 bits.
 * opts (nullable): device, bodies_per_lane (0 = auto, 2, 4, 8, fp32 also 16: bodies per wave) and inner_loop (NBX_LOOP_AUTO,
 * NBX_LOOP_CXX, NBX_LOOP_ASM; ASM fails where no hand-scheduled loop exists: fp64, 16 bodies per wave) are honoured.
 * kernel_variant must be NBX_KERNEL_AUTO or NBX_KERNEL_JLANE, summation_order NBX_ORDER_AUTO or NBX_ORDER_TREE, j_split <= 1,
 * i_begin == i_count == 0, external_stream == 0; anything else is NBX_ERR_ARG naming the field.  The remaining fields are
 * ignored.  Every argument is checked before the first HIP call; without a device valid arguments give NBX_ERR_DEVICE.
 */
int nbx_ensemble_create(nbx_ensemble** out, int32_t n, int32_t precision, int32_t members, const nbx_opts* opts);
void nbx_ensemble_destroy(nbx_ensemble* e); /* NULL-safe */

/*
 * Host -> device for members [first, first + count).  Packs {x, y, z, G*m} and {vx, vy, vz, m} with the same G and the same
 * arithmetic as nbx_upload.  Members may arrive in several calls, in any order; a member uploaded again starts over from the
 * new state.  NBX_ERR_ARG if the range leaves [0, members) or an array is NULL.
 */
int nbx_ensemble_upload(nbx_ensemble* e, int32_t first, int32_t count, const void* pos_x, const void* pos_y, const void* pos_z,
                        const void* vel_x, const void* vel_y, const void* vel_z, const void* mass);

/*
 * nsteps time steps of every member, one launch each.  Asynchronous unless kenergy_out != NULL: then one reduce launch follows
 * the last step, the call synchronises and stores 0.5 * sum m v^2 of member m after the last step in kenergy_out[m].  With
 * nsteps == 0 it reports the energies the last step left (zeros if no step has run), as nbx_step does.
 * NBX_ERR_STATE until every member has been uploaded.
 * dt is the time step of every member and of all nsteps steps, as nbx_step takes it: any finite value, zero and negative values
 * included, converted to the ensemble's precision by round-to-nearest.  NBX_ERR_ARG ("dt is not finite") for a NaN or an
 * infinity, here and in nbx_ensemble_step_trace, before the members' uploads are looked at.
 */
int nbx_ensemble_step(nbx_ensemble* e, double dt, int32_t nsteps, double* kenergy_out /* [members] or NULL */);

/* As nbx_ensemble_step, with the energies after EVERY step: ke_trace[s * members + m]; synchronises. */
int nbx_ensemble_step_trace(nbx_ensemble* e, double dt, int32_t nsteps, double* ke_trace /* [nsteps][members] */);

/* Device -> host for members [first, first + count): current positions and velocities.  Any pointer may be NULL to skip that
 * array.  Synchronises. */
int nbx_ensemble_download(nbx_ensemble* e, int32_t first, int32_t count, void* pos_x, void* pos_y, void* pos_z, void* vel_x,
                          void* vel_y, void* vel_z);

int nbx_ensemble_sync(nbx_ensemble* e);

/* Per-launch HIP-event timing of the step kernel (on the ensemble's stream), reported by nbx_ensemble_stats. */
int nbx_ensemble_profile(nbx_ensemble* e, int32_t enable);
int nbx_ensemble_stats(nbx_ensemble* e, nbx_ensemble_stats_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NBX_ENSEMBLE_H */
