/*
 * nbx_batch_accel.h -- the accelerations of the members of an ensemble (nbx_ensemble.h) or of a ragged ensemble (nbx_ragged.h)
 * at their current positions, without integrating: what nbx_accel does for a context, for any range of members with ONE kernel
 * launch, one device-to-host copy and one synchronisation.  Kept apart from nbx_ensemble.h and nbx_ragged.h, whose symbol sets
 * and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via
 * nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: forces alone -- to measure a force error, to choose a time step, to drive an integrator of one's own -- otherwise take a
 * context per member and an nbx_accel call on each: a launch, a read-back and a synchronisation per member, the cost ensembles
 * exist to remove.
 *
 * Output: the accelerations of the bodies of members [first, first + count) at the current positions, in the object's precision
 * (float for 32, double for 64), in the host layout of the object's download call: member-major count * n elements for an
 * ensemble, member first + k at [k * n, (k + 1) * n); for a ragged ensemble the members end to end without padding, member
 * first at element 0.  Any of acc_x, acc_y, acc_z may be NULL to skip that array, which is then never written; if all three
 * are NULL the call checks its arguments and launches nothing.
 *
 * Bit contract: member k's values are the bits nbx_accel returns for an nbx_ctx of n_k bodies holding the member's state, created
 * with kernel_variant = NBX_KERNEL_JLANE and the bodies_per_lane and inner_loop that the object's stats call reports: the same
 * kernel body over the same workgroups.  They do not depend on first, on count, on the member's place or on its neighbours.
 *
 * Launch shape: whatever the range, one kernel launch over the workgroups of the members in the range alone, one device-to-host
 * copy of the range's span of the acceleration buffer, one synchronisation.  Ordered on the object's stream: after an asynchronous
 * step call the values belong to the state after those steps.
 *
 * No side effects: the call does not change the trajectory, the energies a following step call of no steps reports, steps_done,
 * or launches_timed / step_ms_total (they describe the step kernel; this launch is not timed).  Further steps produce the bits
 * they would have produced without the call.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL; [first, first + count) leaves [0, members) (checked in 64 bits)
 *   NBX_ERR_STATE  a member of the range has not been uploaded (the text names the first such member); members outside the
 *                  range need not have been
 *   NBX_OK         count == 0, or all three arrays NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the acceleration buffer (16 or 32 bytes per body record, the size of the velocity buffer) or, for a ragged
 *                  ensemble, the work list (32 bytes per workgroup) did not fit; both are allocated on the first call that
 *                  launches, kept for the object's life and freed by its destroy call
 * Every argument and state check comes before the first HIP call.
 *
 * Unspecified results: a coordinate or a mass that is not finite, or a coordinate whose square overflows the object's precision,
 * gives unspecified values for every body of that member, and of that member alone.
 *
 * Deliberately not here: output to a device pointer (the arrays are host memory); accelerations in the reference summation
 * order or from the exact (validation) kernel -- members sum in the tree order of the one-launch kernel, as their steps do; a
 * potential per body; hipGraph replay.
 */
#ifndef NBX_BATCH_ACCEL_H
#define NBX_BATCH_ACCEL_H

#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_ensemble_accel(nbx_ensemble* e, int32_t first, int32_t count, void* acc_x, void* acc_y, void* acc_z /* [count * n] or NULL */);
int nbx_ragged_accel(nbx_ragged* r, int32_t first, int32_t count, void* acc_x, void* acc_y, void* acc_z /* [n[first] + ... + n[first + count - 1]] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_BATCH_ACCEL_H */
