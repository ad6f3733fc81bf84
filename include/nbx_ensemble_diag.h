/*
 * nbx_ensemble_diag.h -- the physics diagnostics of nbx_diag.h for the members of an ensemble (nbx_ensemble.h): mass, kinetic
 * and potential energy, momentum and mass moment of each member, for any range of members, with ONE pair-work launch, one
 * reduce launch and one read-back for all of them.  Kept apart from nbx_ensemble.h and nbx_diag.h, whose symbol sets stay as
 * they are; same conventions: plain C, int status, text via nbx_last_error().
 *
 * Why: the members of an ensemble are small systems in the chaotic regime, where energy and momentum conservation are the
 * checks of a trajectory that mean something.  Without this call a member has to be downloaded and uploaded into an nbx_ctx of
 * its own to be asked -- two launches and a synchronising read-back per member, the launch-bound pattern an ensemble removes.
 *
 * What a member's entry holds: field for field and bit for bit what nbx_diagnostics returns for an nbx_ctx of n bodies (owning
 * all of them, same precision) that holds the member's state -- the same kernel body over the same workgroups, the same
 * partial rows, the same reduce order.  Members do not see each other; the result does not depend on first, count or on the
 * member's place in the ensemble.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows the
 * ensemble's precision, gives unspecified values for the entry of that member, and of that member alone.
 */
#ifndef NBX_ENSEMBLE_DIAG_H
#define NBX_ENSEMBLE_DIAG_H

#include "nbx_ensemble.h"
#include "nbx_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * out[k] describes member first + k at the ensemble's current state: mass, kenergy, potential, momentum, mass_moment, with
 * i_count = n and steps_done = the ensemble's.  Ordered on the ensemble's stream (after an asynchronous nbx_ensemble_step it
 * describes the state after those steps); synchronises; does not change the trajectory.  Each out[k].struct_size must be 0 or
 * sizeof(nbx_diag_t) on entry and is set on return.
 * NBX_ERR_ARG: e or out is NULL, [first, first + count) leaves [0, members), or a struct_size is wrong -- nothing is written.
 * NBX_ERR_STATE: a member of the range has not been uploaded (the text names it).  count == 0: NBX_OK, nothing written.
 * NBX_ERR_ALLOC: the partials (allocated on the first call, about 7 % of the position buffers at most) did not fit.
 */
int nbx_ensemble_diagnostics(nbx_ensemble* e, int32_t first, int32_t count, nbx_diag_t* out /* [count] */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_ENSEMBLE_DIAG_H */
