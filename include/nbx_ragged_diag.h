/*
 * nbx_ragged_diag.h -- the physics diagnostics of nbx_diag.h for the members of a ragged ensemble (nbx_ragged.h): mass, kinetic
 * and potential energy, momentum and mass moment of each member, for any range of members, with ONE pair-work launch, one
 * reduce launch and one read-back for all of them, whatever their sizes.  This is where the diagnostics of ragged members live:
 * nbx_ragged.h, whose text and symbol set stay as they are, still lists them under "Deliberately not here".  Kept apart from
 * nbx_ragged.h, nbx_diag.h and nbx_ensemble_diag.h; same conventions: plain C, int status, text via nbx_last_error().
 *
 * Why: the members of a ragged ensemble are small systems in the chaotic regime, where energy and momentum conservation are
 * the checks of a trajectory that mean something.  Without this call a member has to be downloaded and uploaded into an
 * nbx_ctx of its size to be asked -- a create, an upload, two launches and a synchronising read-back per member, the
 * launch-bound pattern a ragged ensemble removes; and where all sizes differ, one ensemble per size does not help either.
 *
 * What a member's entry holds: field for field and bit for bit what nbx_diagnostics returns for an nbx_ctx of n[k] bodies
 * (owning all of them, same precision) that holds the member's state -- the same kernel body over the same workgroups, the same
 * partial rows, the same reduce order.  Members do not see each other; the result does not depend on first, on count, on the
 * member's place in the ragged ensemble or on its neighbours' sizes.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows the
 * ensemble's precision, gives unspecified values for the entry of that member, and of that member alone.
 */
#ifndef NBX_RAGGED_DIAG_H
#define NBX_RAGGED_DIAG_H

#include "nbx_ragged.h"
#include "nbx_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * out[k] describes member first + k at the ragged ensemble's current state: mass, kenergy, potential, momentum, mass_moment,
 * with i_count = n[first + k] and steps_done = the ragged ensemble's.  Ordered on the ragged ensemble's stream (after an
 * asynchronous nbx_ragged_step it describes the state after those steps); synchronises; does not change the trajectory, and
 * leaves the energies nbx_ragged_step(.., 0, ..) reports alone.  Each out[k].struct_size must be 0 or sizeof(nbx_diag_t) on
 * entry and is set on return.
 * NBX_ERR_ARG: r or out is NULL, [first, first + count) leaves [0, members) (checked in 64 bits: first + count does not wrap),
 * or a struct_size is wrong -- nothing is written.
 * NBX_ERR_STATE: a member of the range has not been uploaded (the text names the first such member); members outside the range
 * need not have been.  count == 0: NBX_OK, nothing written.
 * NBX_ERR_ALLOC: the work list, the partials or the reduced fields (built and allocated on the first call, of a size fixed for
 * the object's life: one 32-byte descriptor and 72 bytes of partials per 512 bodies and j split) did not fit.
 * Every argument and state check comes before the first HIP call.
 */
int nbx_ragged_diagnostics(nbx_ragged* r, int32_t first, int32_t count, nbx_diag_t* out /* [count] */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_RAGGED_DIAG_H */
