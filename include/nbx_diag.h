/*
 * nbx_diag.h -- physics diagnostics of libnbx.so: mass, kinetic and potential energy, linear momentum and mass moment
 * of the current state, so that a run can say whether it conserves energy and momentum.  Kept apart from nbx.h, whose
 * symbol set and structs are part of the ABI as it stands.
 *
 * Every field of nbx_diag_t is an additive partial over the bodies [i_begin, i_begin + i_count) a context owns; the sum of
 * the partials over the ranks of a job is the system value:
 *   mass        = sum m_i
 *   kenergy     = 1/2 sum m_i |v_i|^2        (the same terms, in the same precision, as nbx_step's kinetic energy)
 *   potential   = -1/2 sum_{i owned} m_i sum_{j < n, j != i} G m_j / sqrt(|x_j - x_i|^2 + eps^2),
 *                 eps^2 = 1e-3f, G = 6.67259e-11f, G m_j as uploaded (the records' G*m); j == i is excluded exactly,
 *                 distinct bodies at one position are included with the softened term
 *   momentum    = sum m_i v_i
 *   mass_moment = sum m_i x_i                (centre of mass = mass_moment / mass)
 * Positions are the current (committed) buffer.  All accumulation over bodies is in fp64 and in a fixed order: the same
 * state gives the same bits on every call, whatever the context's launch-shape options.  The call does not change the
 * trajectory.
 */
#ifndef NBX_DIAG_H
#define NBX_DIAG_H

#include "nbx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_diag_t {
  int32_t struct_size; /* = sizeof(nbx_diag_t); 0 is accepted as "this version".  Set on return */
  int32_t i_count;     /* bodies covered */
  int64_t steps_done;  /* time steps of the state the values describe */
  double  mass, kenergy, potential;
  double  momentum[3], mass_moment[3];
} nbx_diag_t;

/* Owned-slice partials of the context's current state; synchronises.  NBX_ERR_ARG on NULL, NBX_ERR_STATE before
 * nbx_upload or while a local step awaits nbx_commit. */
int nbx_diagnostics(nbx_ctx* ctx, nbx_diag_t* out);

/* System totals of a group: the ranks' partials summed in rank order.  Single-process groups add them on the host; a
 * one-process-per-GPU group (nbx_group_create_rank) all-gathers them once -- collective, every rank calls it and gets the
 * same numbers, bounded by the collective watchdog.  Same errors as nbx_diagnostics. */
int nbx_group_diagnostics(nbx_group* g, nbx_diag_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NBX_DIAG_H */
