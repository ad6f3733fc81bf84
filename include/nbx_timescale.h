/*
 * nbx_timescale.h -- what the time step should be: the pair approach rate, the pair free-fall rate and the closest softened
 * separation of a system, evaluated on the device from the resident state, for a context, for any range of an ensemble's
 * members or for any range of a ragged ensemble's members in one call.  Kept apart from the other headers, whose symbol sets
 * and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via
 * nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: every step call takes any finite dt and nbx_kick.h makes stepping leapfrog, but nothing says what dt should be.  In a
 * small system that is chaotic after its first bounce a single close encounter decides whether a fixed dt is far too large or
 * a thousand times too small.  Finding out on the host takes a download and an O(n^2) search per system; nbx_accel does not see
 * relative velocities.  This is the standard pair criterion of direct-summation codes:
 *     approach_rate2 = max over i < n, j < n, j != i of |v_j - v_i|^2 / (|x_j - x_i|^2 + eps^2)
 *     freefall_rate2 = max over the same pairs of G (m_i + m_j) / (|x_j - x_i|^2 + eps^2)^(3/2)
 *     min_r2         = min over the same pairs of |x_j - x_i|^2 + eps^2
 * both rates in 1/time^2; a suggested step is eta / sqrt(max(approach_rate2, freefall_rate2)) with eta of a few hundredths.
 * eps^2 and G are the library's (1e-3f and 6.67259e-11f, widened in fp64); G m_i is the value nbx_upload stored in the body's
 * position record, G times m rounded once in the object's precision.
 *
 * Which pairs count: j == i is excluded exactly.  Records at or beyond n -- the zero padding of the position buffer, whatever
 * lies behind a member's last velocity -- are excluded exactly, by a mask and not as a by-product: a padding record has
 * G*m = 0, which removes it from a potential, but it has a position (the origin) and would still produce a non-zero approach
 * rate.  Two DISTINCT bodies at the same position are included, with r2 = eps^2.  A system of one body has no pair: both
 * rates are 0 and min_r2 is +infinity.
 *
 * Per-pair arithmetic, in the object's precision T, one inline device function for all three kinds of object:
 *     dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))        (the force kernels' r2)
 *     ux,uy,uz = v_j - v_i;  w  = fma(ux,ux, fma(uy,uy, uz*uz))
 *     inv = rsq(r2);  inv2 = inv*inv;  approach = w*inv2;  freefall = ((gm_i + gm_j)*inv)*inv2
 * rsq is the force kernels' reciprocal square root (fp32: the hardware's, within 1 ulp; fp64: the hardware's seed and one
 * Newton step).  Every product and sum not written as fma above is rounded separately (mul_rn, add_rn); the power-of-two
 * scales the fp64 records and rsq carry are undone exactly after the reduction.  Maxima and minima are taken in T and widened
 * exactly to double.  To first order, with u the unit round-off of T, a rate is within 16u (approach) and 17.5u (freefall) of
 * the exact value in fp32, about 42u and 57u in fp64; min_r2 is within 5u.
 *
 * Nothing is summed, so: the same state gives the same bits on every call; whatever the context's kernel variant, summation
 * order, bodies per lane or j split; and a member's entry is bit for bit what nbx_timescale returns for a context of n bodies
 * holding that member's state, whatever range it was asked in.
 *
 * Semantics, those of nbx_diagnostics and nbx_ensemble_diagnostics: the call is ordered on the object's stream -- after an
 * asynchronous step call it describes the state after those steps -- and synchronises once.  It reads the current position
 * buffer and the velocities and writes only buffers of its own.  Untouched: positions, velocities, which position buffer is
 * current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and the state of graph replay.  One
 * pair-work launch, one reduce launch and one read-back serve all systems asked for; no atomics.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    out is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members)
 *   NBX_ERR_ARG    a wrong struct_size in any out[k]; nothing is written
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_ERR_STATE  a context does not own all n bodies (the velocities of the others are not resident: the restriction
 *                  nbx_step has)
 *   NBX_ERR_ALLOC  the partials did not fit
 * Every check but the last comes before the first HIP call.  count == 0 returns NBX_OK and writes nothing.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite, or whose square overflows T, gives
 * unspecified values for the entry of that system, and of that system alone.
 *
 * Deliberately not here: groups and sliced contexts; the indices of the extreme pair; a value per body; a dt per member (dt
 * stays one value per step call, this call only helps choose it); a command-line word or an environment knob in nbody.x (its
 * output is the reference's); hipGraph replay.
 */
#ifndef NBX_TIMESCALE_H
#define NBX_TIMESCALE_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_timescale_t {
  int32_t struct_size;   /* = sizeof(nbx_timescale_t); 0 accepted as "this version"; set on return */
  int32_t n;             /* bodies of the system described */
  int64_t steps_done;
  double approach_rate2; /* max over i < n, j < n, j != i of |v_j - v_i|^2 / (|x_j - x_i|^2 + eps^2)   [1/time^2] */
  double freefall_rate2; /* max over the same pairs of G (m_i + m_j) / (|x_j - x_i|^2 + eps^2)^(3/2)   [1/time^2] */
  double min_r2;         /* min over the same pairs of |x_j - x_i|^2 + eps^2 (softened; closest pair) */
} nbx_timescale_t;

int nbx_timescale(nbx_ctx* c, nbx_timescale_t* out);
int nbx_ensemble_timescale(nbx_ensemble* e, int32_t first, int32_t count, nbx_timescale_t* out /* [count] */);
int nbx_ragged_timescale(nbx_ragged* r, int32_t first, int32_t count, nbx_timescale_t* out /* [count] */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_TIMESCALE_H */
