/*
 * nbx_jerk.h -- the jerk: for every body of the resident system its acceleration and the time derivative of that acceleration,
 * evaluated on the device from the resident positions and velocities, for a context, for any range of an ensemble's members or
 * for any range of a ragged ensemble's members in one call.  Kept apart from the other headers, whose symbol sets and structs
 * stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via nbx_last_error(), one host
 * thread drives an object at a time.
 *
 * Why: every analysis call so far describes where the bodies are or how strongly they are bound at one instant.  The quantity a
 * collisional N-body user asks for first is the time derivative of each body's acceleration.  It gives a time step per body --
 * eta |a| / |adot|, the only form of the Aarseth criterion that needs no history, where the time-scale call returns one value
 * per system -- and it is all a fourth-order Hermite predictor-corrector needs besides the acceleration.  Both need relative
 * velocities, so neither the acceleration call nor the field at caller-supplied points can supply them; differencing
 * accelerations over a trial step costs two more O(n^2) launches and most of the fp32 digits.  Without this call the jerk is a
 * download and an O(n^2) host loop per system, the host-bound pattern the batch calls exist to remove.
 *
 * Definition, for body i of a system of n bodies, T the object's precision, gm_j the value the upload call stored in body j's
 * position record (G times m rounded once in T), d = x_j - x_i, u = v_j - v_i,
 * r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2))) (the force kernels' r2; eps^2 and G are the library's, 1e-3f and 6.67259e-11f,
 * widened in fp64):
 *     a_i    = sum over j < n of gm_j d / r2^(3/2)
 *     adot_i = sum over j < n of gm_j [ u / r2^(3/2) - 3 (d.u) d / r2^(5/2) ]
 * adot is the exact time derivative of the softened a along straight-line motion of all bodies: eps2 does not depend on time.
 *
 * Masks: j == i is NOT masked: d = u = 0 makes both of its terms exact zeros, as the term of a point on a body is in the field
 * at caller-supplied points.  Position records at or beyond n -- the zero padding of the position buffer -- have gm = 0 and add
 * exact zeros.  A velocity is loaded only where j < n, and zero is staged otherwise: what lies behind a system's last velocity
 * is never read.
 *
 * Per-pair arithmetic in fp32, one inline device function for all three kinds of object:
 *     inv = rsq(r2);  inv2 = inv*inv;  s = (gm*inv)*inv2;  a += d*s  (fma)
 *     rv = fma(dx,ux, fma(dy,uy, dz*uz));  c = (rv*inv2)*(-3);  t_a = fma(c, d_a, u_a);  adot_a += t_a*s  (fma)
 * The acceleration's operations are exactly those of the field at caller-supplied points, restated.  c takes two separately
 * rounded multiplies, first by inv2 and then by -3.  Every multiply or add not written as an fma goes through mul_rn / add_rn.
 * rsq is the hardware's reciprocal square root, within 1 ulp.
 *
 * Per-pair arithmetic in fp64: the seed y = v_rsq_f64(r2), y2 = y*y and the residual h = fma(-r2, y2, 1) serve both powers:
 *     s    = ((gm*y)*y2) * fma(h, fma(h, 15, 12), 8)      the field's: 8 gm r2^(-3/2) (1 + O(h^3)); the records carry G*m/8
 *     inv2 = fma(y2, fma(h, h, h), y2)                    second order: since r2 y2 = 1 - h, 1/r2 = y2 / (1 - h)
 *                                                         = y2 (1 + h + h^2 + h^3 + ...), and what is left is y2 h^3 / (1 - h):
 *                                                         relative h^3 < 2^-69 for a seed good to 2^-24 (|h| < 2^-23)
 * and rv, c, t and the six sums as in fp32.  The prescale 1/8 and the 8 of the polynomial are powers of two, so every rounding
 * is the one the unscaled operation would make, and what leaves the pair loop carries no scale.
 *
 * Sums and finish: six sums per body, in T, j ascending within a split of the j range; the finish adds a body's splits in fp64
 * in split order and rounds once to T.  Columns, splits and tiles per split are the shape rule of the field at caller-supplied
 * points evaluated at (n, n): a function of n alone.
 *
 * Error of one term, to first order, u the unit round-off of T, relative to the term's scale -- |d_a| gm r2^(-3/2) for a and
 * gm r2^(-3/2) (|u_a| + 3 (|dx ux| + |dy uy| + |dz uz|) |d_a| / r2) for adot.  Each of d, u carries u; r2 carries 5u.
 *   fp32: inv carries 2.5u + 2u (1 ulp) = 4.5u, s three times that and three multiplies: 16.5u; the a term adds d's u and the
 *         product inside the fma: 17.5u.  rv carries 2u per product and 3 roundings: 5u of its scale; inv2 9u + 1u; c two more:
 *         17u; t adds d_a's u and the fma's: 19u of the bracket's scale; the adot term 19u + 16.5u = 35.5u.
 *   fp64: s carries 7.5u from r2 and 5 roundings: 12.5u, the a term 13.5u; inv2 5u and 3 roundings: 8u; c 5u + 8u + 2u = 15u;
 *         t 17u; the adot term 17u + 12.5u = 29.5u -- whatever the seed does, to O(h^3).
 * The sum over a split adds at most (tiles per split * 256) u of the sum of the scales; the finish one rounding.
 *
 * Operation count, fp32, per j record (two pairs, the lane's two bodies, everything on the packed pipe): 3 subtracts (d), 3 fma
 * (r2), 3 multiplies (inv2, the two of s), 3 fma (a), 3 subtracts (u), 1 multiply and 2 fma (rv), 2 multiplies (c), 3 fma (t),
 * 3 fma (adot) = 26 packed VALU and 2 v_rsq_f32, against 13 and 2 of the field at caller-supplied points; two 16-byte LDS reads,
 * the position and the velocity record.
 *
 * Contracts: the same state gives the same bits on every call.  A member's six arrays are bit for bit what nbx_jerk returns for
 * a context of n bodies holding that member's state, whatever range was asked, wherever the member sits and whatever the
 * context's options (kernel variant, summation order, bodies per lane, j split).  acc is bit for bit the acceleration the field
 * call returns at the bodies' own positions with m = n: the same shape rule, the same operations, the same order, the same
 * finish.
 *
 * Arrays: every pointer of nbx_jerk_out_t may be NULL; a NULL array is never written.  If all six are NULL the arguments are
 * checked and nothing is launched.  Host arrays of float for 32 and of double for 64, in the layout of the object's download
 * call: an ensemble is member-major, count * n elements; a ragged ensemble has its members end to end, member `first` at
 * element 0.
 *
 * Contexts: a sliced context (i_count < n) is refused -- the velocities of the other bodies are not resident in it.  A context
 * with a local step awaiting nbx_commit is refused.
 *
 * Semantics: the call is ordered on the object's stream -- after an asynchronous step call it describes the state after those
 * steps -- and synchronises once.  One pair-work launch, one finish launch and one read-back serve the whole range; no atomics.
 * It reads the current position buffer and the velocities and writes only buffers of its own (allocated on first use, grown when
 * a larger call arrives, freed with the object).  Untouched: positions, velocities, which position buffer is current,
 * steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    out is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304, which
 *                  keeps the row indices of the partials in 32 bits
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_ERR_STATE  a context does not own all n bodies (the velocities of the others are not resident)
 *   NBX_OK         count == 0 or all six pointers NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a coordinate, a velocity component or a mass that is not finite gives unspecified values for every body
 * of that system, and of that system alone.
 *
 * Deliberately not here: groups and sliced contexts; caller-supplied points; snap and crackle; per-body maxima of the pair
 * rates; a resident Hermite stepper (nbx.hermite in the Python binding integrates by host round trip on this call); device
 * pointers for the results; hipGraph replay; a command-line word or an environment knob in nbody.x.
 */
#ifndef NBX_JERK_H
#define NBX_JERK_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_jerk_out_t { /* every pointer may be NULL; a NULL array is never written */
  void* acc[3];                 /* a_i,     in T, arrays in the layout of the object's download call */
  void* jerk[3];                /* da_i/dt, in T */
} nbx_jerk_out_t;

int nbx_jerk(nbx_ctx* c, const nbx_jerk_out_t* out);
int nbx_ensemble_jerk(nbx_ensemble* e, int32_t first, int32_t count, const nbx_jerk_out_t* out);
int nbx_ragged_jerk(nbx_ragged* r, int32_t first, int32_t count, const nbx_jerk_out_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NBX_JERK_H */
