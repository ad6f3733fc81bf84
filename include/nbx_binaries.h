/*
 * nbx_binaries.h -- who is bound to whom: for every body of the resident system its most bound partner, the specific two-body
 * energy of that pair and the number of bodies it is bound to, evaluated on the device from the resident state, for a context,
 * for any range of an ensemble's members or for any range of a ragged ensemble's members in one call.  Kept apart from the other
 * headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int
 * status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: the proximity calls (nbx_neighbours, nbx_paircount, nbx_knn, nbx_fof) answer geometric questions from positions alone,
 * and mutual nearest neighbours are only binary CANDIDATES; nbx_timescale reads relative velocities but returns three extremes
 * per system, neither the pair nor a value per body.  The question those candidates exist for -- which pairs are gravitationally
 * bound, how tightly, and which bodies are bound to nobody (escapers) -- had no call.  Users of small chaotic systems ask it
 * every few steps: binary formation, hardening and ejection are what such runs are about.  Without this call that is a download
 * and an O(n^2) host search per system, the launch-bound and host-bound pattern the batch calls exist to remove.
 *
 * Definition, for body i of a system of n bodies, T the object's precision, gm the value nbx_upload stored in the body's
 * position record (G times m rounded once in T, as in nbx_timescale.h):
 *     e(i, j)    = |v_j - v_i|^2 / 2 - G (m_i + m_j) / sqrt(|x_j - x_i|^2 + eps^2): the specific two-body energy, the energy
 *                  of the pair's relative motion per reduced mass; eps^2 and G are the library's (1e-3f and 6.67259e-11f,
 *                  widened in fp64)
 *     partner[i] = the j < n, j != i with the smallest e(i, j); among equal bit patterns the LOWEST j
 *     energy[i]  = that smallest value, in T (a host array of float for 32, of double for 64)
 *     bound[i]   = the number of j < n, j != i with e(i, j) < 0
 * A system of one body has partner = -1, energy = +infinity, bound = 0.  Which pairs count: j == i is excluded exactly, and
 * records at or beyond n -- the zero padding of the position buffer, whatever lies behind a system's last velocity -- are
 * excluded exactly, by a mask and not as a by-product, as in nbx_timescale.h: a padding record has a position (the origin) and
 * a zero velocity and would otherwise be the partner of a body that is bound to nobody; velocity records at or beyond n are
 * never read.  Two DISTINCT bodies at one position count, with r2 = eps^2.
 *
 * Per-pair arithmetic, in T, one inline device function for all three kinds of object:
 *     dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))        (the force kernels' and nbx_timescale's r2)
 *     ux,uy,uz = v_j - v_i;  w  = fma(ux,ux, fma(uy,uy, uz*uz))                   (nbx_timescale's w)
 *     s = add_rn(gm_i, gm_j);  inv = rsq(r2);  e = fma(-s, inv, w/2)
 * rsq is the force kernels' reciprocal square root (fp32: the hardware's, within 1 ulp; fp64: the hardware's seed and one
 * Newton step).  w/2 is exact.  Every product and sum not written as fma above is rounded separately (mul_rn, add_rn).  The
 * kernels carry an exact power-of-two scale through the minimum -- the doubled value fma(-2s, inv, w), the fp64 records' G*m/8
 * and rsq's 2/sqrt -- and undo it once per body afterwards: a minimum and a sign commute with a positive scale.
 * Consequences:
 *     the subtractions are exact under i <-> j up to sign, the squares do not see the sign and the sum s is commutative, so
 *     e(i, j) and e(j, i) are the same bits;
 *     partner[i] == j && partner[j] == i && energy[i] < 0 identifies a mutual bound pair exactly;
 *     if partner[i] == j then energy[j] <= energy[i];
 *     (bound[i] > 0) == (energy[i] < 0);
 *     the sum of bound over a system is even.
 * The error, to first order, with u the unit round-off of T.  e is a difference of two non-negative terms, A = w/2 and
 * B = s * inv, and cancels, so the bound is relative to A + B and not to |e|.  A: each of ux, uy, uz carries u, a square 2u,
 * the multiply and the two fma one u each: 5u.  B: s carries u; r2 carries 5u (nbx_neighbours.h), of which rsq passes on half,
 * and adds its own error: 2u in fp32 (1 ulp); in fp64 the Newton step leaves 3/2 d^2, d the relative error of the hardware's
 * seed, and adds three roundings, about 3u -- 12u + 3u at d = 2^-25, the figure nbx_pair.hpp works with, 48u + 3u at d = 2^-24
 * (the device tests have seen 30u on e, a d of about 2^-24.4).  So inv carries 4.5u in fp32 and 17.5u to 53.5u in fp64, B 5.5u
 * and 18.5u to 54.5u.  The product s * inv is not rounded, the final fma rounds once: u |e| <= u (A + B).  So
 *     |e - exact| <= 6.5u (A + B) in fp32 and, for d <= 2^-24, 55.5u (A + B) in fp64:
 * each term is a strict subset of the operations of nbx_timescale.h's approach (w * inv^2) and freefall (s * inv^3), which see
 * the error of inv twice and three times.  A pair whose |e| is below that bound may be counted in bound[] on either side of 0.
 *
 * Nothing is summed in floating point: the partner is a minimum with a lowest-index tie-break, the count an integer sum.  So
 * the same state gives the same bits on every call, for every launch shape and whatever the context's kernel variant,
 * summation order, bodies per lane or j split; and a member's results are bit for bit what nbx_binaries returns for a context
 * of n bodies holding that member's state, whatever range it was asked in and wherever the member sits in its object.
 *
 * Arrays: any of partner, energy, bound may be NULL; a NULL array is never written.  If all three are NULL the arguments are
 * checked and nothing is launched.  Callers who pass bound == NULL do not pay for the count.  The layout is that of the object's
 * download call: an ensemble is member-major, count * n elements; a ragged ensemble has its members end to end, member `first`
 * at element 0.  partner is member-local: an index into the member's own bodies.
 *
 * Contexts: a sliced context (i_count < n) is refused -- the velocities of the other bodies are not resident in it: the
 * restriction nbx_timescale and nbx_step have.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_neighbours and nbx_timescale: the call is ordered on the object's stream -- after an asynchronous
 * step call it describes the state after those steps -- and synchronises once.  One pair-work launch, one finish launch and one
 * read-back serve the whole range; no atomics.  It reads the current position buffer and the velocities and writes only buffers
 * of its own (allocated on first use, grown when a larger call arrives, freed with the object).  Untouched: positions,
 * velocities, which position buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and
 * the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304: the
 *                  bound of nbx_field.h, which keeps the row indices of the partials in 32 bits and the scratch below 1 GiB
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_ERR_STATE  a context does not own all n bodies (the velocities of the others are not resident)
 *   NBX_OK         count == 0 or all of partner, energy, bound NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a body with a coordinate, a velocity component or a mass that is not finite, or whose r2, w or s
 * overflows T for every partner, gives unspecified values for that body only (and for the bodies it is a partner of).
 *
 * Deliberately not here: groups and sliced contexts; triples and hierarchies beyond what bound hints at (bound[i] >= 2); orbital
 * elements on the device (semi-major axis, eccentricity and period of the pairs found are a few operations per PAIR on the
 * host); tidal or energy thresholds ("hard" and "soft" binaries: a choice of the caller's, made on energy[]); device pointers
 * for the results; hipGraph replay; a command-line word or an environment knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_BINARIES_H
#define NBX_BINARIES_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_binaries(nbx_ctx* c,
                 int32_t* partner, void* energy, int32_t* bound /* [n] or NULL */);
int nbx_ensemble_binaries(nbx_ensemble* e, int32_t first, int32_t count,
                          int32_t* partner, void* energy, int32_t* bound /* [count * n] or NULL */);
int nbx_ragged_binaries(nbx_ragged* r, int32_t first, int32_t count,
                        int32_t* partner, void* energy, int32_t* bound /* members end to end, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_BINARIES_H */
