/*
 * nbx_neighbours.h -- who is next to whom: for every body of the resident system its nearest neighbour, the softened squared
 * distance to it and the number of bodies within a radius, evaluated on the device from the resident state, for a context, for
 * any range of an ensemble's members or for any range of a ragged ensemble's members in one call.  Kept apart from the other
 * headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int
 * status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: the other analysis calls answer whole-system questions with sums or extremes (nbx_diagnostics, nbx_timescale) or give a
 * body a sum over all others (nbx_accel, nbx_field).  None says which bodies are close to each other: nbx_timescale finds that
 * SOME pair is at min_r2, not which one.  Users of small chaotic systems ask about close encounters and hard binaries: which
 * body is each body's nearest neighbour, which two bodies are mutual nearest neighbours (binary or collision candidates), how
 * many bodies lie within a radius of each body (local density, crowding).  Without this call that is a download and an O(n^2)
 * host search per system, the launch-bound and host-bound pattern the batch calls exist to remove.
 *
 * Definition, for body i of a system of n bodies, T the object's precision:
 *     r2(i, j)  = |x_j - x_i|^2 + eps^2, softened, eps^2 the library's (1e-3f, widened in fp64)
 *     index[i]  = the j < n, j != i with the smallest r2(i, j); among equal bit patterns the LOWEST j
 *     r2[i]     = that smallest value, in T (a host array of float for 32, of double for 64)
 *     within[i] = the number of j < n, j != i with r2(i, j) <= h2,  h2 = fma(rT, rT, eps2) evaluated once on the host in T,
 *                 rT = (T)radius
 * A system of one body has index = -1, r2 = +infinity, within = 0.  Which pairs count: j == i is excluded exactly, and records
 * at or beyond n -- the zero padding of the position buffer -- are excluded exactly, by a mask and not as a by-product, as in
 * nbx_timescale.h: a padding record sits at the origin and would otherwise be somebody's nearest neighbour.  Two DISTINCT
 * bodies at one position count, with r2 = eps^2.
 *
 * Per-pair arithmetic, in T, one inline device function for all three kinds of object:
 *     dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))        (the force kernels' and nbx_timescale's r2)
 * then a strict compare against the running minimum and a compare against h2; no square root, no reciprocal, no multiply.
 * Consequences:
 *     the subtraction is exact under i <-> j up to sign and the squares do not see the sign, so r2(i, j) and r2(j, i) are the
 *     same bits;
 *     if index[i] == j then r2[j] <= r2[i];
 *     the minimum over i of r2[i] is bit for bit nbx_timescale_t.min_r2;
 *     index[i] == j && index[j] == i identifies a mutual pair.
 * To first order r2 is within 5u of the exact value, u the unit round-off of T.
 *
 * Nothing is summed in floating point: the nearest neighbour is a minimum with a lowest-index tie-break, the count an integer
 * sum.  So the same state gives the same bits on every call, for every launch shape and whatever the context's kernel variant,
 * summation order, bodies per lane or j split; and a member's results are bit for bit what nbx_neighbours returns for a context
 * of n bodies holding that member's state, whatever range it was asked in.
 *
 * Arrays: any of index, r2, within may be NULL; a NULL array is never written.  If all three are NULL the arguments are checked
 * and nothing is launched.  radius is used only for within, but is checked always; callers who pass within == NULL do not pay
 * for the count.  The layout is that of the object's download call: an ensemble is member-major, count * n elements; a ragged
 * ensemble has its members end to end, member `first` at element 0.
 *
 * Contexts: a sliced context (i_count < n) is accepted and returns all n bodies, what the whole context returns, because all n
 * positions are resident in it.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_field and nbx_timescale: the call is ordered on the object's stream -- after an asynchronous step
 * call it describes the state after those steps -- and synchronises once.  One pair-work launch, one finish launch and one
 * read-back serve the whole range; no atomics.  It reads the current position buffer only and writes only buffers of its own
 * (allocated on first use, grown when a larger call arrives, freed with the object).  Untouched: positions, velocities, which
 * position buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and the state of graph
 * replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    radius is NaN or negative
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304: the
 *                  bound of nbx_field.h, which keeps the row indices of the partials in 32 bits and the scratch below 1 GiB
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         count == 0 or all of index, r2, within NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a body with a coordinate that is not finite, or whose r2 overflows T for every partner, gives
 * unspecified values for that body, and that body is nobody's nearest neighbour and within no finite radius of anybody: r2 to it is
 * NaN or +infinity.  The other bodies' values are those of the system without it -- for n == 2, index -1, r2 +infinity and within 0.
 * Other systems of the call are not touched.
 *
 * Deliberately not here: groups; device pointers for the results; k > 1 neighbours; a neighbour list (variable length);
 * relative velocities and bound or unbound tests (the arithmetic of nbx_timescale.h); merging bodies; hipGraph replay; a
 * command-line word or an environment knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_NEIGHBOURS_H
#define NBX_NEIGHBOURS_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_neighbours(nbx_ctx* c, double radius,
                   int32_t* index, void* r2, int32_t* within /* [n] or NULL */);
int nbx_ensemble_neighbours(nbx_ensemble* e, int32_t first, int32_t count, double radius,
                            int32_t* index, void* r2, int32_t* within /* [count * n] or NULL */);
int nbx_ragged_neighbours(nbx_ragged* r, int32_t first, int32_t count, double radius,
                          int32_t* index, void* r2, int32_t* within /* members end to end, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_NEIGHBOURS_H */
