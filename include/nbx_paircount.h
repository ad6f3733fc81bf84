/*
 * nbx_paircount.h -- how the bodies are distributed in separation: N(<r), the number of pairs of the resident system closer than
 * r, for a whole list of radii in one pass over the pairs, evaluated on the device from the resident state, for a context, for
 * any range of an ensemble's members or for any range of a ragged ensemble's members in one call.  Kept apart from the other
 * headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int
 * status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: the radial pair-count function is the standard first look at a system's structure; its differences are the
 * pair-separation histogram, from which g(r), the two-point correlation and the clustering of an ensemble's members follow.
 * nbx_neighbours counts within ONE radius per body: B radii cost B passes over the pairs and B synchronisations plus a host sum;
 * the alternative is a download and an O(n^2) host loop.  Both are the launch-bound and host-bound pattern the batch calls exist
 * to remove.
 *
 * Definition, for a system of n bodies, T the object's precision:
 *     r2(i, j)  = |x_j - x_i|^2 + eps^2, softened, eps^2 the library's (1e-3f, widened in fp64): exactly nbx_neighbours.h's r2,
 *                 in T,  dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))
 *     h2_k      = fma(rT, rT, eps2) evaluated once on the host in T, rT = (T)radii[k]: the rule of nbx_neighbours' within
 *     counts[k] = #{ (i, j) : i < j < n,  r2(i, j) <= h2_k }
 * Radii may come in any order and may repeat; +infinity is allowed and gives n (n - 1) / 2.  A system of one body has all zeros.
 * Which pairs count: j == i is excluded exactly, and records at or beyond n -- the zero padding of the position buffer -- are
 * excluded exactly, by a mask on the result of the compare and not as a by-product: with h2 = +infinity nothing done to r2 would
 * keep them out.  Two DISTINCT bodies at one position count, with r2 = eps^2, so radius 0 counts the coincident pairs.
 *
 * Consequences:
 *     counts[k] is exactly half the sum over i of within[i] that nbx_neighbours returns at radii[k] on the same object (that sum
 *     is even, because r2(i, j) and r2(j, i) are the same bits);
 *     counts are monotone in the radius;
 *     for ascending radii the differences of counts are the pair-separation histogram.
 *
 * Nothing is summed in floating point: the count is an integer sum of one predicate.  So the same state gives the same bits on
 * every call, for every launch shape and whatever the context's kernel variant, summation order, bodies per lane or j split;
 * a member's counts are bit for bit what nbx_paircount returns for a context of n bodies holding that member's state, whatever
 * range it was asked in.  The device walks the full square of ordered pairs and halves the total, which is exact; walking the
 * triangle i < j alone would halve the work but unbalance the j splits: a follow-up, not done here.
 *
 * Arrays: radii is a host array of nradii doubles, counts a host array of uint64: nradii for a context, count * nradii
 * member-major for an ensemble and for a ragged ensemble (member `first` at element 0).  If counts is NULL the arguments are
 * checked and nothing is launched.
 *
 * Contexts: a sliced context (i_count < n) is accepted and returns the whole context's counts, because all n positions are
 * resident in it.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_neighbours: the call is ordered on the object's stream -- after an asynchronous step call it describes
 * the state after those steps -- and synchronises once.  ceil(nradii / 16) pair-work launches back to back (16 radii are held
 * as uniform kernel arguments per pass), one finish launch and one read-back serve the whole range; no atomics.  It reads the
 * current position buffer only and writes only buffers of its own (allocated on first use, grown when a larger call arrives,
 * freed with the object).  Untouched: positions, velocities, which position buffer is current, steps_done, every *_timed /
 * *_ms_total field, the kinetic-energy partials and the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    nradii is outside [1, NBX_PAIRCOUNT_MAX_RADII], or radii is NULL
 *   NBX_ERR_ARG    some radius is NaN or negative; the text names the first such k
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304: the
 *                  bound of nbx_neighbours.h.  It is also what keeps a workgroup's partial count in 32 bits: 512 bodies of a
 *                  workgroup times at most 2^22 partners is 2^31.  The counts themselves are 64 bits.
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         count == 0 or counts NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a body with a coordinate that is not finite gives unspecified counts for the pairs it is part of.
 *
 * Deliberately not here: groups; device pointers; per-body profiles (within at many radii per body); mass weighting;
 * cross-counts between two members; the triangular half of the pair square (above); hipGraph replay; a command-line word or an
 * environment knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_PAIRCOUNT_H
#define NBX_PAIRCOUNT_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NBX_PAIRCOUNT_MAX_RADII 256

int nbx_paircount(nbx_ctx* c, int32_t nradii, const double* radii, uint64_t* counts /* [nradii] */);
int nbx_ensemble_paircount(nbx_ensemble* e, int32_t first, int32_t count, int32_t nradii, const double* radii,
                           uint64_t* counts /* [count * nradii], member-major */);
int nbx_ragged_paircount(nbx_ragged* r, int32_t first, int32_t count, int32_t nradii, const double* radii,
                         uint64_t* counts /* [count * nradii], member `first` at element 0 */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_PAIRCOUNT_H */
