/*
 * nbx_knn.h -- the k nearest neighbours of every body: for every body of the resident system its k closest partners and the
 * softened squared distances to them, evaluated on the device from the resident state, for a context, for any range of an
 * ensemble's members or for any range of a ragged ensemble's members in one call.  Kept apart from the other headers, whose
 * symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via
 * nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: nbx_neighbours answers "who is my closest partner".  The structural diagnostics of a direct-sum cluster code need the
 * k-th neighbour: the local density estimator rho_k of Casertano & Hut (k = 6 by convention), the density centre every
 * Lagrangian-radius and core-collapse analysis takes as its origin, the core radius, and triple and hierarchy candidates (the
 * second and third neighbour).  Without this call that is a download and an O(n^2) host search with a partial sort per system,
 * the host-bound pattern the batch calls exist to remove; for the members of a batch object there is no on-device way at all.
 *
 * Definition, for body i of a system of n bodies, T the object's precision, 1 <= k <= NBX_KNN_MAX:
 *     r2(i, j)         = |x_j - x_i|^2 + eps^2, softened, eps^2 the library's (1e-3f, widened in fp64): nbx_neighbours.h's r2
 *     row i            = the k partners j < n, j != i that are smallest under the lexicographic order (r2 bits, j), listed
 *                        ascending in that order
 *     index[i * k + q] = the q-th partner of body i
 *     r2[i * k + q]    = its r2, in T (a host array of float for 32, of double for 64)
 * The layout is body-major: the k entries of a body are adjacent.  A body with fewer than k partners (n - 1 < k) has its
 * remaining entries filled with index = -1, r2 = +infinity; a system of one body is all fill.  Which pairs count: j == i is
 * excluded exactly, and records at or beyond n -- the zero padding of the position buffer -- are excluded exactly, by a mask
 * and not as a by-product, as in nbx_neighbours.h: a padding record sits at the origin and would otherwise be somebody's
 * neighbour.  Two DISTINCT bodies at one position count, with r2 = eps^2.
 *
 * Per-pair arithmetic, in T, one inline device function for all three kinds of object:
 *     dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))        (nbx_neighbours.h's r2, restated)
 * then one strict compare against the body's current k-th value; only a pair that passes it is inserted into the body's sorted
 * list.  No square root, no reciprocal, no multiply.
 * Consequences:
 *     column 0 of a k = 1 call, and of a call with any k, is bit for bit nbx_neighbours' index and r2;
 *     the result for k is bit for bit the first k columns of the result for any k' > k;
 *     rows are non-decreasing in r2, and strictly increasing in j among equal r2;
 *     #(r2[i, :] <= h2) == min(within[i], k) with nbx_neighbours' h2 and within;
 *     r2(i, j) and r2(j, i) are the same bits.
 *
 * Nothing is summed in floating point: a row is a selection under a total order.  So the same state gives the same bits on
 * every call, for every launch shape, for every compiled list capacity and whatever the context's kernel variant, summation
 * order, bodies per lane or j split; and a member's results are bit for bit what nbx_knn returns for a context of n bodies
 * holding that member's state, whatever range it was asked in and wherever the member lies.
 *
 * Arrays: index or r2 may be NULL; a NULL array is never written.  If both are NULL the arguments are checked and nothing is
 * launched.  k is checked always.  The layout across systems is that of the object's download call: an ensemble is
 * member-major, count * n rows of k; a ragged ensemble has its members end to end, member `first` at row 0.
 *
 * Contexts: a sliced context (i_count < n) is accepted and returns all n bodies, what the whole context returns, because all n
 * positions are resident in it.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_neighbours: the call is ordered on the object's stream -- after an asynchronous step call it
 * describes the state after those steps -- and synchronises once.  One pair-work launch, one finish launch and one read-back
 * serve the whole range; no atomics.  It reads the current position buffer only and writes only buffers of its own (allocated
 * on first use, grown when a larger call arrives, freed with the object).  Untouched: positions, velocities, which position
 * buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    k < 1 or k > NBX_KNN_MAX (checked even when both outputs are NULL)
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- times k exceed 2^22 = 4194304:
 *                  the bound of nbx_field.h scaled by the row width, which keeps the partial rows (bodies x splits x k
 *                  records) at the scratch size the neighbours call may already reach.  A context of more bodies is served
 *                  with a smaller k (1M bodies: k <= 4)
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         count == 0 or both of index, r2 NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a body with a coordinate that is not finite, or whose r2 overflows T for every partner, gives
 * unspecified values for that body, and that body is missing from the rows of the others: r2 to it is NaN or +infinity, which
 * no strict compare against a row's +infinity passes.  Where k < n - 1 the other rows are then the rows of the system without
 * it; where k >= n - 1 they end one entry early, index -1 and r2 +infinity where the body would have stood.  No other entry of
 * another body's row changes, and other systems of the call are not touched.
 *
 * Cost: the pair loop compares every pair once and inserts rarely: for bodies in no particular order a body sees about
 * k ln(n / k) insertions.  Bodies sorted by decreasing distance from a body make that body insert at every pair: the result
 * is the same, the call is slower.
 *
 * Deliberately not here: groups; device pointers for the results; k > 16; variable-length neighbour lists; an i range for a
 * context; a radius cut-off; mass-weighted selection; hipGraph replay; a command-line word or an environment knob in nbody.x
 * (its output is the reference's).
 */
#ifndef NBX_KNN_H
#define NBX_KNN_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NBX_KNN_MAX 16

int nbx_knn(nbx_ctx* c, int32_t k, int32_t* index, void* r2 /* [n][k] or NULL */);
int nbx_ensemble_knn(nbx_ensemble* e, int32_t first, int32_t count, int32_t k,
                     int32_t* index, void* r2 /* [count * n][k] or NULL */);
int nbx_ragged_knn(nbx_ragged* r, int32_t first, int32_t count, int32_t k,
                   int32_t* index, void* r2 /* members end to end, [bodies][k], or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_KNN_H */
