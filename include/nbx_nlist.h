/*
 * nbx_nlist.h -- who is within a radius of whom, as a list: for every body of the resident system the indices of ALL bodies
 * within a radius and the softened squared distances to them, evaluated on the device from the resident state, for a context,
 * for any range of an ensemble's members or for any range of a ragged ensemble's members in one call.  Kept apart from the other
 * headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int
 * status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: nbx_neighbours and nbx_paircount say HOW MANY bodies lie within a radius, nbx_knn names the closest 16 at most, nbx_fof
 * names the connected component.  None returns WHICH bodies are within the radius.  Collision and merger candidates, a local
 * velocity dispersion or an SPH-style density with the caller's own kernel, every pair closer than r for a regularised
 * integrator, the edges of the friends-of-friends graph: all need the list, and without this call that is a download and an
 * O(n^2) host search per system.
 *
 * Definition, for body i of a system of n bodies, T the object's precision (nbx_neighbours.h's, restated):
 *     r2(i, j)  = |x_j - x_i|^2 + eps^2, softened, eps^2 the library's (1e-3f, widened in fp64); per pair, in T,
 *                 dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))
 *     h2        = fma(rT, rT, eps2) evaluated once on the host in T, rT = (T)radius
 *     list(i)   = every j < n, j != i with r2(i, j) <= h2, in ASCENDING j
 * j == i is excluded exactly, and records at or beyond n -- the zero padding of the position buffer -- are excluded exactly, by
 * a mask and not as a by-product.  Two DISTINCT bodies at one position count, with r2 = eps^2.  radius = +infinity is allowed:
 * every list is all the other bodies.
 *
 * Layout: b is the body's place in the call's output order, the object's download layout: member-major for an ensemble
 * (b = k * n + i for member first + k), members end to end for a ragged ensemble, member `first` at 0.  Then
 *     index[offsets[b] .. offsets[b + 1])   the list of body b; j is MEMBER-LOCAL (0 <= j < the member's n)
 *     r2[...]                               the pair's r2 in T at the same place (a host array of float for 32, of double for 64)
 *     offsets[0] = 0,  offsets[bodies] = *total;  offsets run across the members of a range
 *
 * The two-call protocol.  The size of the result depends on the state, so the caller states what its arrays hold:
 *     offsets [bodies + 1] and *total are ALWAYS written; both are required (non-NULL);
 *     the lists are written if and only if *total <= capacity.  Otherwise index and r2 are not touched, the call returns NBX_OK,
 *     and the caller sizes its arrays from *total and calls again;
 *     capacity == 0 with index and r2 both NULL is the counting call;
 *     with capacity > 0 either of index and r2 may be NULL; a NULL array is never written.
 *
 * Consequences, all integer or bit-exact:
 *     offsets[b + 1] - offsets[b] equals nbx_neighbours' within[b] at the same radius;
 *     *total is twice nbx_paircount at that radius;
 *     j in list(i) <=> i in list(j), with the same r2 bits (the subtraction is exact under i <-> j up to sign and the squares do
 *     not see the sign);
 *     where within[i] > 0, the entry of list(i) with the smallest (r2, j) is nbx_neighbours' index[i] and r2[i];
 *     where within[i] <= k, list(i) as a set is the first within[i] columns of nbx_knn(k), with r2 bit for bit;
 *     the connected components of the graph whose edges are the lists are nbx_fof's partition at that radius.
 * Nothing is summed in floating point: a list is a set of pairs decided by one compare each, written in index order, and the
 * offsets are integer sums.  So the same state gives the same bits on every call, for every launch shape and whatever the
 * context's kernel variant, summation order, bodies per lane or j split; a member's lists are bit for bit what nbx_nlist returns
 * for a context of n bodies holding that member's state, whatever range it was asked in and wherever the member lies; a sliced
 * context (i_count < n) returns the whole context's lists, because all n positions are resident in it.
 *
 * Semantics, otherwise those of nbx_neighbours: the call is ordered on the object's stream -- after an asynchronous step call
 * it describes the state after those steps.  A counting call is one pair-work launch, four small launches (a finish and a 64-bit
 * prefix sum on the device, two levels of 2048) and one synchronisation; a filling call adds a second pair-work launch, which
 * decides every pair with the same function on the same bits, and a second synchronisation.  No atomics, and no kernel waits for
 * another workgroup.  It reads the current position buffer only and writes only buffers of its own (allocated on first use,
 * grown when a larger call arrives, the device lists sized by *total and never by capacity, freed with the object).  Untouched:
 * positions, velocities, which position buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy
 * partials, the profile and the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    radius is NaN or negative
 *   NBX_ERR_ARG    capacity < 0 or capacity > 2^28 = 268435456: the bound keeps the device lists -- 4 bytes of index and, in
 *                  fp64, 8 bytes of r2 per entry -- at or below 3 GiB
 *   NBX_ERR_ARG    capacity > 0 with index and r2 both NULL, or offsets or total NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304: the
 *                  bound of nbx_field.h; it is also exactly what the two-level prefix sum serves, 2048 blocks of 2048 bodies
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         count == 0: offsets[0] = 0 and *total = 0, nothing is launched
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.  After a failure the contents of the caller's arrays are unspecified.
 *
 * Unspecified results: a body with a coordinate that is not finite gives unspecified lists for that body and for the lists it
 * would appear in.
 *
 * Deliberately not here: groups; device pointers for the results; a radius per body; half lists (i < j only: nbx.py's
 * nlist_pairs makes them on the host); velocities in the list; merging bodies; hipGraph replay; a command-line word or an
 * environment knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_NLIST_H
#define NBX_NLIST_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_nlist(nbx_ctx* c, double radius, int64_t capacity,
              int64_t* offsets /* [n + 1] */, int32_t* index /* [capacity] or NULL */,
              void* r2 /* [capacity] of T, or NULL */, int64_t* total);
int nbx_ensemble_nlist(nbx_ensemble* e, int32_t first, int32_t count, double radius, int64_t capacity,
                       int64_t* offsets /* [count * n + 1] */, int32_t* index, void* r2, int64_t* total);
int nbx_ragged_nlist(nbx_ragged* r, int32_t first, int32_t count, double radius, int64_t capacity,
                     int64_t* offsets /* [bodies of the range + 1] */, int32_t* index, void* r2, int64_t* total);

#ifdef __cplusplus
}
#endif
#endif /* NBX_NLIST_H */
