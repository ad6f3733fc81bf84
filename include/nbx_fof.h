/*
 * nbx_fof.h -- which bodies belong together: the friends-of-friends (FoF) groups of the resident system, evaluated on the device
 * from the resident state, for a context, for any range of an ensemble's members or for any range of a ragged ensemble's members
 * in one call.  Kept apart from the other headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not
 * change); same conventions: plain C, int status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: nbx_neighbours, nbx_paircount and nbx_knn answer per-body proximity questions -- who is closest, how many lie within a
 * radius, how the pairs are distributed in separation, the k closest partners.  None says which bodies belong TOGETHER, and a
 * caller cannot build that from what they return: index and knn give at most 16 edges per body, within gives a count and not
 * the partners (nbx_neighbours.h lists a neighbour list under "deliberately not here").  Friends-of-friends is the standard tool:
 * subclumps, bound-cluster candidates, ejected binaries and triples, escapers (singletons), the number and the mass function of
 * fragments in every member of an ensemble all start from FoF labels.  Without this call that is a download and an O(n^2) host
 * search per system, the launch-bound and host-bound pattern the batch calls exist to remove.
 *
 * Definition, for a system of n bodies, T the object's precision:
 *     r2(i, j)  = |x_j - x_i|^2 + eps^2, softened, eps^2 the library's (1e-3f, widened in fp64): exactly nbx_neighbours'
 *     h2        = fma(rT, rT, eps2) evaluated once on the host in T, rT = (T)radius (the linking length)
 *     friends   i and j are friends iff i != j, both < n, and r2(i, j) <= h2
 *     group     a connected component of the friendship graph
 *     label[i]  = the LOWEST index of any body in i's group (int32; member-local for an ensemble and a ragged ensemble)
 *     size[i]   = the number of bodies in i's group (int32, >= 1)
 *     info[k]   = nbx_fof_info_t { groups, largest } of system k of the call: groups the number of groups, i.e. of bodies with
 *                 label[i] == i; largest the size of the largest group
 *     *passes   = the number of pair-work launches the call made (a scalar for the whole call)
 * A system of one body has label = 0, size = 1, groups = 1, largest = 1.  Padding records (index >= n) are never anybody's
 * friend.  Two DISTINCT bodies at one position are friends at every radius (r2 = eps^2 <= h2).
 *
 * Per-pair arithmetic, in T, one inline device function for all three kinds of object:
 *     dx,dy,dz = x_j - x_i;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))        (the force kernels' and nbx_neighbours' r2)
 * then one compare against h2, one integer minimum and one select; no square root, no reciprocal, no multiply.  Labels are
 * compared as integers and never touched by floating-point arithmetic.
 * Consequences:
 *     friendship is symmetric: r2(i, j) and r2(j, i) are the same bits;
 *     with nbx_neighbours(radius): r2[i] <= h2 implies label[i] == label[index[i]]; size[i] >= within[i] + 1; groups == n iff
 *     within is all zero;
 *     every nbx_knn partner with r2 <= h2 shares the body's label.
 *
 * How: labels L start at L[i] = i.  One PASS is (1) a pair-work launch: m[i] = min(L[i], L[j] over i's friends j), per j split;
 * (2) finish and hook: N[i] = min(L[i], m[i]) and N[L[i]] = min(N[L[i]], m[i]), N a second buffer that equals L beforehand,
 * every read from L and every write an integer atomic minimum on N; (3) shortcut: N[i] = N[N[i]] until nothing changes
 * (pointer jumping to the root); (4) the labels are restaged for the next pass and a "changed" word is set where N != L.  The
 * call ends after the first pass that changes nothing; that pass counts.  Labels only decrease, a label is always the index of
 * a body of the same group, and at a fixed point both ends of every edge carry the same label: the group's lowest-index body
 * keeps its own index and all others share it.  Paths of 4097 and 131072 bodies in random order need about 10 and 12 passes,
 * lattices and random geometric graphs 2 to 6.  For a range of members every pass is one launch of each kind over the whole
 * range and the call ends when no member changed, so passes is the largest of the members' own counts.
 *
 * A partition with lowest-index labels does not depend on the order anything is evaluated in: the same state gives the same
 * bits on every call, for every launch shape and whatever the context's kernel variant, summation order, bodies per lane or
 * j split; and a member's label and size are bit for bit what nbx_fof returns for a context of n bodies holding that member's
 * state, whatever range it was asked in.
 *
 * Arrays: any of label, size, info, passes may be NULL; a NULL array is never written.  If label, size and info are all NULL the
 * arguments are checked and nothing is launched or written (passes included).  The layout of label and size is that of the
 * object's download call: an ensemble is member-major, count * n elements; a ragged ensemble has its members end to end,
 * member `first` at element 0.  info has one element for a context and count elements otherwise.
 *
 * Contexts: a sliced context (i_count < n) is accepted and returns all n bodies, what the whole context returns, because all n
 * positions are resident in it.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_neighbours: the call is ordered on the object's stream -- after an asynchronous step call it
 * describes the state after those steps.  It synchronises once per pass (a 4-byte read-back of the "changed" word) and once for
 * the results.  It reads the current position buffer only and writes only buffers of its own (allocated on first use, grown
 * when a larger call arrives, freed with the object).  Untouched: positions, velocities, which position buffer is current,
 * steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG       the handle is NULL
 *   NBX_ERR_ARG       radius is NaN or negative
 *   NBX_ERR_ARG       members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG       the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304: the
 *                     bound of nbx_field.h, which keeps the row indices of the partials in 32 bits
 *   NBX_ERR_STATE     not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE     a context has a local step awaiting nbx_commit
 *   NBX_OK            count == 0 or all of label, size, info NULL: nothing is launched or written
 *   NBX_ERR_ALLOC     the buffers did not fit
 *   NBX_ERR_INTERNAL  more than n + 1 passes (n the largest system of the call): unreachable, labels only decrease.  The code
 *                     is defined below, nbx.h's enum stays as it is
 * Every check but the last two comes before the first HIP call.
 *
 * Unspecified results: a body with a coordinate that is not finite has no friends or unspecified ones; the other bodies' groups
 * are those of the graph without it or with it.
 *
 * Deliberately not here: groups (multi-GPU); periodic boxes; bound or unbound tests (the arithmetic of nbx_timescale.h); a
 * linking length per member; device pointers for the results; hipGraph replay; a command-line word or an environment knob in
 * nbody.x (its output is the reference's).
 */
#ifndef NBX_FOF_H
#define NBX_FOF_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NBX_ERR_INTERNAL (-5) /* an invariant of the library did not hold: a defect, not a misuse */

typedef struct nbx_fof_info_t {
  int32_t groups;  /* the number of groups of the system */
  int32_t largest; /* the size of its largest group */
} nbx_fof_info_t;

int nbx_fof(nbx_ctx* c, double radius,
            int32_t* label, int32_t* size /* [n] or NULL */, nbx_fof_info_t* info /* one, or NULL */, int32_t* passes /* or NULL */);
int nbx_ensemble_fof(nbx_ensemble* e, int32_t first, int32_t count, double radius,
                     int32_t* label, int32_t* size /* [count * n] or NULL */, nbx_fof_info_t* info /* [count] or NULL */,
                     int32_t* passes /* or NULL */);
int nbx_ragged_fof(nbx_ragged* r, int32_t first, int32_t count, double radius,
                   int32_t* label, int32_t* size /* members end to end, or NULL */, nbx_fof_info_t* info /* [count] or NULL */,
                   int32_t* passes /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_FOF_H */
