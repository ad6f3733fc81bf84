/*
 * nbx_clumps.h -- which bodies are bound to their group, and how tightly: for every body of the resident system, under a label
 * the caller supplies, the members, mass, centre of mass and mean velocity of its clump, the potential of the clump's OTHER
 * members at the body and the body's specific energy in the clump's centre-of-mass frame, evaluated on the device from the
 * resident state, for a context, for any range of an ensemble's members or for any range of a ragged ensemble's members in one
 * call.  Kept apart from the other headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does not change);
 * same conventions: plain C, int status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: nbx_fof says which bodies belong together geometrically, nbx_binaries which PAIRS are bound, nbx_tidal gives the tidal
 * radius "of an nbx_fof group" -- and nothing said whether a group is bound or which of its members are bound to it.  This header
 * supplies what nbx_fof.h lists under "Deliberately not here" as bound or unbound tests.  nbx_field cannot: it sums over every
 * resident body, not over a group's members, and at a body it includes the body's own term G m_i / eps; nbx_diagnostics gives one
 * potential energy per system.  The restricted self-potential of every group and each member's energy in the group's frame are
 * the unbinding step of every halo or cluster finder, the test for subclumps, fragments and ejected multiples, and the source of
 * the mass, centre and velocity that tidal() and tidal_radius() ask for.  Without this call that is a download and an O(n^2) host
 * search per system, the launch-bound and host-bound pattern the batch calls exist to remove.
 *
 * Definition, for body i of a system of n bodies, T the object's precision, gm_j the value nbx_upload stored in body j's position
 * record (G times m rounded once in T), r2(i, j) = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2))) the force kernels' r2:
 *     label       is the caller's, int32 per body, one upload per call as nbx_field's points are.  Any value >= 0 is a clump
 *                 name -- values >= n and above 2^24 included; labels are compared AS INTEGERS and never pass through a
 *                 floating-point value.  A negative label means "in no clump".
 *     c(i)        = { j < n : label[j] == label[i] } if label[i] >= 0, else empty
 *     members[i]  = |c(i)|
 *     gm[i]       = sum over c(i) of gm_j
 *     centre[i]   = sum over c(i) of gm_j x_j / gm[i]
 *     velocity[i] = sum over c(i) of gm_j v_j / gm[i]
 *     phi[i]      = - sum over j in c(i), j != i, of gm_j / sqrt(r2(i, j))
 *     energy[i]   = |v_i - velocity[i]|^2 / 2 + phi[i]
 * j == i is never formed in phi; it is counted in the other sums.  Records at or beyond n never count.  A body with a negative
 * label returns members = 0 and zeros everywhere else, contributes to nobody, and negative labels do not match each other.  A
 * clump of one body returns its centre as the body's position and its velocity as the body's velocity, exactly, phi = 0 and
 * energy = 0.  Where gm == 0 with several members, centre and velocity are 0.
 *
 * Arithmetic.  Per pair, in T: g = (label_j == label_i) ? gm_j : 0 -- one integer compare and one select --, inv = rsq(r2), and
 * eight sums per body over the records of one j split, j ascending: S += g inv (fma), M += g, P_a += g v_ja (fma), X_a += g x_ja
 * (fma), and the integer count.  rsq is the force kernels' reciprocal square root (fp32: the hardware's, within 1 ulp; fp64: the
 * hardware's seed and one Newton step).  The kernels carry exact power-of-two scales through the sums (the fp64 records' G m / 8,
 * rsq's 2 / sqrt) and undo them once per body.  The finish adds the splits in fp64 in split order, forms P / M and X / M in fp64,
 * rounds centre and velocity once to T, evaluates energy in fp64 from the UNROUNDED quotients and rounds once.
 *
 * Every member of a clump recomputes the clump's mass, momentum and moment: the sequence of g it sees is the same for every
 * member, so all members of a clump return the SAME BITS for members, gm, centre and velocity; a bijective renaming of the
 * labels changes no bit of any result.  No atomics, no sort, no second pass.
 *
 * Error of one term, to first order, u the unit round-off of T.  g inv: the product inside the fma is not rounded; r2 carries
 * 5u (nbx_neighbours.h) of which rsq passes on half, and rsq adds its own: 2u in fp32, in fp64 3/2 d^2 + 3u for a seed of
 * relative error d, 51u at d = 2^-24 (nbx_binaries.h).  So one term of phi carries 4.5u in fp32 and up to 53.5u in fp64; the
 * terms of M, P and X carry none (g v and g x are not rounded inside the fma), their error is that of the sums alone.  A
 * quotient X / M carries the relative errors of both sums against sum gm_j |x_j| / gm; energy carries those of velocity
 * through (|v_i| + W)^2 / 2, W_a = sum gm_j |v_ja| / gm, and that of phi.
 *
 * The same state and labels give the same bits on every call; a member's results are bit for bit what nbx_clumps returns for a
 * context of n bodies holding that member's state and labels, whatever range it was asked in, wherever the member sits in its
 * object and whatever the context's options.
 *
 * Arrays: every pointer of nbx_clumps_out_t may be NULL; a NULL array is never written.  If all are NULL the arguments are
 * checked and nothing is launched.  members is int32; the others are host arrays of float for 32, of double for 64.  The layout
 * of label and of every result is that of the object's download call: an ensemble is member-major, count * n elements; a ragged
 * ensemble has its members end to end, member `first` at element 0.  Labels are member-local: equal values in two members do not
 * meet.
 *
 * Contexts: a sliced context (i_count < n) is refused -- the velocities of the other bodies are not resident in it: the
 * restriction nbx_binaries, nbx_timescale and nbx_step have.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_binaries: the call is ordered on the object's stream -- after an asynchronous step call it describes
 * the state after those steps -- and synchronises once.  One label upload, one pair-work launch, one finish launch and one
 * read-back serve the whole range.  It reads the current position buffer and the velocities and writes only buffers of its own
 * (allocated on first use, grown when a larger call arrives, freed with the object).  Untouched: positions, velocities, which
 * position buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and the state of graph
 * replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    label or out is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^22 = 4194304
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_ERR_STATE  a context does not own all n bodies (the velocities of the others are not resident)
 *   NBX_OK         count == 0 or every pointer of out NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a body with a coordinate, a velocity component or a mass that is not finite -- whatever its label, a
 * negative one included -- gives unspecified values for EVERY body of its system: a record that does not match enters the sums
 * as 0 times its values, and 0 times a value that is not finite is not 0.  The other systems of the call are not touched.
 *
 * Deliberately not here: groups and sliced contexts; finding the clumps (nbx_fof, or any labelling of the caller's); the
 * iteration that removes unbound members (a few calls of this one; nbx.unbind in Python); an external tidal field or a
 * background potential in energy; device pointers for labels or results; hipGraph replay; a command-line word or an environment
 * knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_CLUMPS_H
#define NBX_CLUMPS_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbx_clumps_out_t { /* every pointer may be NULL; a NULL array is never written */
  int32_t* members;               /* bodies in i's clump, i included */
  void* gm;                       /* G * mass of i's clump, in T */
  void* centre[3];                /* its centre of mass */
  void* velocity[3];              /* its mass-weighted mean velocity */
  void* phi;                      /* i's potential from the OTHER members of its clump */
  void* energy;                   /* i's specific energy in the clump's frame */
} nbx_clumps_out_t;

int nbx_clumps(nbx_ctx* c, const int32_t* label /* [n] */, const nbx_clumps_out_t* out);
int nbx_ensemble_clumps(nbx_ensemble* e, int32_t first, int32_t count,
                        const int32_t* label /* [count * n] */, const nbx_clumps_out_t* out);
int nbx_ragged_clumps(nbx_ragged* r, int32_t first, int32_t count,
                      const int32_t* label /* members end to end */, const nbx_clumps_out_t* out);

#ifdef __cplusplus
}
#endif
#endif /* NBX_CLUMPS_H */
