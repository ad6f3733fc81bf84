/*
 * nbx_field.h -- the field of the resident system at points of the caller's choosing: the softened acceleration and the
 * softened potential at m host-supplied points, evaluated on the device from the resident state, for a context, for any range of
 * an ensemble's members or for any range of a ragged ensemble's members in one call.  Kept apart from the other headers, whose
 * symbol sets and structs stay as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via
 * nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: every other entry point that evaluates gravity does so at the resident bodies' own positions.  Tracers and test
 * particles, potential or force maps on a grid, the escape speed at a point, the per-body potential that nbx_batch_accel.h lists
 * under "Deliberately not here", an integrator of the caller's own that needs forces at trial positions: all ask for the field
 * somewhere else.  The workaround -- a second context of n + m bodies with the points appended as massless bodies, an upload
 * and nbx_accel -- costs O((n + m)^2) pairs where O(n m) are wanted, gives no potential and does not exist for members at all.
 *
 * Definition, for a point p and a system of n bodies:
 *     a(p)   =   sum over j < n of G m_j (x_j - p) / (|x_j - p|^2 + eps^2)^(3/2)
 *     phi(p) = - sum over j < n of G m_j / sqrt(|x_j - p|^2 + eps^2)
 * eps^2 and G are the library's (1e-3f and 6.67259e-11f, widened in fp64); G m_j is the value nbx_upload stored in the body's
 * position record, G times m rounded once in the object's precision.  EVERY body counts: there is no self-exclusion, because a
 * point is not a body.  A point that coincides with body i gets a zero acceleration term from it, since the delta is zero, and
 * the potential term -G m_i / eps.  Hence two identities:
 *     a(x_i) is body i's acceleration;
 *     phi(x_i) + G m_i / eps is body i's potential, so 1/2 sum_i m_i (phi(x_i) + G m_i / eps) is nbx_diag_t.potential.
 * Records at or beyond n -- the zero padding of the position buffer -- have G m = 0 and a finite softened distance, so they
 * contribute exactly nothing to either sum.  Here that is sufficient and no mask is needed; nbx_timescale.h needs one because
 * its approach rate does not carry the mass as a factor: a padding record has a position and would still produce a rate.
 *
 * Arrays: points and results are host SoA arrays in the object's precision (float for 32, double for 64).  A batch kind gives
 * every member of the range its own m points: member first + k uses elements [k m, (k + 1) m) of every array, for ensembles
 * and ragged ensembles alike.  Any of ax, ay, az, phi may be NULL; a NULL array is never written.  If all four are NULL the
 * arguments are checked and nothing is launched.
 *
 * Per-pair arithmetic, in the object's precision T, one inline device function for all three kinds of object:
 *     dx,dy,dz = x_j - p;  r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))        (the force kernels' r2)
 *     s = G m_j r2^(-3/2) as the force kernels form it (gm_inv_cube);  a += d s (fma);  sum += G m_j r2^(-1/2) (fma)
 * fp32: the hardware's reciprocal square root, within 1 ulp.  fp64: the hardware's seed corrected to second order in its
 * residual, the residual shared by the cube and the inverse; the power-of-two scales the fp64 records carry are undone exactly.
 * A point's four sums are kept in T over the bodies of one j split, j ascending; the splits' partial sums are added in fp64 in
 * split order and rounded once to T; phi takes its minus sign there.  This is not the reference's summation order.
 *
 * The launch shape -- 512 points per workgroup column, 256 bodies per tile, the number of j splits -- is a function of (m, n)
 * alone, never of the device or of the object's options.  So the same state, the same points and the same m give the same bits
 * on every call and on every object that holds them: a member's results are bit for bit what nbx_field returns for a context of
 * n bodies holding that member's state and given the same m points, whatever range the member was asked in, and a context that
 * owns a slice [i_begin, i_begin + i_count) returns what the whole one returns.
 *
 * Contexts: a sliced context (i_count < n) is accepted, because all n positions are resident in it.  A context with a local step
 * awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_timescale: the call is ordered on the object's stream -- after an asynchronous step call it
 * describes the state after those steps -- and synchronises once.  One upload of the points, one pair-work launch, one finish
 * launch and one read-back serve the whole range; no atomics.  It reads the current position buffer and writes only buffers of
 * its own (allocated on first use, grown when a larger call arrives, freed with the object).  Untouched: positions,
 * velocities, which position buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials and
 * the state of graph replay.
 *
 * Status, in this order:
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    m < 0
 *   NBX_ERR_ARG    m > 0 and any of px, py, pz is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members)
 *   NBX_ERR_ARG    (int64) count * m > 2^22 = 4194304 (a context: m > 2^22): the bound that keeps the row indices of the
 *                  partials in 32 bits and the scratch below 1 GiB
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         m == 0, count == 0 or all of ax, ay, az, phi NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a coordinate of a point that is not finite, or whose square overflows T, gives unspecified values for
 * that point only.
 *
 * Deliberately not here: groups; device pointers for points or results; jerk; self-exclusion by index (take the identities
 * above); the reference summation order; hipGraph replay; a command-line word or an environment knob in nbody.x (its output is
 * the reference's).  This list used to say "tidal tensors or jerk": the tidal tensor, the second derivative of the potential
 * at points or at the bodies, is now nbx_tidal.h; jerk stays out.
 */
#ifndef NBX_FIELD_H
#define NBX_FIELD_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_field(nbx_ctx* c, int32_t m, const void* px, const void* py, const void* pz, /* [m] */
              void* ax, void* ay, void* az, void* phi /* [m] or NULL */);
int nbx_ensemble_field(nbx_ensemble* e, int32_t first, int32_t count, int32_t m,
                       const void* px, const void* py, const void* pz, /* [count * m] */
                       void* ax, void* ay, void* az, void* phi /* [count * m] or NULL */);
int nbx_ragged_field(nbx_ragged* r, int32_t first, int32_t count, int32_t m,
                     const void* px, const void* py, const void* pz, /* [count * m] */
                     void* ax, void* ay, void* az, void* phi /* [count * m] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_FIELD_H */
