/*
 * nbx_tidal.h -- the tidal tensor of the resident system, the second derivative of its softened potential, at m host-supplied
 * points (points mode) or at the resident bodies themselves with each body's own term left out (bodies mode), evaluated on the
 * device from the resident state, for a context, for any range of an ensemble's members or for any range of a ragged ensemble's
 * members in one call.  Kept apart from the other headers, whose symbol sets and structs stay as they are (NBX_ABI_VERSION does
 * not change); same conventions: plain C, int status, text via nbx_last_error(), one host thread drives an object at a time.
 *
 * Why: every other call that evaluates gravity stops at the first derivative of the potential: nbx_field returns a(p) and
 * phi(p), the step kernels a(x_i).  The tidal radius of an nbx_fof group or an nbx_binaries pair, r_t = (G M / lambda_max)^(1/3);
 * whether a tracer of nbx_tracers is being stretched or compressed; the softened density at a point without a neighbour search,
 * tr T = -4 pi G rho_Plummer; the variational equation delta a = T delta x: all need the second derivative.  The workaround, six
 * more nbx_field calls and central differences, trades the step h against u |a| / h and keeps about three digits in fp32, and at
 * a body the body's own softened term dominates the result and nbx_field cannot leave it out.
 *
 * Definition, for a point p and a system of n bodies, d = x_j - p, r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2))) (the force
 * kernels' r2):
 *     T_ab(p) = d a_a / d p_b = sum over j of G m_j [ 3 d_a d_b r2^(-5/2) - delta_ab r2^(-3/2) ]
 * symmetric, six components, always in the order xx, xy, xz, yy, yz, zz.  eps^2 and G are the library's (1e-3f and
 * 6.67259e-11f, widened in fp64); G m_j is the value nbx_upload stored in the body's position record, G times m rounded once in
 * the object's precision.  Records at or beyond n -- the zero padding of the position buffer -- have G m = 0 and a finite r2, so
 * they add exactly nothing and no mask is needed for them.
 *
 * Points mode (nbx_tidal, nbx_ensemble_tidal, nbx_ragged_tidal): like nbx_field.  EVERY body counts, because a point is not a
 * body; a point that coincides with body i receives the self term -G m_i / eps^3 delta_ab, since d = 0.
 * Bodies mode (nbx_tidal_bodies, nbx_ensemble_tidal_bodies, nbx_ragged_tidal_bodies): at the resident bodies themselves, the sum
 * over j != i.  The pair j == i is excluded exactly: its term is never formed into the sums, it is not subtracted afterwards.
 * With eps^2 = 1e-3 the self term is G m_i 3.2e4 and exceeds the sum of all the others unless n is large: subtracting it in T
 * would destroy the answer.  A DIFFERENT body that coincides with body i (j != i, d = 0) still counts, through its delta_ab term
 * only.
 *
 * Two identities:
 *     T_xx + T_yy + T_zz = -3 eps^2 sum over j of G m_j r2^(-5/2) <= 0       (the Plummer density: tr T = -4 pi G rho)
 *     points mode at x_i  =  bodies mode at i  -  G m_i / eps^3 delta_ab
 *
 * Arrays: points and results are host SoA arrays in the object's precision (float for 32, double for 64).  t is an array of six
 * host pointers, one per component in the order above.  Any of the six may be NULL; a NULL array is never written.  If all six
 * are NULL the arguments are checked and nothing is launched.  t itself must not be NULL.  Points mode has nbx_field's layout: a
 * batch kind gives every member of the range its own m points, member first + k uses elements [k m, (k + 1) m) of every array.
 * Bodies mode has nbx_neighbours' layout: a context n elements, an ensemble member-major, count * n elements, a ragged ensemble
 * its members end to end, member `first` at element 0.
 *
 * Per-pair arithmetic, in the object's precision T, one inline device function for all three kinds of object and both modes.  A
 * point keeps seven sums over the bodies of one j split, j ascending:
 *     s3 = G m_j r2^(-3/2) as the force kernels form it (gm_inv_cube);  s5 = G m_j r2^(-5/2)
 *     S_ab += (d_a s5) d_b (fma), six of them;   Q += s3
 * fp32: inv = the hardware's reciprocal square root, within 1 ulp; s3 = (G m inv) inv^2; s5 = s3 inv^2.  fp64: the hardware's
 * seed y, its residual h = fma(-r2, y^2, 1), the cube polynomial of nbx_field and, for the fifth power,
 * 8 (1 + 5/2 h + 35/8 h^2) = fma(h, fma(h, 35, 20), 8); the next term is 6.6 h^3 < 2^-65 for seeds good to 2^-24 (the bound
 * nbx_binaries.h had to assume); the power-of-two scale the fp64 records carry is undone exactly.  The splits' partial sums are
 * added in fp64 in split order; T_ab = 3 S_ab - delta_ab Q is formed there, in fp64, and rounded once to T.  In bodies mode the
 * record j == i enters with G m = 0, so s3 and s5 are exact zeros and every sum takes an exact zero from it.
 *
 * Error of one term, to first order, u the unit round-off of T, relative to the magnitude of the part it belongs to.  The part
 * 3 d_a d_b s5: the two differences 2 u; r2 within 5 u (nbx_neighbours.h), to the power -5/2: 12.5 u; fp32: the reciprocal
 * square root within 1 ulp <= 2 u, to the fifth power: 10 u; the roundings of inv^2 (it enters twice), G m inv, s3 and s5: 5 u;
 * d_a s5: 1 u: 30.5 u in all.  fp64: the seed's error is removed down to 2^-65, what the polynomial form costs instead is y^2
 * (twice), G m y, the two products of t3 y^2, the two fma of the polynomial and the last product, 8 u, and half a rounding of
 * y^2 that the residual does not see: 2 + 12.5 + 8.5 + 1 = 24 u.  The part delta_ab s3 stays below both (7.5 + 6 + 3 = 16.5 u in
 * fp32).  Both figures are above the 16 u floor the gates of the other pair sums use (tests/force_ref.py), so the tests of this
 * header take 30.5 u (fp32) and 24 u (fp64) as the floor of their gate: K <= 2 max(K_ref, floor), K the error in units of
 * u A_ab, A_ab = sum over j of G m_j (3 |d_a| |d_b| + delta_ab r2) r2^(-5/2), the magnitudes of the two parts every term is the
 * difference of.  The sums add their length as they do for nbx_field.
 *
 * The launch shape -- 512 points per workgroup column, 256 bodies per tile, the number of j splits -- is nbx_field's rule,
 * unchanged: field_shape(m, n) in points mode, field_shape(n, n) in bodies mode, a function of the sizes alone, never of the
 * device or of the object's options.  So the same state (and the same points and m) give the same bits on every call and on
 * every object that holds them: a member's results are bit for bit what a context of n bodies holding that member's state
 * returns, whatever range the member was asked in, and a context that owns a slice [i_begin, i_begin + i_count) returns what the
 * whole one returns.
 *
 * Contexts: a sliced context (i_count < n) is accepted in both modes, because all n positions are resident in it; in bodies mode
 * it returns all n bodies.  A context with a local step awaiting nbx_commit is refused.
 *
 * Semantics, those of nbx_field: the call is ordered on the object's stream -- after an asynchronous step call it describes the
 * state after those steps -- and synchronises once.  One upload of the points (none in bodies mode), one pair-work launch, one
 * finish launch and one read-back serve the whole range; no atomics.  It reads the current position buffer and writes only
 * buffers of its own (allocated on first use, grown when a larger call arrives, freed with the object).  Untouched: positions,
 * velocities, which position buffer is current, steps_done, every *_timed / *_ms_total field, the kinetic-energy partials, the
 * state of graph replay, the tracers and the results and buffers of the other analysis calls.
 *
 * The size bound, 2^21 = 2097152 points or bodies per call, half of nbx_field's 2^22: a point leaves two partial records per
 * split where the field leaves one.  One system of p points (p = m, or n in bodies mode) has s <= max(1, ceil(1024 / ceil(p /
 * 512))) splits by the shape rule, so p s <= 2^19 + p rows, each of two records of at most 32 bytes: at p = 2^21 that is
 * (2^19 + 2^21) 64 bytes = 160 MiB of partials, 128 MiB of results and 64 MiB of points: 352 MiB, below 1 GiB with room for the
 * splits of a few members more; at 2^22 the same sum is 672 MiB for one system alone.  The row indices stay far inside 32 bits.
 * The members of a range add their rows, at most count 2^19 + count m: count m is bounded as above, the other part only by the
 * members' sizes (a member has splits from 2048 bodies on), so a range of many large members can ask for more scratch than
 * 1 GiB or than the device has: that is NBX_ERR_ALLOC, as it is for nbx_field.
 *
 * Status of points mode, in this order (nbx_field.h's, with t in it):
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    m < 0
 *   NBX_ERR_ARG    m > 0 and any of px, py, pz is NULL
 *   NBX_ERR_ARG    t is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members)
 *   NBX_ERR_ARG    (int64) count * m > 2^21 (a context: m > 2^21)
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         m == 0, count == 0 or all six of t NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Status of bodies mode, in this order (nbx_neighbours.h's, with t in place of the radius):
 *   NBX_ERR_ARG    the handle is NULL
 *   NBX_ERR_ARG    t is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members) (checked in 64 bits)
 *   NBX_ERR_ARG    the bodies of the call -- n, (int64) count * n, or the total of the range -- exceed 2^21
 *   NBX_ERR_STATE  not uploaded; for an ensemble or a ragged ensemble the text names the first such member of the range
 *   NBX_ERR_STATE  a context has a local step awaiting nbx_commit
 *   NBX_OK         count == 0 or all six of t NULL: nothing is launched or written
 *   NBX_ERR_ALLOC  the buffers did not fit
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a coordinate of a point or a body that is not finite, or whose square overflows T, gives unspecified
 * values for that point or body only; r2^(-5/2) leaves the normal range of fp32 beyond |d| ~ 1e15, where the terms flush to zero.
 *
 * Deliberately not here: groups; device pointers for points or results; jerk; the pairwise tensors of the full variational
 * equation; eigenvalues on the device (nbx.py has tidal_matrix and tidal_radius on the host); the reference summation order;
 * hipGraph replay; a command-line word or an environment knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_TIDAL_H
#define NBX_TIDAL_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_tidal(nbx_ctx* c, int32_t m, const void* px, const void* py, const void* pz, /* [m] */
              void* t[6] /* xx, xy, xz, yy, yz, zz: each [m] or NULL */);
int nbx_ensemble_tidal(nbx_ensemble* e, int32_t first, int32_t count, int32_t m,
                       const void* px, const void* py, const void* pz, /* [count * m] */
                       void* t[6] /* each [count * m] or NULL */);
int nbx_ragged_tidal(nbx_ragged* r, int32_t first, int32_t count, int32_t m,
                     const void* px, const void* py, const void* pz, /* [count * m] */
                     void* t[6] /* each [count * m] or NULL */);

int nbx_tidal_bodies(nbx_ctx* c, void* t[6] /* each [n] or NULL */);
int nbx_ensemble_tidal_bodies(nbx_ensemble* e, int32_t first, int32_t count, void* t[6] /* each [count * n] or NULL */);
int nbx_ragged_tidal_bodies(nbx_ragged* r, int32_t first, int32_t count, void* t[6] /* each: members end to end, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* NBX_TIDAL_H */
