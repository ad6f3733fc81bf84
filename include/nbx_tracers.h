/*
 * nbx_tracers.h -- resident test particles that step with the bodies: m massless tracers per system, kept on the device and
 * advanced by the same scheme, from the same positions and in the same stream as the bodies, for a context, for every member of
 * an ensemble or for every member of a ragged ensemble.  Kept apart from the other headers, whose symbol sets and structs stay
 * as they are (NBX_ABI_VERSION does not change); same conventions: plain C, int status, text via nbx_last_error(), one host
 * thread drives an object at a time.
 *
 * Why: restricted N-body -- tidal streams, ring and disc particles, orbits in a live potential, escapers -- is the standard use
 * of a direct-sum code beyond the bodies themselves.  nbx_field.h serves it with a round trip per step: upload the points, two
 * launches, read back, synchronise, update on the host, nbx_step(dt, 1).  That is two copies and one synchronisation per step,
 * and nsteps = 1 cuts the bodies off from everything a longer step call can do.  The bodies never wait on the host in this
 * library; with this header neither do their massless companions.
 *
 * Definition: a tracer is a position p and a velocity w in the object's precision T.  It feels every body and is felt by none.
 * There is no self-exclusion, as in nbx_field.h: a tracer is not a body, and a tracer that sits on a body gets a zero term from
 * it.  One step of nbx_tracers_step takes the bodies from x(t) to x(t + dt) exactly as nbx_step does, and advances every tracer
 * by the same semi-implicit Euler step in the field of the bodies at time t -- the positions the bodies' own force launch of
 * that step reads:
 *     a  = a(p) as nbx_field defines it, from the bodies' positions BEFORE their step of this iteration
 *     w += fl(a * dt);   p += fl(w * dt)         (separately rounded multiply and add, never contracted; dt rounded once to T)
 * nbx_tracers_kick is the velocity half alone: w += fl(a(p) * h), positions untouched.
 *
 * Arrays: host SoA arrays in the object's precision (float for 32, double for 64), [m] for a context.  A batch kind gives every
 * member the same number m of tracers: member first + k uses elements [k m, (k + 1) m) of every array, for ensembles and ragged
 * ensembles alike.  nbx_tracers_upload replaces the set (m == 0 removes it).  For a batch kind the first upload fixes m for the
 * object; a later upload with another m is NBX_ERR_ARG unless its range covers all members, which replaces the set (m == 0:
 * removes it).  Any pointer of a download may be NULL; a NULL array is never written.
 *
 * Contracts:
 *   Bodies are untouched.  After nbx_tracers_step(dt, N) the bodies' positions, velocities, kinetic energy and steps_done are
 *     bit for bit what nbx_step(dt, N) gives, for every context option and launch plan, whether or not that nbx_step would
 *     have replayed a graph.  The body launches are the step's own: the library calls the very one-step function nbx_step's
 *     plain loop calls.  kenergy_out is the bodies' (tracers have no mass).
 *   The tracer acceleration is nbx_field's.  At every step the acceleration applied to tracer q is the bits nbx_field (or
 *     nbx_ensemble_field / nbx_ragged_field) returns for the same state and the same m points: the launch shape is that header's
 *     function of (m, n) alone, a j split sums in T with j ascending, the finish adds the splits in fp64 in split order and
 *     rounds once.  Hence a member's tracers are bit for bit those of a context that holds that member's state and tracers
 *     and steps its bodies as the member's are stepped (the context nbx_ensemble.h and nbx_ragged.h name for the bodies' own
 *     bits), and step(3); step(2) is step(5).
 *   nbx_tracers_kick is velocity-only: w + fl(a h) with that same a.  With nbx_kick on the bodies (nbx_kick.h), kick-drift-kick
 *     leapfrog of the joint system is kick(-dt/2) on both, nbx_tracers_step N times, kick(+dt/2) on both.
 *   Independence.  Plain nbx_step, nbx_upload, nbx_kick and every analysis call leave the tracers' bits alone (tracers uploaded
 *     before the bodies, or kept across a new nbx_upload, simply feel the new bodies).  The tracer calls in turn leave alone what
 *     they do not own: nbx_field's results, the kinetic-energy partials (nbx_tracers_step leaves the partials nbx_step leaves),
 *     the *_timed / *_ms_total fields -- the tracer launches are not counted in the profile of the force kernel -- and the
 *     cached graphs.
 *   Launches per step: one pair-work launch and one update launch for the tracers of all systems, then the body step's own
 *     launches, all on the object's stream.  No atomics.
 *
 * Semantics: calls are ordered on the object's stream.  nbx_tracers_step follows nbx_step's asynchrony rule: it synchronises
 * only when kenergy_out is given ([members] for a batch kind, or NULL).  nbx_tracers_kick does not synchronise.  Upload and
 * download synchronise.  Batch step and kick act on all members.  The buffers are allocated on first upload, grown when a larger
 * set arrives, never shrunk, and freed with the object.
 *
 * Status, in this order (a call skips the lines that name arguments it does not have):
 *   NBX_ERR_ARG    the handle is NULL (nbx_tracers_count: or m is NULL)
 *   NBX_ERR_ARG    m < 0
 *   NBX_ERR_ARG    m > 0 and any of the six upload arrays is NULL
 *   NBX_ERR_ARG    members [first, first + count) leave [0, members)
 *   NBX_ERR_ARG    (int64) members * m > 2^22 = 4194304 (a context: m > 2^22), the field's bound for the field's reason: the row
 *                  indices of the partials stay in 32 bits.  Then, for a batch kind: m differs from the object's m and the range
 *                  does not cover all members
 *   NBX_ERR_ARG    nsteps < 0
 *   NBX_ERR_ARG    dt or h is not finite
 *   NBX_ERR_STATE  step and kick: the bodies have not been uploaded; for an ensemble or a ragged ensemble the text names the
 *                  first such member
 *   NBX_ERR_STATE  step, kick and download: no tracers have been uploaded; for a batch kind whose m is fixed the text names the
 *                  first member (of the range, for a download) without tracers
 *   NBX_ERR_STATE  step and kick: the context owns a slice (i_count < n), or has a local step awaiting nbx_commit, as nbx_step
 *   NBX_OK         upload or download with count == 0: nothing is copied
 *   NBX_ERR_ALLOC  upload: the buffers did not fit (the set that was there is gone)
 * Every check but the last comes before the first HIP call.
 *
 * Unspecified results: a coordinate of a tracer that is not finite, or whose square overflows T, gives unspecified values for
 * that tracer only, from then on.
 *
 * Deliberately not here: groups and sliced contexts; tracers with mass, or any back-reaction on the bodies; a different m per
 * ragged member; per-tracer time steps; device pointers; tracer energies (take nbx_field's phi at the downloaded positions);
 * hipGraph replay of the tracer loop; a command-line word or an environment knob in nbody.x (its output is the reference's).
 */
#ifndef NBX_TRACERS_H
#define NBX_TRACERS_H

#include "nbx.h"
#include "nbx_ensemble.h"
#include "nbx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

int nbx_tracers_upload(nbx_ctx* c, int32_t m, const void* px, const void* py, const void* pz,
                       const void* vx, const void* vy, const void* vz /* [m] */);
int nbx_tracers_download(nbx_ctx* c, void* px, void* py, void* pz, void* vx, void* vy, void* vz /* [m] or NULL */);
int nbx_tracers_count(nbx_ctx* c, int32_t* m);
int nbx_tracers_step(nbx_ctx* c, double dt, int32_t nsteps, double* kenergy_out /* or NULL */);
int nbx_tracers_kick(nbx_ctx* c, double h);

int nbx_ensemble_tracers_upload(nbx_ensemble* e, int32_t first, int32_t count, int32_t m, const void* px, const void* py,
                                const void* pz, const void* vx, const void* vy, const void* vz /* [count * m] */);
int nbx_ensemble_tracers_download(nbx_ensemble* e, int32_t first, int32_t count, void* px, void* py, void* pz,
                                  void* vx, void* vy, void* vz /* [count * m] or NULL */);
int nbx_ensemble_tracers_count(nbx_ensemble* e, int32_t* m);
int nbx_ensemble_tracers_step(nbx_ensemble* e, double dt, int32_t nsteps, double* kenergy_out /* [members] or NULL */);
int nbx_ensemble_tracers_kick(nbx_ensemble* e, double h);

int nbx_ragged_tracers_upload(nbx_ragged* r, int32_t first, int32_t count, int32_t m, const void* px, const void* py,
                              const void* pz, const void* vx, const void* vy, const void* vz /* [count * m] */);
int nbx_ragged_tracers_download(nbx_ragged* r, int32_t first, int32_t count, void* px, void* py, void* pz,
                                void* vx, void* vy, void* vz /* [count * m] or NULL */);
int nbx_ragged_tracers_count(nbx_ragged* r, int32_t* m);
int nbx_ragged_tracers_step(nbx_ragged* r, double dt, int32_t nsteps, double* kenergy_out /* [members] or NULL */);
int nbx_ragged_tracers_kick(nbx_ragged* r, double h);

#ifdef __cplusplus
}
#endif
#endif /* NBX_TRACERS_H */
