"""numpy restatement of the library's update and of the kick of include/nbx_kick.h, and the small systems the kick tests use.

The update is the reference's: v += a(x) * dt; x += v * dt, every operation in the state's precision.  The acceleration is a plain
direct sum a_i = sum_j G m_j (x_j - x_i) / (|x_j - x_i|^2 + eps^2)^(3/2) in the state's precision (the j == i term is zero by
itself, as in the kernels); the library's kernels differ from it in summation order and in the rounding of the pair term, not in
what they compute.  The energy is energy_ref's fp64 read-out, the one the diagnostics tests hold the library to.

The systems: n bodies, G * sum m ~ 1 (masses uniform in [0.5, 1.5] / (G n)), positions uniform in [-1, 1]^3, velocities
0.3 * uniform in [-1, 1]^3, from numpy's PCG64 at a fixed seed -- a crossing time of a few units, so that T = 0.5 at dt = 1/64
... 1/256 is well inside the asymptotic range of both integrators.  A leapfrog energy error oscillates about zero, so at any one T
a system can sit near a zero crossing, where the ratio between two step sizes says nothing about the order: SEEDS are three systems
chosen, with this restatement alone, away from one -- their errors are the figures test_kick_cpu.py states, with room on both
sides of every gate the device tests apply to the same systems.
"""
import numpy as np

import energy_ref as E

FIELDS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")
SEEDS = (95, 119, 307)
N = 96
T_END = 0.5


def make_state(seed, n=N, dtype=np.float64):
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.5, 1.5, n) / (float(E.G32) * n)
    pos = rng.uniform(-1.0, 1.0, (3, n))
    vel = 0.3 * rng.uniform(-1.0, 1.0, (3, n))
    s = dict(zip(FIELDS, list(pos) + list(vel) + [m]))
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in s.items()}


def copy(state):
    return {k: v.copy() for k, v in state.items()}


def accel(state):
    T = state["mass"].dtype.type
    gm = (T(E.G32) * state["mass"]).astype(T)
    d = [state[k][None, :] - state[k][:, None] for k in FIELDS[:3]]
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + T(E.EPS2)
    s = gm[None, :] / (r2 * np.sqrt(r2))
    return [(c * s).sum(axis=1, dtype=T) for c in d]


def kick(state, h):
    """v += a(x) * h in place; positions untouched."""
    T = state["mass"].dtype.type
    for k, a in zip(FIELDS[3:6], accel(state)):
        state[k] = state[k] + a * T(h)


def step(state, nsteps, dt):
    T = state["mass"].dtype.type
    for _ in range(nsteps):
        kick(state, dt)
        for p, v in zip(FIELDS[:3], FIELDS[3:6]):
            state[p] = state[p] + state[v] * T(dt)


def leapfrog(state, nsteps, dt):
    kick(state, -0.5 * dt)
    step(state, nsteps, dt)
    kick(state, 0.5 * dt)


def etotal(state):
    return E.diagnostics(state)["etotal"]


def energy_error(state0, dt, leap, t_end=T_END):
    """|E(T) - E(0)| / |E(0)| of `state0` advanced over t_end with steps of dt, plainly or with the two half kicks."""
    s = copy(state0)
    n = int(round(t_end / dt))
    (leapfrog if leap else step)(s, n, dt)
    e0 = etotal(state0)
    return abs(etotal(s) - e0) / abs(e0)


def there_and_back(state0, nsteps, dt, leap):
    """max |state - state0| over positions and velocities after nsteps forward and nsteps back."""
    s = copy(state0)
    run = leapfrog if leap else step
    run(s, nsteps, dt)
    run(s, nsteps, -dt)
    return max(float(np.abs(s[k].astype(np.float64) - state0[k].astype(np.float64)).max()) for k in FIELDS[:6])
