"""fp64 numpy restatement of include/nbx_timescale.h, the states the timescale tests plant extreme pairs in, and the adaptive
loop of nbx.py's adaptive() over kick_ref.step.

The three values are evaluated in fp64 from the state as libnbx stores it: positions and velocities as given (fp32 or fp64)
and widened, G*m rounded as nbx_upload rounds it (energy_ref.gm_as_uploaded), eps^2 = 1e-3f widened.  The search runs over
all pairs in row chunks, j == i excluded; a system of one body has no pair: rates 0, min_r2 +inf.
"""
import math

import numpy as np

import energy_ref as E
import kick_ref as K

KEYS = ("approach_rate2", "freefall_rate2", "min_r2")


def _search(state, exclude, chunk):
    """(all pairs, all pairs but `exclude`) in one pass over the pair arrays."""
    x, y, z, u, v, w = (np.asarray(state[k]).astype(np.float64) for k in K.FIELDS[:6])
    gm = E.gm_as_uploaded(state["mass"])
    n = len(gm)
    outs = [{"approach_rate2": 0.0, "freefall_rate2": 0.0, "min_r2": math.inf, "n": n} for _ in range(2)]
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        dx, dy, dz = x[None, :] - x[a:b, None], y[None, :] - y[a:b, None], z[None, :] - z[a:b, None]
        r2 = dx * dx + dy * dy + dz * dz + E.EPS2
        ux, uy, uz = u[None, :] - u[a:b, None], v[None, :] - v[a:b, None], w[None, :] - w[a:b, None]
        approach = (ux * ux + uy * uy + uz * uz) / r2
        freefall = (gm[None, :] + gm[a:b, None]) / (r2 * np.sqrt(r2))
        rows = np.arange(b - a)
        drops = [(rows, np.arange(a, b))]  # j == i excluded
        if exclude:
            ex = [(i - a, j) for i, j in exclude if a <= i < b]
            drops.append((np.array([e[0] for e in ex], dtype=int), np.array([e[1] for e in ex], dtype=int)))
        for out, drop in zip(outs, drops):
            approach[drop] = 0.0
            freefall[drop] = 0.0
            r2[drop] = math.inf
            out["approach_rate2"] = max(out["approach_rate2"], float(approach.max()))
            out["freefall_rate2"] = max(out["freefall_rate2"], float(freefall.max()))
            out["min_r2"] = min(out["min_r2"], float(r2.min()))
    return outs


def timescale(state, chunk=64, exclude=()):
    """{approach_rate2, freefall_rate2, min_r2, n} of `state` (a dict of the seven arrays).  `exclude`: ordered pairs (i, j)
    left out besides j == i (the tests ask for the background of a planted pair with it)."""
    return _search(state, tuple(exclude), chunk)[1 if exclude else 0]


def timescale_and_background(state, i, j, chunk=64):
    """(timescale(state), timescale(state) without the pair (i, j) in either order) from one pass."""
    return tuple(_search(state, ((i, j), (j, i)), chunk))


def pair_values(state, i, j):
    """The three values of the one pair (i, j), in fp64 from the state as stored."""
    d = [float(state[k][j]) - float(state[k][i]) for k in K.FIELDS[:6]]
    gm = E.gm_as_uploaded(state["mass"])
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + E.EPS2
    return {"approach_rate2": (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) / r2,
            "freefall_rate2": float(gm[i] + gm[j]) / (r2 * math.sqrt(r2)), "min_r2": r2}


def suggest_dt(ts, eta):
    """nbx.suggest_dt, restated: eta / sqrt(the largest rate of one dict or of a list of them); inf where every rate is 0."""
    entries = [ts] if isinstance(ts, dict) else list(ts)
    rate = max([max(t["approach_rate2"], t["freefall_rate2"]) for t in entries], default=0.0)
    return eta / math.sqrt(rate) if rate > 0.0 else math.inf


# ---------------------------------------------------------------------------------------------------------------------------
# states with one planted extreme pair (the device tests)
# ---------------------------------------------------------------------------------------------------------------------------
SPREAD = 40.0  # eps^2 = 1e-3 is the floor of r2: a pair can be closest BY A FACTOR only in a background whose bodies are apart
PLANT_SEP, PLANT_SPEED, PLANT_MASS = 1.0 / 1024, 2.0, 10.0


def spread_state(seed, n, dtype=np.float64):
    """kick_ref.make_state with the positions scaled by SPREAD, so that the closest background pair of 4097 bodies is some
    tenths apart (r2 >= 10 eps^2) and a planted pair can undercut it by the factor the tests ask for."""
    s = K.make_state(seed, n, dtype=np.float64)
    for k in K.FIELDS[:3]:
        s[k] = s[k] * SPREAD
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in s.items()}


def plant_pair(state, i, j):
    """Body j next to body i (PLANT_SEP away in x), the two moving against each other at PLANT_SPEED in y, each PLANT_MASS
    times the heaviest background body: the closest, the fastest-approaching and the heaviest pair.  In place."""
    T = state["mass"].dtype.type
    heavy = T(PLANT_MASS) * state["mass"].max()
    state["pos_x"][j] = state["pos_x"][i] + T(PLANT_SEP)
    state["pos_y"][j], state["pos_z"][j] = state["pos_y"][i], state["pos_z"][i]
    for b, sign in ((i, 0.5), (j, -0.5)):
        state["vel_x"][b], state["vel_y"][b], state["vel_z"][b] = T(0), T(sign * PLANT_SPEED), T(0)
        state["mass"][b] = heavy
    return state


# ---------------------------------------------------------------------------------------------------------------------------
# the adaptive loop, and the 96-body systems with one near-collision of two heavy bodies (CPU and device tests)
# ---------------------------------------------------------------------------------------------------------------------------
ENCOUNTER_SEEDS = (2, 4, 5)
ENCOUNTER_T, ENCOUNTER_ETA, ENCOUNTER_DT_MAX = 0.5, 0.05, 1.0 / 16
ENCOUNTER_SPEED, ENCOUNTER_MASS = 80.0, 40.0


def encounter_state(seed, dtype=np.float64):
    """kick_ref.make_state(seed) with bodies 0 and 1 made ENCOUNTER_MASS times the heaviest body and sent head-on at each other
    along x at a relative speed of ENCOUNTER_SPEED, from a distance they close in ENCOUNTER_T / 2: they pass through each other
    (r2 = eps^2) in the middle of the run, in about eps / speed = 4e-4 time units -- less than half of the 1e-3 a fixed step of
    the same count comes to."""
    s = K.make_state(seed)
    heavy = ENCOUNTER_MASS * s["mass"].max()
    sep = ENCOUNTER_SPEED * ENCOUNTER_T / 2
    for i, sign in ((0, -1.0), (1, 1.0)):
        s["pos_x"][i], s["pos_y"][i], s["pos_z"][i] = sign * sep / 2, 0.0, 0.0
        s["vel_x"][i], s["vel_y"][i], s["vel_z"][i] = -sign * ENCOUNTER_SPEED / 2, 0.0, 0.0
        s["mass"][i] = heavy
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in s.items()}


def adaptive(states, t_end, eta, dt_max, max_steps=100000):
    """nbx.py's adaptive() over kick_ref.step, in place: (t, steps, dts).  `states`: one state, or a list of them stepped
    together as the members of a batch object are -- every one takes the same dt, the smallest any of them asks for."""
    members = [states] if isinstance(states, dict) else list(states)
    t, dts = 0.0, []
    while t < t_end:
        if len(dts) >= max_steps:
            raise RuntimeError("adaptive: t = %r of %r after max_steps = %d steps" % (t, t_end, max_steps))
        dt = min(dt_max, suggest_dt([timescale(s) for s in members], eta), t_end - t)
        for s in members:
            K.step(s, 1, dt)
        dts.append(dt)
        t = t_end if dt == t_end - t else t + dt
    return t, len(dts), dts


def energy_errors(states0, states):
    """|E - E0| / |E0| per state, energy_ref's fp64 read-out."""
    return [abs(K.etotal(s) - K.etotal(s0)) / abs(K.etotal(s0)) for s0, s in zip(states0, states)]
