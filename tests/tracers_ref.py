"""Resident tracers (include/nbx_tracers.h): the round trip they replace, the comparison the tests apply, and a numpy restatement
of one nbx_tracers_step and one nbx_tracers_kick for one system with plantable faults.  Used by tests/test_tracers_cpu.py and
tests/test_tracers_gpu.py; numpy only, no device.

The round trip (round_trip): per step, the field at the host's tracer positions from a twin object that holds the bodies, the
update w += fl(a dt); p += fl(w dt) in numpy in the object's dtype -- separately rounded operations, dt rounded once to T -- and
one plain step of the twin.  The twin is anything with Context's field(px, py, pz) and step(nsteps, dt, kenergy): an nbx.Context on
the device, a RefTwin here.  A result is right when it holds the round trip's bits (same).

RefTwin: bodies advanced by kick_ref.step (a plain direct sum in T), the field by field_ref.restate -- the kernel's own order:
columns, splits and tiles per split from field_shape(m, n), a split's sums in T with j ascending, the splits added in fp64 in
split order and rounded once.  numpy has no FMA and its 1 / sqrt is not v_rsq: these are not the device's bits, but the round
trip and the restatement below are built from the same parts, so the unfaulted restatement holds the round trip's bits and a
faulted one does not.

The restatement (restate_step, restate_kick) is written apart from round_trip: it takes the bodies' states x(t_0) ... x(t_N) and
walks the steps itself.  fault = one of FAULTS plants what the device code could get wrong.
"""
import numpy as np

import field_ref as R
import kick_ref as K

KEYS = K.FIELDS[:6]
POS, VEL = KEYS[:3], KEYS[3:]
ACC = R.KEYS[:3]
COL = R.COL

FAULTS = ("force from the bodies after their step", "position advanced with the old velocity", "a dt fused into the add",
          "tail tracers of the last column not advanced", "member k reads member 0's tracers", "the kick also moves positions",
          "the finish adds only the first split", "cur not flipped between steps")


def same(a, b):
    """Two tracer (or body) dicts hold the same bits in the six arrays."""
    return all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).shape == np.asarray(b[k]).shape and
               np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def copy(tr):
    return {k: np.array(tr[k], copy=True) for k in KEYS}


def make_tracers(precision, state, m, seed=0):
    """m tracers of a state: positions uniform in the bodies' bounding box (field_ref's "box" points), velocities 0.3 uniform in
    [-1, 1]^3, in T."""
    T = R.DTYPE[precision]
    p = R.make_points(precision, state, m, "box", seed=seed)
    v = 0.3 * np.random.default_rng([91, len(state["mass"]), m, seed]).uniform(-1.0, 1.0, (3, m))
    out = dict(zip(POS, p))
    out.update({k: np.ascontiguousarray(c.astype(T)) for k, c in zip(VEL, v)})
    return out


def euler(tr, acc, dt, T):
    """w += fl(a dt); p += fl(w dt) in place, every operation rounded to T."""
    h = T(dt)
    for p, w, a in zip(POS, VEL, acc):
        tr[w] = (tr[w] + (np.asarray(a, dtype=T) * h).astype(T)).astype(T)
        tr[p] = (tr[p] + (tr[w] * h).astype(T)).astype(T)


def kick(tr, acc, h, T):
    """w += fl(a h) in place; positions untouched."""
    h = T(h)
    for w, a in zip(VEL, acc):
        tr[w] = (tr[w] + (np.asarray(a, dtype=T) * h).astype(T)).astype(T)


def round_trip(twin, tracers, precision, dt, nsteps):
    """(tracers after nsteps steps, the twin's kinetic energy after its last step): what nbx_field, a host update and
    nbx_step(dt, 1) give, per step.  The twin is advanced by nsteps steps."""
    T = R.DTYPE[precision]
    tr = copy(tracers)
    ke = None
    for _ in range(nsteps):
        f = twin.field(*[tr[k] for k in POS])
        euler(tr, [f[k] for k in ACC], dt, T)
        ke = twin.step(1, dt, kenergy=True)
    return tr, ke


def round_trip_kick(twin, tracers, precision, h):
    """The tracers after w += fl(a(p) h) with the twin's field; the twin is untouched."""
    tr = copy(tracers)
    f = twin.field(*[tr[k] for k in POS])
    kick(tr, [f[k] for k in ACC], h, R.DTYPE[precision])
    return tr


class RefTwin:
    """A context's field() and step() in numpy: kick_ref.step for the bodies, field_ref.restate for the field."""

    def __init__(self, state, precision):
        self.precision = precision
        self.state = K.copy(state)

    def field(self, px, py, pz):
        return R.restate(self.state, (px, py, pz), self.precision)

    def step(self, nsteps, dt, kenergy=True):
        K.step(self.state, nsteps, dt)
        return None


def body_states(state, dt, nsteps):
    """[x(t_0), ..., x(t_nsteps)]: the states a RefTwin passes through."""
    out = [K.copy(state)]
    for _ in range(nsteps):
        s = K.copy(out[-1])
        K.step(s, 1, dt)
        out.append(s)
    return out


def _fused(w, a, h, T):
    """fl(w + a h) with ONE rounding: in fp64 for fp32 (the product is exact there); in np.longdouble for fp64."""
    wide = np.float64 if T == np.float32 else np.longdouble
    return (w.astype(wide) + a.astype(wide) * wide(h)).astype(T)


def _accel(state, pos, precision, fault):
    T = R.DTYPE[precision]
    if fault == "the finish adds only the first split":  # the bodies of split 0 alone: one split, the same sequential sums in T
        n, m = len(state["mass"]), len(pos[0])
        _, _, splits, per = R.field_shape(m, n)
        assert splits > 1, "the fault needs a shape with more than one split"
        head = {k: v[:per * R.TILE] for k, v in state.items()}
        assert R.field_shape(m, per * R.TILE)[2] == 1
        f = R.restate(head, pos, precision)
    else:
        f = R.restate(state, pos, precision)
    return [np.asarray(f[k], dtype=T) for k in ACC]


def restate_step(states, tracers, precision, dt, nsteps, fault=None, member0=None):
    """The tracers after nbx_tracers_step(dt, nsteps), `states` = body_states(...) of the system they belong to.  fault: one of
    FAULTS; member0: member 0's tracers, for "member k reads member 0's tracers" (the pair kernel then evaluates the field at
    their positions, which move with it)."""
    assert fault is None or fault in FAULTS, fault
    T = R.DTYPE[precision]
    h = T(dt)
    tr = copy(tracers)
    src = copy(member0) if fault == "member k reads member 0's tracers" else None
    m = len(tr["pos_x"])
    for s in range(nsteps):
        at = s
        if fault == "force from the bodies after their step":
            at = s + 1
        elif fault == "cur not flipped between steps":
            at = 0
        a = _accel(states[at], [(src or tr)[k] for k in POS], precision, fault)
        if src is not None:
            euler(src, a, dt, T)
        live = slice(0, m)
        if fault == "tail tracers of the last column not advanced":
            live = slice(0, (m // COL) * COL)
        for p, w, c in zip(POS, VEL, a):
            old = tr[w].copy()
            if fault == "a dt fused into the add":
                tr[w][live] = _fused(tr[w], c, dt, T)[live]
            else:
                tr[w][live] = (tr[w] + (c * h).astype(T)).astype(T)[live]
            v = old if fault == "position advanced with the old velocity" else tr[w]
            tr[p][live] = (tr[p] + (v * h).astype(T)).astype(T)[live]
    return tr


def restate_kick(state, tracers, precision, hk, fault=None):
    """The tracers after nbx_tracers_kick(hk)."""
    assert fault is None or fault in FAULTS, fault
    T = R.DTYPE[precision]
    h = T(hk)
    tr = copy(tracers)
    a = _accel(state, [tr[k] for k in POS], precision, fault)
    for p, w, c in zip(POS, VEL, a):
        tr[w] = (tr[w] + (c * h).astype(T)).astype(T)
        if fault == "the kick also moves positions":
            tr[p] = (tr[p] + (tr[w] * h).astype(T)).astype(T)
    return tr
