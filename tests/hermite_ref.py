"""The resident fourth-order Hermite stepper (include/nbx_hermite.h): the header's formulas in numpy, and the round trip of public
calls the resident step is held to bit for bit.  Used by tests/test_hermite_cpu.py, tests/test_hermite_gpu.py and
tools/hermite_cost.py; numpy only, no device of its own.

The formulas: T-valued state, every operation a separately rounded fp64 multiply or add -- numpy fuses nothing, so these are the
device's operations bit for bit -- innermost bracket first, per component:
    h = dt rounded once to T, widened;  k2 = h * 0.5;  k6 = h / 6.0;  h3 = h / 3.0
    vp = v + h*(a0 + k2*j0)                     xp = x + h*(v + k2*(a0 + h3*j0))             each rounded once to T
    v1 = v + k2*((a0 + a1) + k6*(j0 - j1))      x1 = x + k2*((v + v1) + k6*(a0 - a1))        the unrounded v1 enters x1
a1, j1 come from an `evaluate` callback, state -> (a, adot) as two (3, n) arrays: jerk_ref.direct for the tests without a device,
device_evaluate(obj) -- upload, then jerk() -- for the round trip.  (a1, j1) are (a0, j0) of the next step.

FAULTS can be planted into the formulas; tests/test_hermite_cpu.py shows that each either costs the scheme its order or changes
bits against the unfaulted restatement."""
import numpy as np

import jerk_ref as R

POS, VEL = R.POS, R.VEL
DTYPE = R.DTYPE
FAULTS = ("the predictor drops the jerk term", "j1 - j0 in the corrector", "x1 uses v in place of v + v1",
          "a0 is not replaced after a step", "v1 is rounded to T before x1", "k6 = h/12")


def consts(dt, precision):
    """(h, k2, k6, h3) as the host computes them, Python floats (fp64)."""
    h = float(DTYPE[precision](dt))
    return h, h * 0.5, h / 6.0, h / 3.0


def _wide(*arrays):
    return [np.asarray(a).astype(np.float64) for a in arrays]


def predict(x, v, a0, j0, k, T, fault=None):
    """(xp, vp) in T from (3, n) arrays in T."""
    h, k2, _, h3 = k
    x, v, a0, j0 = _wide(x, v, a0, j0)
    if fault == "the predictor drops the jerk term":
        vp = v + h * a0
        xp = x + h * (v + k2 * a0)
    else:
        vp = v + h * (a0 + k2 * j0)
        xp = x + h * (v + k2 * (a0 + h3 * j0))
    return xp.astype(T), vp.astype(T)


def correct(x, v, a0, j0, a1, j1, k, T, fault=None):
    """(x1, v1) in T."""
    _, k2, k6, _ = k
    if fault == "k6 = h/12":
        k6 = k[0] / 12.0
    x, v, a0, j0, a1, j1 = _wide(x, v, a0, j0, a1, j1)
    dj = (j1 - j0) if fault == "j1 - j0 in the corrector" else (j0 - j1)
    v1 = v + k2 * ((a0 + a1) + k6 * dj)
    if fault == "v1 is rounded to T before x1":
        v1 = v1.astype(T).astype(np.float64)
    vv = v if fault == "x1 uses v in place of v + v1" else (v + v1)
    x1 = x + k2 * (vv + k6 * (a0 - a1))
    return x1.astype(T), v1.astype(T)


def unpack(state, T):
    return (np.stack([np.asarray(state[f], dtype=T) for f in POS]), np.stack([np.asarray(state[f], dtype=T) for f in VEL]))


def pack(x, v, mass):
    return dict(zip(POS + VEL + ("mass",), [np.ascontiguousarray(c) for c in list(x) + list(v)] + [mass]))


def steps(state, dt, nsteps, precision, evaluate, carry=None, fault=None):
    """nsteps P(EC) steps of dt from `state` (a dict of the seven arrays).  carry: (a0, j0) kept by the steps before (None: they
    are evaluated at `state`).  Returns (the state after the steps, in T; (a1, j1) of the last step)."""
    assert fault is None or fault in FAULTS, fault
    T = DTYPE[precision]
    k = consts(dt, precision)
    mass = np.asarray(state["mass"], dtype=T)
    x, v = unpack(state, T)
    a0, j0 = evaluate(pack(x, v, mass)) if carry is None else carry
    a0, j0 = np.asarray(a0).astype(T), np.asarray(j0).astype(T)
    for _ in range(nsteps):
        xp, vp = predict(x, v, a0, j0, k, T, fault)
        a1, j1 = evaluate(pack(xp, vp, mass))
        a1, j1 = np.asarray(a1).astype(T), np.asarray(j1).astype(T)
        x, v = correct(x, v, a0, j0, a1, j1, k, T, fault)
        if fault != "a0 is not replaced after a step":
            a0 = a1
        j0 = j1
    return pack(x, v, mass), (a0, j0)


def joined(states):
    """The members of a ragged ensemble end to end: one state of sum(sizes) bodies (the formulas are per body)."""
    return {f: np.concatenate([np.asarray(s[f]) for s in states]) for f in POS + VEL + ("mass",)}


def parted(state, sizes, keys=POS + VEL + ("mass",)):
    at = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    return [{f: state[f][at[k]:at[k + 1]] for f in keys} for k in range(len(sizes))]


def device_upload(obj, state):
    """upload() of a state as steps() holds it: (n,) arrays for a Context, (members, n) for an Ensemble, joined() for a Ragged."""
    obj.upload(parted(state, obj.sizes) if hasattr(obj, "sizes") else state)


def device_evaluate(obj):
    """evaluate() of the round trip on a Context, an Ensemble or a Ragged: upload the state, ask jerk()."""
    def ev(state):
        device_upload(obj, state)
        r = obj.jerk()
        if isinstance(r, list):
            r = {k: np.concatenate([m[k] for m in r]) for k in R.KEYS}
        return np.stack([r[k] for k in R.ACC]), np.stack([r[k] for k in R.JERK])
    return ev


def round_trip(obj, state, dt, nsteps, carry=None):
    """The round trip of public calls that a resident step replaces: jerk() (unless carried), and per step the host predictor,
    upload(predicted state, same masses), jerk(), the host corrector; the corrected state is uploaded last.  Returns (that last
    upload, (a1, j1) to carry into the next call).  state: as device_upload takes it."""
    end, kept = steps(state, dt, nsteps, obj.precision, device_evaluate(obj), carry)
    device_upload(obj, end)
    return end, kept


def same(a, b, keys=POS + VEL):
    """Bit for bit (values compared as bytes)."""
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)
