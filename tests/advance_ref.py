"""Adaptive power-of-two time steps chosen on the device (include/nbx_advance.h): the header's criterion and quantiser in numpy,
and run(), the whole scheme on top of hermite_ref.predict and hermite_ref.correct.  Used by tests/test_advance_cpu.py,
tests/test_advance_gpu.py and tools/advance_cost.py; numpy only, no device of its own.

The criterion: T-valued (3, n) arrays widened, every operation a separately rounded fp64 multiply or add -- numpy fuses nothing --
innermost bracket first, per component, one correctly rounded sqrt and one division where written:
    d = a0 - a1;  a2 = (((-6 d) - h*((4 j0) + (2 j1))) * ih) * ih;  a3 = ((((12 d) + (6 h)*(j0 + j1)) * ih) * ih) * ih
    a2 = a2 + h*a3;  |v|^2 = (vx*vx + vy*vy) + vz*vz;  A = |a1|^2, J = |j1|^2, S = |a2|^2, C = |a3|^2
    s_i = (sqrt(A*S) + J) / (sqrt(J*C) + S) where the denominator is > 0, else +inf;  at the start A / J where J > 0, else +inf
q = min_i s_i, a NaN never selected.  The quantiser, integers only: E = the exponent field of eta2 * q minus 1023,
k_crit = floor(E / 2); after a step of 2^k: k + 1 if k_crit > k and t is a multiple of 2^(k+1), else k if k_crit >= k, else
k_crit; at the start k_crit; clamped to [k_cap - levels, k_cap], a step the clamp raised counting as a floor step once taken.

FAULTS can be planted; tests/test_advance_cpu.py shows that each changes a recorded history or an end state.  FLOOR_FAULTS sit in the
clamp, the floor count and the start rule where J is 0: they change nothing where the floor never binds and no body is at rest --
every case of that module -- and tests/test_large_steppers_cpu.py shows that each changes a clock of the clamp and cold-start cases
of tests/test_advance_gpu.py."""
import math

import numpy as np

import hermite_ref as H

TILE = 256
FAULTS = ("a2 is not advanced to the end of the step", "the factor 12 in a3", "doubling without the commensurability test",
          "E / 2 rounded towards zero", "the start rule on every step", "the minimum over padding records")
FLOOR_FAULTS = ("floor_steps counts a step when it is chosen", "raised is evaluated after the clamp",
                "a done system's floor_steps keeps counting", "the start candidate is 0 where J is 0")


def exponent(x):
    """The exponent field of the double x >= 0 minus 1023: +inf gives 1024, zero and the subnormals -1023."""
    return int((np.array(x, dtype=np.float64).view(np.int64) >> 52) & 0x7FF) - 1023


def _norm2(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def start_candidates(a, j, fault=None):
    """(n,) candidates after the evaluation that starts a call: A / J where J > 0, else +inf."""
    a, j = (np.asarray(x).astype(np.float64) for x in (a, j))
    A, J = _norm2(a), _norm2(j)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(J > 0.0, A / J, 0.0 if fault == "the start candidate is 0 where J is 0" else np.inf)


def candidates(a0, j0, a1, j1, h, fault=None):
    """(n,) candidates after a step of h from (3, n) arrays in T."""
    a0, j0, a1, j1 = (np.asarray(x).astype(np.float64) for x in (a0, j0, a1, j1))
    h = float(h)
    ih = 1.0 / h
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = a0 - a1
        a2 = (((-6.0 * d) - h * ((4.0 * j0) + (2.0 * j1))) * ih) * ih
        twelve = 6.0 if fault == "the factor 12 in a3" else 12.0
        a3 = ((((twelve * d) + (6.0 * h) * (j0 + j1)) * ih) * ih) * ih
        if fault != "a2 is not advanced to the end of the step":
            a2 = a2 + h * a3
        A, J, S, C = _norm2(a1), _norm2(j1), _norm2(a2), _norm2(a3)
        num = np.sqrt(A * S) + J
        den = np.sqrt(J * C) + S
        return np.where(den > 0.0, num / den, np.inf)


def minimum(s, fault=None):
    """q: the smallest candidate that is not a NaN, +inf if there is none."""
    s = np.asarray(s, dtype=np.float64)
    if fault == "the minimum over padding records":
        s = np.concatenate([s, np.zeros(-len(s) % TILE + TILE)])  # records behind the system's, as a cleared buffer holds them
    s = s[~np.isnan(s)]
    return float(s.min()) if len(s) else math.inf


def k_crit(q, eta2, fault=None):
    e = exponent(np.float64(eta2) * np.float64(q))
    if fault == "E / 2 rounded towards zero":
        return int(e / 2)
    return e >> 1  # the floor, for negative odd E too


def choose(q, eta2, k_cap, levels, k=None, t=None, fault=None):
    """(the exponent of the next step, whether the floor raised it).  k, t: the exponent of the step just taken and the time after
    it (None: the start)."""
    kc = k_crit(q, eta2, fault)
    nxt = kc
    if k is not None and fault != "the start rule on every step" and kc >= k:
        u = t * (0.5 * 2.0 ** -k)  # t / 2^(k+1), exact
        fits = u == math.floor(u) or fault == "doubling without the commensurability test"
        nxt = k + 1 if (kc > k and fits) else k
    k_floor = k_cap - levels
    clamped = min(max(nxt, k_floor), k_cap)
    return clamped, (clamped if fault == "raised is evaluated after the clamp" else nxt) < k_floor


def new_clock():
    return {"t": 0.0, "dt_last": 0.0, "dt_next": 0.0, "steps": 0, "floor_steps": 0, "floor_next": False}


def start(clock, a, j, eta, k_cap, levels, fault=None):
    """The clock after the evaluation (a, j) that starts a call without resume."""
    k, raised = choose(minimum(start_candidates(a, j, fault), fault), float(eta) * float(eta), k_cap, levels, fault=fault)
    clock.update(new_clock())
    clock.update(dt_next=2.0 ** k, floor_next=raised)
    if fault == "floor_steps counts a step when it is chosen":
        clock.update(floor_steps=int(raised))
    return clock


def after_step(clock, a0, j0, a1, j1, eta, k_cap, levels, fault=None):
    """The clock after a step of clock["dt_next"] whose evaluations were (a0, j0) before and (a1, j1) after."""
    h = clock["dt_next"]
    k = exponent(h)
    t = clock["t"] + h
    if fault is None:
        assert t - h == clock["t"] and (t / h) == math.floor(t / h)  # t += h is exact and t stays a multiple of h
    q = minimum(candidates(a0, j0, a1, j1, h, fault), fault)
    nk, raised = choose(q, float(eta) * float(eta), k_cap, levels, k, t, fault)
    counted = raised if fault == "floor_steps counts a step when it is chosen" else clock["floor_next"]
    clock.update(t=t, dt_last=h, dt_next=2.0 ** nk, steps=clock["steps"] + 1, floor_steps=clock["floor_steps"] + int(counted), floor_next=raised)
    return clock, q


def public(clock, t_end, n=None):
    """The clock as nbx_*_clock reports it."""
    d = {k: clock[k] for k in ("t", "dt_last", "dt_next", "steps", "floor_steps")}
    d["done"] = clock["t"] >= t_end
    if n is not None:
        d["n"] = n
    return d


def run(state, precision, t_end, k_cap, levels, eta, max_steps, evaluate, fault=None, clock=None, carry=None):
    """Up to max_steps steps of one system towards t_end.  clock, carry: what a previous run left (None: t = 0 and an evaluation
    at `state`).  Returns {"state", "carry": (a, j), "clock", "history": [(t before the step, h, eta2 * q after it), ...]}."""
    assert fault is None or fault in FAULTS + FLOOR_FAULTS, fault
    T = H.DTYPE[precision]
    mass = np.asarray(state["mass"], dtype=T)
    x, v = H.unpack(state, T)
    if clock is None:
        a0, j0 = evaluate(H.pack(x, v, mass))
        a0, j0 = np.asarray(a0).astype(T), np.asarray(j0).astype(T)
        clock = start({}, a0, j0, eta, k_cap, levels, fault)
    else:
        clock = dict(clock)
        a0, j0 = carry
    history = []
    for _ in range(max_steps):
        if clock["t"] >= t_end:
            if fault == "a done system's floor_steps keeps counting":  # the launches of the steps a done system does not take
                clock["floor_steps"] += int(clock["floor_next"])
                continue
            break
        h = clock["dt_next"]
        k = H.consts(h, precision)
        assert k[0] == h
        xp, vp = H.predict(x, v, a0, j0, k, T)
        a1, j1 = evaluate(H.pack(xp, vp, mass))
        a1, j1 = np.asarray(a1).astype(T), np.asarray(j1).astype(T)
        x, v = H.correct(x, v, a0, j0, a1, j1, k, T)
        t0 = clock["t"]
        clock, q = after_step(clock, a0, j0, a1, j1, eta, k_cap, levels, fault)
        history.append((t0, h, float(eta) * float(eta) * q))
        a0, j0 = a1, j1
    return {"state": H.pack(x, v, mass), "carry": (a0, j0), "clock": clock, "history": history}


def boundary_distance(x):
    """The relative distance of x > 0 (finite) from the nearest power of four."""
    m, e = math.frexp(x)  # x = m 2^e, m in [0.5, 1)
    m, e = (m * 2.0, e - 1) if e % 2 else (m * 4.0, e - 2)  # x = m 4^(e / 2), m in [1, 4)
    return min(m - 1.0, (4.0 - m) / 4.0)
