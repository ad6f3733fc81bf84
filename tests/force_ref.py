"""High-precision direct sum of the softened-gravity acceleration, a per-body error metric, and the state families of the
step probe (tests/test_step_probe_cpu.py, tests/test_step_probe_gpu.py) and of the moving probe (tests/test_moving_probe_cpu.py,
tests/test_moving_probe_gpu.py), whose velocities and identities are at the end of the metric section.

The values are taken as libnbx stores them: positions in T (fp32 or fp64), G*m rounded as nbx_upload rounds it
(energy_ref.gm_as_uploaded), eps^2 = 1e-3f widened.  Every term

    t_ij^c = G m_j d_ij^c (r_ij^2 + eps^2)^(-3/2)

is evaluated in a precision higher than T -- numpy fp64 for fp32 states, np.longdouble (x87 extended) for fp64 states, or a
two-sum / two-product double-double evaluation where longdouble is no wider than double.  truth() returns, for a list of bodies,

    a_i^c = sum_j t_ij^c          as hi + lo (two fp64 arrays; lo is 0 for fp32 states)
    A_i   = max_c sum_j |t_ij^c|  the scale rounding-error bounds of a sum are stated in: it does not shrink when terms cancel

and K_i = max_c |got_i^c - a_i^c| / (u_T A_i), with u_32 = 2^-24 and u_64 = 2^-53, is the metric.  The one tolerance is

    K_max(kernel) <= M max(K_ref, K_TERM)

K_ref: the same metric for the reference's own arithmetic (the CPU oracle) on the same state and bodies.  K_TERM = 16: the floor
where the sum is short and the per-term arithmetic dominates -- 1 u per coordinate difference, about 4 u on r^2, 1 ulp on the
reciprocal square root, cubed, and the two multiplies; the oracle measures 8.5 to 15.2 at n = 257.  M = 2: the kernels' per-term
arithmetic is not the reference's (rsq instruction and FMA against sqrt, divide and separate roundings), and two correct
roundings of sums of the same length differ by about that much (the five families spread over 109 to 210 at n = 16384).
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from energy_ref import EPS2, gm_as_uploaded

U = {32: 2.0 ** -24, 64: 2.0 ** -53}
K_TERM = 16.0
M = 2.0
DT = float(np.float32(0.1))  # (float)0.1 widened: what nbx_step receives and converts to T (exact in both)
FAMILIES = ("seed42", "adversarial", "offset1000", "lattice", "signedbox")
HAVE_LONGDOUBLE = float(np.finfo(np.longdouble).eps) < 2e-19
_PAIRS_PER_CHUNK = 1 << 21
_THREADS = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))


def gate(k_ref):
    return M * max(float(k_ref), K_TERM)


# ---- the terms -------------------------------------------------------------------------------------------------------------
def term_rows(pos, gm, rows, eps2=EPS2, dtype=np.float64):
    """(tx, ty, tz), each (len(rows), n): the terms of the bodies `rows` against every source, evaluated in `dtype`."""
    x, y, z = (np.asarray(a).astype(dtype) for a in pos)
    g = np.asarray(gm).astype(dtype)
    rows = np.asarray(rows, dtype=np.int64)
    dx = x[None, :] - x[rows, None]
    dy = y[None, :] - y[rows, None]
    dz = z[None, :] - z[rows, None]
    r2 = dx * dx + dy * dy + dz * dz + dtype(eps2)
    s = g[None, :] / (r2 * np.sqrt(r2))
    return dx * s, dy * s, dz * s


def _row_chunks(count, n):
    step = max(1, _PAIRS_PER_CHUNK // max(n, 1))
    return [(a, min(a + step, count)) for a in range(0, count, step)]


# ---- double-double, for platforms whose long double is a double ---------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a  # 2^27 + 1
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(a, b):
    s, e = _two_sum(a[0], b[0])
    return _two_sum(s, e + a[1] + b[1])


def _dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    return _two_sum(p, e + (a[0] * b[1] + a[1] * b[0]))


def _dd_term_rows(pos, gm, rows, eps2):
    """term_rows in double-double: ((hi, lo) per coordinate).  About 100 bits; the inputs are fp64 values."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in pos)
    g = np.asarray(gm, dtype=np.float64)
    d = [_two_sum(c[None, :], -c[rows, None]) for c in (x, y, z)]
    zero = np.zeros_like(d[0][0])
    r2 = (zero + eps2, zero)
    for c in d:
        r2 = _dd_add(r2, _dd_mul(c, c))
    y0 = 1.0 / np.sqrt(r2[0])                       # 1/sqrt to fp64, then one Newton step carried in double-double
    e = _dd_add((zero + 1.0, zero), tuple(-v for v in _dd_mul(r2, _two_prod(y0, y0))))
    w = _two_sum(y0, y0 * (e[0] + e[1]) * 0.5)      # relative error ~ (3/8) e^2 ~ 1e-32
    s = _dd_mul(_dd_mul(w, w), _dd_mul(w, (g[None, :] + zero, zero)))
    return [_dd_mul(c, s) for c in d]


def _dd_rowsum(t):
    hi = np.empty(t[0].shape[0])
    lo = np.empty_like(hi)
    for k in range(len(hi)):
        v = np.concatenate([t[0][k], t[1][k]]).tolist()
        hi[k] = math.fsum(v)
        lo[k] = math.fsum(v + [-hi[k]])
    return hi, lo


# ---- the truth -------------------------------------------------------------------------------------------------------------
def truth(pos, gm, rows, precision, eps2=EPS2, force_dd=False):
    """(a_hi, a_lo, A): a_hi + a_lo = sum_j t_ij for the bodies `rows`, shape (len(rows), 3); A_i = max_c sum_j |t_ij^c|."""
    rows = np.asarray(rows, dtype=np.int64)
    n = len(np.asarray(gm))
    hi = np.zeros((len(rows), 3))
    lo = np.zeros((len(rows), 3))
    A = np.zeros(len(rows))
    wide = precision == 64
    if wide and not force_dd:
        assert HAVE_LONGDOUBLE, "np.longdouble is no wider than double here: call with force_dd"

    def chunk(ab):
        a, b = ab
        if wide and force_dd:
            t = _dd_term_rows(pos, gm, rows[a:b], eps2)
            for c in range(3):
                hi[a:b, c], lo[a:b, c] = _dd_rowsum(t[c])
            A[a:b] = np.max([np.abs(t[c][0]).sum(axis=1) for c in range(3)], axis=0)
            return
        dtype = np.longdouble if wide else np.float64
        t = term_rows(pos, gm, rows[a:b], eps2, dtype)
        for c in range(3):
            s = t[c].sum(axis=1)  # pairwise in numpy: far below u_T in `dtype`
            hi[a:b, c] = s.astype(np.float64)
            lo[a:b, c] = (s - hi[a:b, c].astype(dtype)).astype(np.float64)
        A[a:b] = np.max([np.abs(t[c]).sum(axis=1).astype(np.float64) for c in range(3)], axis=0)

    chunks = _row_chunks(len(rows), n)
    if _THREADS > 1 and len(chunks) > 1:
        with ThreadPoolExecutor(_THREADS) as ex:
            list(ex.map(chunk, chunks))
    else:
        for ab in chunks:
            chunk(ab)
    return hi, lo, A


def truth64(pos, gm, rows, precision, eps2=EPS2):
    """truth() for either precision on any platform: double-double where long double is a double."""
    return truth(pos, gm, rows, precision, eps2, force_dd=(precision == 64 and not HAVE_LONGDOUBLE))


def k_metric(got, tr, precision):
    """K_i of `got` ((rows, 3), fp64 or longdouble values of T numbers or of v1 / dt) against tr = truth(...).  Bodies with
    A_i == 0 -- n = 1, or every other mass zero -- must have got == 0 exactly: they get K = 0 if so and inf if not."""
    hi, lo, A = tr
    wide = np.longdouble if (precision == 64 and HAVE_LONGDOUBLE) else np.float64
    g = np.asarray(got).astype(wide)
    err = np.abs((g - hi.astype(wide)) - lo.astype(wide)).max(axis=1).astype(np.float64)
    K = np.zeros(len(A))
    nz = A > 0
    K[nz] = err[nz] / (U[precision] * A[nz])
    K[~nz] = np.where(err[~nz] == 0, 0.0, np.inf)
    return K


def accel_from_v1(vel, precision, dt=DT):
    """The acceleration a step kernel applied, from the velocities one step of `dt` after an upload with v = 0: euler_update
    rounds v1 = fl(a dt), so v1 / dt is a to half an ulp of T.  vel: (rows, 3) in T; dt: a value of T (exact in the wide type)."""
    wide = np.longdouble if (precision == 64 and HAVE_LONGDOUBLE) else np.float64
    return np.asarray(vel).astype(wide) / wide(dt)


def position_identity(p0, v1, precision, dt=DT):
    """fl(p0 + fl(v1 dt)) in T, as euler_update evaluates it: must equal the downloaded position bit for bit.  dt is converted
    to T by round-to-nearest, as the library converts the double it is given."""
    T = np.float32 if precision == 32 else np.float64
    p0, v1 = np.asarray(p0, dtype=T), np.asarray(v1, dtype=T)
    return (p0 + (v1 * T(dt)).astype(T)).astype(T)


def velocity_identity(v0, v1_rest, precision):
    """fl(v0 + v1_rest) in T.  v1_rest = fl(a dt) is what one step leaves from rest; the acceleration depends on the positions
    only, so the same step from v0 must leave exactly this (euler_update: v = add_rn(v, mul_rn(a, dt)))."""
    T = np.float32 if precision == 32 else np.float64
    return (np.asarray(v0, dtype=T) + np.asarray(v1_rest, dtype=T)).astype(T)


def moving_identity_failures(p0, v0, v1_rest, v1, p1, precision, dt):
    """(rows where v1 != fl(v0 + v1_rest), rows where p1 != fl(p0 + fl(v1 dt))) of one moving step; all arrays (rows, 3) in T."""
    bad_v = np.flatnonzero((np.asarray(v1) != velocity_identity(v0, v1_rest, precision)).any(axis=1))
    bad_p = np.flatnonzero((np.asarray(p1) != position_identity(p0, v1, precision, dt)).any(axis=1))
    return bad_v, bad_p


MOVING_RECIPES =("uniform in [-1, 1]", "fl(v1_rest u), u uniform in [-4, 4]", "-v1_rest", "0", "fl(v1_rest 1e3 N(0, 1))")


def moving_velocities(v1_rest, precision, seed):
    """(n, 3) initial velocities in T for the moving probe; body i takes MOVING_RECIPES[i % 5]: far above a dt; of the magnitude
    of a dt, where the rounding of the add matters; cancelling to zero exactly; zero; and a thousand times a dt with either
    sign.  Every body and component draws its own number, so an index or component mix-up cannot cancel."""
    T = np.float32 if precision == 32 else np.float64
    r = np.asarray(v1_rest, dtype=T)
    n = r.shape[0]
    rng = np.random.default_rng([seed, n, precision])
    draws = (rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-4.0, 4.0, (n, 3)), rng.standard_normal((n, 3)))
    k = (np.arange(n) % 5)[:, None]
    v = np.zeros((n, 3), dtype=T)
    v = np.where(k == 0, draws[0].astype(T), v)
    v = np.where(k == 1, (r * draws[1].astype(T)).astype(T), v)
    v = np.where(k == 2, -r, v)
    v = np.where(k == 4, ((r * T(1e3)).astype(T) * draws[2].astype(T)).astype(T), v)
    return v.astype(T)


# ---- the reference's own arithmetic --------------------------------------------------------------------------------------------
def oracle_accel(oracle, state, rows=None):
    """The CPU oracle's accelerations of `rows` (all bodies if None), (rows, 3) in the state's precision."""
    T = np.asarray(state["mass"]).dtype
    s = oracle.State(len(state["mass"]), T)
    for f in ("pos_x", "pos_y", "pos_z", "mass"):
        getattr(s, f)[:] = state[f]
    if rows is None:
        oracle.accel(s)
        rows = slice(None)
    else:
        rows = np.asarray(rows, dtype=np.int64)
        for i in rows:
            oracle.accel(s, int(i), int(i) + 1)
    return np.stack([s.acc_x[rows], s.acc_y[rows], s.acc_z[rows]], axis=1)


def state_truth(state, rows=None, eps2=EPS2):
    precision = 32 if np.asarray(state["mass"]).dtype == np.float32 else 64
    n = len(state["mass"])
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    return truth64((state["pos_x"], state["pos_y"], state["pos_z"]), gm_as_uploaded(state["mass"]), rows, precision, eps2)


# ---- state families (zero velocities: the probe) ---------------------------------------------------------------------------------
def tile_edges(n, tile=256):
    """Bodies 0, n - 1 and both sides of every tile edge."""
    e = {0, n - 1}
    for k in range(tile, n, tile):
        e.update((k - 1, k))
    return np.array(sorted(i for i in e if 0 <= i < n), dtype=np.int64)


def make_state(oracle, family, n, precision=32, seed=1):
    """One of FAMILIES as the dict of seven arrays nbx.Context.upload takes, in T, all velocities zero."""
    T = np.float32 if precision == 32 else np.float64
    rng = np.random.default_rng([seed, n, FAMILIES.index(family)])
    st = {f: np.zeros(n, dtype=T) for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
    P = ("pos_x", "pos_y", "pos_z")

    def uniform(lo, hi, size):  # fp64 states carry all 53 bits
        return (lo + (hi - lo) * rng.random(size)).astype(T)

    if family in ("seed42", "offset1000"):
        s = oracle.init_state(n)
        for f in P:
            st[f] = getattr(s, f).astype(T)
            if precision == 64:  # the fp32-drawn cloud, plus low bits an fp32 number cannot hold
                st[f] = (st[f] * (1.0 + 2.0 ** -30 * rng.random(n))).astype(T)
            if family == "offset1000":
                st[f] = (st[f] + T(1000.0)).astype(T)  # rounded in T: the differences lose ten bits of the coordinates
        st["mass"] = s.mass.astype(T)
    elif family == "adversarial":  # the recipe of test_hand_scheduled_loop_bit_equal_on_adversarial_states, at any n
        centres = rng.random((16, 3))
        k = rng.integers(0, 16, n)
        spread = 10.0 ** rng.uniform(-7, -1, n)
        for a, f in enumerate(P):
            st[f] = (centres[k, a] + spread * rng.standard_normal(n)).astype(T)
            st[f][1::97] = st[f][0]                      # coincident bodies
        if n > 5:
            st["pos_x"][5] = T(3.0e3)                    # outlier
        m = 10.0 ** rng.uniform(-6, 6, n)                # twelve decades
        m[::13] = 0.0
        m[3::29] = 1e-22                                 # G m = 6.7e-33: times 1 / r^3 of the outlier far below the smallest normal float
        m[4::31] = 3e-26
        edges = tile_edges(n)
        m[edges] = 1e6 * (1.0 + rng.random(len(edges)))  # heavy bodies where an index fault would drop or repeat a record
        st["mass"] = m.astype(T)
    elif family == "lattice":  # equal masses on a regular grid in the unit box: interior accelerations cancel almost completely
        side = max(1, int(math.ceil(n ** (1.0 / 3.0) - 1e-9)))
        i = np.arange(n)
        h = 1.0 / side
        for a, f in enumerate(P):
            st[f] = (((i // side ** a) % side) * h).astype(T)
        st["mass"][:] = T(1.0)
    elif family == "signedbox":  # both signs, r >> eps
        for f in P:
            st[f] = uniform(-100.0, 100.0, n)
        st["mass"] = (n * rng.random(n)).astype(T)
    else:
        raise ValueError(family)
    return st


def hand_placed(precision=32):
    """Closed-form systems: (name, state, expected accelerations (n, 3) in fp64 from the formula written out by hand)."""
    T = np.float32 if precision == 32 else np.float64
    out = []

    def state(xs, ms):
        n = len(ms)
        st = {f: np.zeros(n, dtype=T) for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
        for f, col in zip(("pos_x", "pos_y", "pos_z"), zip(*xs)):
            st[f] = np.array(col, dtype=T)
        st["mass"] = np.array(ms, dtype=T)
        return st

    # two bodies on the x axis, 2 apart (all exactly representable): a_0 = +G m_1 2 / (4 + eps^2)^1.5 x, a_1 = -G m_0 2 / (...) x
    st = state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)], [3.0e9, 5.0e9])
    gm = gm_as_uploaded(st["mass"])
    f = 2.0 / (4.0 + EPS2) ** 1.5
    out.append(("n2_axis", st, np.array([[gm[1] * f, 0, 0], [-gm[0] * f, 0, 0]])))
    # a 3-4-5 triangle in the z = 0 plane (every distance exact): each body is pulled by the two others along the sides
    st = state([(0.0, 0.0, 0.0), (3.0, 0.0, 0.0), (0.0, 4.0, 0.0)], [4.0e9, 7.0e9, 2.0e9])
    gm = gm_as_uploaded(st["mass"])
    f3, f4, f5 = ((d * d + EPS2) ** -1.5 for d in (3.0, 4.0, 5.0))
    out.append(("n3_triangle", st, np.array([[gm[1] * 3 * f3, gm[2] * 4 * f4, 0],
                                             [-gm[0] * 3 * f3 - gm[2] * 3 * f5, gm[2] * 4 * f5, 0],
                                             [gm[1] * 3 * f5, -gm[0] * 4 * f4 - gm[1] * 4 * f5, 0]])))
    # one body: the only pair is j == i, which contributes exactly 0
    out.append(("n1", state([(0.3, 0.7, 0.9)], [5.0]), np.zeros((1, 3))))
    # a massive body and a massless one 1 apart along y: the massless one falls, the massive one feels nothing (A == 0)
    st = state([(0.0, 0.0, 0.0), (0.0, 1.0, 0.0)], [1.0e10, 0.0])
    gm = gm_as_uploaded(st["mass"])
    out.append(("n2_massless", st, np.array([[0, 0, 0], [0, -gm[0] / (1.0 + EPS2) ** 1.5, 0]])))
    return out
