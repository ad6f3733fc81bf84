"""The tidal tensor at caller-supplied points and at the bodies (include/nbx_tidal.h): truth, the scale A, the K metric and its
gate, a numpy restatement of the kernel's own order with plantable faults, and the cases the tidal tests share.  Used by
tests/test_tidal_cpu.py and tests/test_tidal_gpu.py; numpy only, no device.  States, point families, SHAPES, RAGGED_SIZES and
field_shape are tests/field_ref.py's.

Truth, per component, O(m n): T_ab = sum_j G m_j (3 d_a d_b - delta_ab r2) r2^(-5/2) from the positions as stored in T and from
gm_as_uploaded, evaluated in fp64 for fp32 values and in np.longdouble for fp64 values (plain fp64 where the platform's long
double is a double); bodies mode leaves j == i out.  Scale: A_ab = sum_j G m_j (3 |d_a| |d_b| + delta_ab r2) r2^(-5/2), the
magnitudes of the two parts every term is the difference of.  K_ab = |got - truth| / (u_T A_ab), K the largest of the six; where
A_ab == 0 the value must be exactly 0 (K = 0, else inf).

Gate: 2 max(K_ref, floor), force_ref's gate with the floor include/nbx_tidal.h derives for one term to first order -- 30.5 u in
fp32, 24 u in fp64, both above force_ref's 16 u, so they take its place.  K_ref is the K of sequential(): the arithmetic of the
header restated in T with a correctly rounded 1 / sqrt, ONE sequential sum over j ascending and the finish formula -- never a
device value.

Restatement: restate() follows the kernel's own order -- columns, splits and tiles per split from field_shape(), two points per
lane, a point's seven sums in T over a split, j ascending, the masked tiles of bodies mode, the splits added in fp64 in split
order, 3 S_ab - delta_ab Q in fp64 rounded once to T.  numpy has no FMA and its 1 / sqrt is not v_rsq: a second correct
evaluation of the same sums, not the device's bits.
"""
import numpy as np

import field_ref as FR
import force_ref as F
import potential_ref as P
from energy_ref import EPS2, gm_as_uploaded

TILE, COL, POS, DTYPE = FR.TILE, FR.COL, FR.POS, FR.DTYPE
MAX_POINTS = 1 << 21
KEYS = ("t_xx", "t_xy", "t_xz", "t_yy", "t_yz", "t_zz")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
DIAG = (0, 3, 5)
FLOOR = {32: 30.5, 64: 24.0}  # include/nbx_tidal.h, "Error of one term"
BODY_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1025, 2049, 4097)
BODY_FAMILIES = ("cloud", "adversarial")
_ROWS = 512            # points per chunk of a restatement, at most
_ELEMENTS = 1 << 22    # pairs per chunk of a restatement, about


def gate(k_ref, precision):
    return F.M * max(float(k_ref), FLOOR[precision], F.K_TERM)


def _wide(precision):
    return np.longdouble if precision == 64 and F.HAVE_LONGDOUBLE else np.float64


def body_state(precision, n, family):
    """The state of n bodies a bodies-mode case is asked of, in T: a kick_ref cloud or force_ref's adversarial state."""
    if family == "adversarial":
        return F.make_state(None, "adversarial", n, precision)
    return FR.make_state(precision, n, "box")


def positions(state):
    return tuple(np.ascontiguousarray(state[f]) for f in POS)


# ---- truth, metric --------------------------------------------------------------------------------------------------------------------
def truth(state, points, precision, bodies=False, rows=None):
    """(hi, lo, A), each (len(rows), 6) fp64: hi + lo = T_ab at the points `rows` (default: all), A its scale.  bodies: the points
    are the bodies' own positions and point i leaves body i out."""
    dtype = _wide(precision)
    if bodies:
        points = positions(state)
    rows = np.arange(len(points[0])) if rows is None else np.asarray(rows, dtype=np.int64)
    x = [np.asarray(state[f]).astype(dtype) for f in POS]
    p = [np.asarray(c).astype(dtype)[rows] for c in points]
    g = gm_as_uploaded(state["mass"]).astype(dtype)
    k, n = len(rows), len(g)
    hi, lo, A = np.zeros((k, 6)), np.zeros((k, 6)), np.zeros((k, 6))

    def chunk(ab):
        a, b = ab
        d = [x[c][None, :] - p[c][a:b, None] for c in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + dtype(EPS2)
        w = np.broadcast_to(g[None, :], r2.shape) / (r2 * r2 * np.sqrt(r2))  # G m r2^(-5/2)
        if bodies:
            w = w.copy()
            w[np.arange(b - a), rows[a:b]] = 0
        q = w * r2
        for c, (i, j) in enumerate(PAIRS):
            t = 3 * d[i] * d[j] * w
            mag = np.abs(t)
            if i == j:
                t = t - q
                mag = mag + q
            s = t.sum(axis=1)
            hi[a:b, c] = s.astype(np.float64)
            lo[a:b, c] = (s - hi[a:b, c].astype(dtype)).astype(np.float64)
            A[a:b, c] = mag.sum(axis=1).astype(np.float64)

    P._pmap(chunk, F._row_chunks(k, n))
    return hi, lo, A


def as_array(result):
    """(m, 6) in the result's own dtype from a dict of the six KEYS (any shape, flattened) or an (m, 6) array."""
    if isinstance(result, dict):
        return np.stack([np.asarray(result[k]).reshape(-1) for k in KEYS], axis=1)
    return np.asarray(result)


def k_metric(result, tr, precision, rows=None):
    """K per point: the largest over the six components of |got - truth| / (u A); exact zeros where A == 0."""
    got = as_array(result)
    if rows is not None:
        got = got[np.asarray(rows)]
    hi, lo, A = tr
    err = np.abs((got.astype(np.float64) - hi) - lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(A > 0, err / (F.U[precision] * A), np.where(got == 0, 0.0, np.inf))
    return k.max(axis=1)


def trace_truth(state, points, precision, bodies=False, rows=None):
    """-3 eps^2 sum_j G m_j r2^(-5/2) in fp64 (wide arithmetic): what T_xx + T_yy + T_zz must be."""
    dtype = _wide(precision)
    if bodies:
        points = positions(state)
    rows = np.arange(len(points[0])) if rows is None else np.asarray(rows, dtype=np.int64)
    x = [np.asarray(state[f]).astype(dtype) for f in POS]
    p = [np.asarray(c).astype(dtype)[rows] for c in points]
    g = gm_as_uploaded(state["mass"]).astype(dtype)
    out = np.zeros(len(rows))
    for a, b in F._row_chunks(len(rows), len(g)):
        d = [x[c][None, :] - p[c][a:b, None] for c in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + dtype(EPS2)
        w = np.broadcast_to(g[None, :], r2.shape) / (r2 * r2 * np.sqrt(r2))
        if bodies:
            w = w.copy()
            w[np.arange(b - a), rows[a:b]] = 0
        out[a:b] = (-3 * dtype(EPS2) * w.sum(axis=1)).astype(np.float64)
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
FAULTS = ("dropped record", "doubled record", "padding record with mass", "last tile of the last split skipped",
          "split partial added twice", "point index shifted by one", "the lane's two points swapped", "xy and yz exchanged",
          "the factor 3 missing", "Q not subtracted", "the self term kept in bodies mode", "a neighbour masked instead of self")


def restate(state, points, precision, bodies=False, fault=None, one_split=False, rows=None):
    """(m, 6) in T, in the kernel's own order (see the module docstring); rows: only these points of the m, (len(rows), 6).

    fault = (name of FAULTS, p, j): one fault of the kind tidal_body / tidal_finish_kernel could have, at point p and record j (a
    split index for "split partial added twice"); names that need neither ignore them.  one_split: one sequential sum over all j
    (sequential())."""
    T = DTYPE[precision]
    if bodies:
        points = positions(state)
    n, m = len(state["mass"]), len(points[0])
    columns, tiles, splits, per = FR.field_shape(m, n)
    if one_split:
        splits, per = 1, tiles
    name, fp, fj = fault if fault else (None, -1, -1)
    assert name is None or name in FAULTS, name
    npad = tiles * TILE
    rec = [np.zeros(npad, dtype=T) for _ in range(4)]
    for c, f in zip(rec, POS):
        c[:n] = state[f]
    rec[3][:n] = gm_as_uploaded(np.asarray(state["mass"], dtype=T)).astype(T)  # exact: the product was rounded in T
    if name == "padding record with mass":
        assert n < npad
        rec[3][n] = rec[3][:n].max()
    assert rows is None or name is None
    idx = np.arange(m) if rows is None else np.asarray(rows, dtype=np.int64)
    src = idx
    if name == "point index shifted by one":
        src = np.minimum(idx + 1, m - 1)
    elif name == "the lane's two points swapped":  # points l and l + 256 of one column sit in one lane
        partner = np.where(idx % COL < TILE, idx + TILE, idx - TILE)
        src = np.where(partner < m, partner, idx)
    pt = [np.asarray(p, dtype=T)[src] for p in points]
    own = idx.copy()  # the record a body masks: its own
    if name == "a neighbour masked instead of self":
        own = np.where(idx + 1 < n, idx + 1, idx - 1)
    k = len(idx)
    parts = np.zeros((splits, k, 7), dtype=T)

    def chunk(ab):
        a, b = ab
        for s in range(splits):
            k0 = s * per
            k1 = min(tiles, k0 + per)
            if name == "last tile of the last split skipped" and s == splits - 1:
                k1 -= 1
            j0, j1 = k0 * TILE, k1 * TILE
            if j1 <= j0:
                continue
            d = [rec[c][None, j0:j1] - pt[c][a:b, None] for c in range(3)]
            inv = FR._inv_sqrt(((T(EPS2) + d[2] * d[2]) + d[1] * d[1]) + d[0] * d[0], T)
            g = np.broadcast_to(rec[3][None, j0:j1], inv.shape)
            if bodies and name != "the self term kept in bodies mode":  # only the column's own two tiles hold a masked record
                g = g.copy()
                hit = (own[a:b] >= j0) & (own[a:b] < j1)
                g[np.nonzero(hit)[0], own[a:b][hit] - j0] = 0
            inv2 = inv * inv
            s3 = (g * inv) * inv2
            s5 = s3 * inv2
            u = [d[c] * s5 for c in range(3)]
            terms = [u[i] * d[j] for i, j in PAIRS] + [s3]
            here = name in ("dropped record", "doubled record") and a <= fp < b and j0 <= fj < j1
            extra = [t[fp - a, fj - j0] for t in terms] if here else None
            if here and name == "dropped record":
                for t in terms:
                    t[fp - a, fj - j0] = 0
            for c, t in enumerate(terms):
                parts[s, a:b, c] = np.add.accumulate(t, axis=1, dtype=T)[:, -1]
                if here and name == "doubled record":
                    parts[s, fp, c] = T(parts[s, fp, c] + extra[c])

    step = max(1, min(_ROWS, _ELEMENTS // npad))
    P._pmap(chunk, [(a, min(a + step, k)) for a in range(0, k, step)])
    tot = np.zeros((k, 7))
    for s in range(splits):
        tot += parts[s].astype(np.float64)
        if name == "split partial added twice" and s == fj:
            tot += parts[s].astype(np.float64)
    out = (1.0 if name == "the factor 3 missing" else 3.0) * tot[:, :6]
    if name != "Q not subtracted":
        out[:, DIAG] -= tot[:, 6:7]
    out = out.astype(T)
    if name == "xy and yz exchanged":
        out = out[:, [0, 4, 2, 3, 1, 5]]
    return out


def sequential(state, points, precision, bodies=False, rows=None):
    """T_ab in T with one sequential sum over j ascending: what K_ref is measured on."""
    return restate(state, points, precision, bodies=bodies, one_split=True, rows=rows)


# ---- one case, everything computed once -----------------------------------------------------------------------------------------------
_cases = {}


def point_cases():
    return FR.cases()


def body_cases():
    return [(n, fam) for n in BODY_SIZES for fam in BODY_FAMILIES]


def _finish(state, points, precision, bodies):
    tr = truth(state, points, precision, bodies=bodies)
    kref = float(k_metric(sequential(state, points, precision, bodies=bodies), tr, precision).max())
    return {"state": state, "points": points, "truth": tr, "kref": kref, "gate": gate(kref, precision), "bodies": bodies}


def case(precision, n, m, family):
    """Points mode: {"state", "points", "truth", "kref", "gate", "bodies"} of one (precision, n, m, family) of field_ref, cached."""
    key = (precision, n, m, family)
    if key not in _cases:
        state = FR.make_state(precision, n, family)
        _cases[key] = _finish(state, FR.make_points(precision, state, m, family), precision, False)
    return _cases[key]


def body_case(precision, n, family):
    """Bodies mode: the same of one (precision, n, family of BODY_FAMILIES), cached; "points" are the bodies' own positions."""
    key = (precision, n, "bodies", family)
    if key not in _cases:
        state = body_state(precision, n, family)
        _cases[key] = _finish(state, positions(state), precision, True)
    return _cases[key]


def worst(result, c, precision):
    """The largest K of a result (dict of KEYS or (m, 6)) over every point of case c."""
    return float(k_metric(result, c["truth"], precision).max())
