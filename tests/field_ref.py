"""The field at caller-supplied points (include/nbx_field.h): truth, the K metrics and their gates, a numpy restatement of the
kernel's own order with plantable faults, and the states and point families the field tests share.  Used by
tests/test_field_cpu.py and tests/test_field_gpu.py; numpy only, no device.

Truth by augmentation: the m points are appended to the n bodies as bodies of mass 0.  force_ref.truth64 on rows n ... n + m - 1
of the augmented state gives a(p) and the scale A (a row's own term is an exact zero and the other points have no mass, so what
is left is the sum over the n bodies); potential_ref.weighted_inverse_distances with the masses as uploaded gives
-phi(p) = sum_j W_pj G m_j, where W_pp = 0 removes only the point itself, whose weight is 0 anyway.

Acceleration: K = force_ref.k_metric against that truth; K_ref: the same metric for force_ref.oracle_accel -- the reference's own
arithmetic, never a device value -- on the same augmented state and rows; gate = force_ref.gate(K_ref) = 2 max(K_ref, 16).
Potential: K = |phi - truth| / (u_T |truth|), all terms having one sign; K_ref: the same for phi_sequential(), a restatement in T
(differences, r^2, a correctly rounded 1 / sqrt, gm * inv, one sequential sum over j ascending); the same gate.

Restatement: the kernel's own order -- columns, splits and tiles per split from field_shape() (csrc/nbx_field_shape.hpp written
out again; tests/test_field_cpu.py holds it against the header through tests/field_shape_driver.cpp), a point's four sums in T
over a split, j ascending, the splits added in fp64 in split order and rounded once to T.  numpy has no FMA and its 1 / sqrt is
not v_rsq: a second correct evaluation of the same sums, not the device's bits.
"""
import numpy as np

import force_ref as F
import kick_ref as KR
import potential_ref as P
from energy_ref import EPS2, gm_as_uploaded

TILE = 256
COL = 512            # points per workgroup column: kBlock * kFieldPoints
MAX_POINTS = 1 << 22
POS = ("pos_x", "pos_y", "pos_z")
KEYS = ("acc_x", "acc_y", "acc_z", "phi")
DTYPE = {32: np.float32, 64: np.float64}
_ROWS = 512          # points per chunk of a restatement


def field_shape(m, n):
    """(columns, tiles, splits, tiles_per_split) of csrc/nbx_field_shape.hpp: field_shape(m, n)."""
    columns, tiles = -(-m // COL), -(-n // TILE)
    s = max(1, min(-(-1024 // columns), tiles // 4))
    per = -(-tiles // s)
    return columns, tiles, -(-tiles // per), per


# ---- states and points -------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 3), (255, 511), (256, 512), (257, 513), (513, 1), (2049, 1025), (4097, 2), (4097, 4097), (300, 2049))
FAMILIES = ("box", "own", "far", "heavy", "origin")
RAGGED_SIZES = (1, 2, 255, 257, 513, 2049, 300)


def families_of(n, m):
    """The point families a shape (n, m) is tested with."""
    out = ["box"]
    if m <= n:
        out.append("own")                       # the bodies' own positions
    if (n, m) in ((2, 3), (257, 513), (2049, 1025)):
        out.append("far")                       # 10^3 box sizes away
    if (n, m) in ((513, 1), (257, 513), (4097, 2)):
        out.append("heavy")                     # on a heavy body and 1e-4 beside it, force_ref's "adversarial" state
    if (n, m) in ((255, 511), (257, 513), (300, 2049)):
        out.append("origin")                    # all bodies 50 away in every coordinate; the origin and its neighbourhood
    return out


def cases():
    return [(n, m, fam) for n, m in SHAPES for fam in families_of(n, m)]


def make_state(precision, n, family):
    """The state of n bodies a family's points are asked of, in T."""
    T = DTYPE[precision]
    if family == "heavy":
        return F.make_state(None, "adversarial", n, precision)
    s = KR.make_state(4000 + n, n, np.float64)
    if family == "origin":
        for f in POS:
            s[f] = s[f] + 50.0
    return {k: np.ascontiguousarray(v.astype(T)) for k, v in s.items()}


def make_points(precision, state, m, family, seed=0):
    """(px, py, pz), each (m,) in T."""
    T = DTYPE[precision]
    n = len(state["mass"])
    rng = np.random.default_rng([77, n, m, FAMILIES.index(family), seed])
    lo = np.array([state[f].astype(np.float64).min() for f in POS])
    hi = np.array([state[f].astype(np.float64).max() for f in POS])
    size = max(float((hi - lo).max()), 1.0)
    if family == "box":
        p = lo[None, :] + (hi - lo)[None, :] * rng.random((m, 3))
    elif family == "own":
        assert m <= n
        p = np.stack([state[f][:m].astype(np.float64) for f in POS], axis=1)
    elif family == "far":
        d = rng.standard_normal((m, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        p = 0.5 * (lo + hi)[None, :] + 1.0e3 * size * d
    elif family == "heavy":
        e = F.tile_edges(n)                     # the heavy bodies of the adversarial state
        k = e[(np.arange(m) // 2) % len(e)]
        p = np.stack([state[f][k].astype(np.float64) for f in POS], axis=1)
        p[1::2, 0] += 1.0e-4
    elif family == "origin":
        p = rng.uniform(-0.5, 0.5, (m, 3))
        p[0] = 0.0
    else:
        raise ValueError(family)
    return tuple(np.ascontiguousarray(p[:, c].astype(T)) for c in range(3))


def augmented(state, points):
    """The state with the points appended as bodies of mass 0 (positions and masses only)."""
    out = {f: np.concatenate([state[f], np.asarray(p, dtype=state[f].dtype)]) for f, p in zip(POS, points)}
    out["mass"] = np.concatenate([state["mass"], np.zeros(len(points[0]), dtype=state["mass"].dtype)])
    return out


# ---- truth, metrics, gates ------------------------------------------------------------------------------------------------------------
def truth(state, points, precision):
    """{"acc": (hi, lo, A) of force_ref.truth64 for the m points, "phi": (hi, lo), hi + lo = phi(p) <= 0}."""
    n, m = len(state["mass"]), len(points[0])
    aug = augmented(state, points)
    gm = gm_as_uploaded(aug["mass"])
    rows = np.arange(n, n + m)
    acc = F.truth64([aug[f] for f in POS], gm, rows, precision)
    (w,) = P.weighted_inverse_distances([aug[f] for f in POS], [gm], precision)
    return {"acc": acc, "phi": (-w[0][rows], -w[1][rows])}


def truth_at(state, points, precision):
    """truth() without the detour through an augmented state, O(m n): the same sums, the n bodies as the only sources, in fp64
    for fp32 values and np.longdouble for fp64 values (tests/test_large_shapes_cpu.py holds it against truth()).  For shapes
    whose m^2 an augmented state cannot afford."""
    wide = precision == 64
    if wide and not F.HAVE_LONGDOUBLE:
        return truth(state, points, precision)
    dtype = np.longdouble if wide else np.float64
    m = len(points[0])
    x = [np.asarray(state[f]).astype(dtype) for f in POS]
    p = [np.asarray(c).astype(dtype) for c in points]
    g = gm_as_uploaded(state["mass"]).astype(dtype)
    hi, lo, A = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m)
    phi_hi, phi_lo = np.zeros(m), np.zeros(m)

    def split(s):
        h = s.astype(np.float64)
        return h, (s - h.astype(dtype)).astype(np.float64)

    def chunk(ab):
        a, b = ab
        d = [x[c][None, :] - p[c][a:b, None] for c in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + dtype(EPS2)
        w = g[None, :] / np.sqrt(r2)
        phi_hi[a:b], phi_lo[a:b] = split(-w.sum(axis=1))
        w /= r2
        for c in range(3):
            t = d[c] * w
            hi[a:b, c], lo[a:b, c] = split(t.sum(axis=1))
            A[a:b] = np.maximum(A[a:b], np.abs(t).sum(axis=1).astype(np.float64))

    P._pmap(chunk, F._row_chunks(m, len(g)))
    return {"acc": (hi, lo, A), "phi": (phi_hi, phi_lo)}


def k_acc(acc, tr, precision):
    """K per point of accelerations (m, 3) (or three arrays of m); where A == 0 the value must be exactly 0 (K = 0, else inf)."""
    a = np.stack([np.asarray(c) for c in acc], axis=1) if isinstance(acc, (list, tuple)) else np.asarray(acc)
    return F.k_metric(a, tr["acc"], precision)


def k_phi(phi, tr, precision):
    return P.k_metric(np.asarray(phi, dtype=np.float64), tr["phi"], precision)


def oracle_acc(oracle, state, points):
    """The reference's own arithmetic for a(p): the CPU oracle on the augmented state, rows n ... n + m - 1."""
    n, m = len(state["mass"]), len(points[0])
    return F.oracle_accel(oracle, augmented(state, points), np.arange(n, n + m))


def _inv_sqrt(r2, T):
    """1 / sqrt(r2) rounded once to T (evaluated in a wider type)."""
    if T == np.float32:
        return (1.0 / np.sqrt(r2.astype(np.float64))).astype(T)
    if F.HAVE_LONGDOUBLE:
        return (np.longdouble(1) / np.sqrt(r2.astype(np.longdouble))).astype(T)
    return T(1) / np.sqrt(r2)


FAULTS = ("dropped record", "doubled record", "padding record with mass", "last tile of the last split skipped",
          "split partial added twice", "point index shifted by one", "the lane's two points swapped", "phi without its sign")


def restate(state, points, precision, fault=None, one_split=False):
    """{"acc_x", "acc_y", "acc_z", "phi"}: arrays (m,) in T, in the kernel's own order (see the module docstring).

    fault = (name of FAULTS, p, j): one fault of the kind field_body / field_finish_kernel could have, at point p and record j
    (a split index for "split partial added twice"); names that need neither ignore them.  one_split: one sequential sum over all
    j (phi_sequential)."""
    T = DTYPE[precision]
    n, m = len(state["mass"]), len(points[0])
    columns, tiles, splits, per = field_shape(m, n)
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
    idx = np.arange(m)
    src = idx
    if name == "point index shifted by one":
        src = np.minimum(idx + 1, m - 1)
    elif name == "the lane's two points swapped":  # points l and l + 256 of one column sit in one lane
        partner = np.where(idx % COL < TILE, idx + TILE, idx - TILE)
        src = np.where(partner < m, partner, idx)
    pt = [np.asarray(p, dtype=T)[src] for p in points]
    parts = np.zeros((splits, m, 4), dtype=T)

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
            dx, dy, dz = (rec[c][None, j0:j1] - pt[c][a:b, None] for c in range(3))
            inv = _inv_sqrt(((T(EPS2) + dz * dz) + dy * dy) + dx * dx, T)
            gi = rec[3][None, j0:j1] * inv
            sf = gi * (inv * inv)
            terms = [dx * sf, dy * sf, dz * sf, gi]
            hit = name in ("dropped record", "doubled record") and a <= fp < b and j0 <= fj < j1
            extra = [t[fp - a, fj - j0] for t in terms] if hit else None
            if hit and name == "dropped record":
                for t in terms:
                    t[fp - a, fj - j0] = 0
            for c, t in enumerate(terms):
                parts[s, a:b, c] = np.add.accumulate(t, axis=1, dtype=T)[:, -1]
                if hit and name == "doubled record":
                    parts[s, fp, c] = T(parts[s, fp, c] + extra[c])

    P._pmap(chunk, [(a, min(a + _ROWS, m)) for a in range(0, m, _ROWS)])
    tot = np.zeros((m, 4))
    for s in range(splits):
        tot += parts[s].astype(np.float64)
        if name == "split partial added twice" and s == fj:
            tot += parts[s].astype(np.float64)
    out = tot.astype(T)
    return {"acc_x": out[:, 0], "acc_y": out[:, 1], "acc_z": out[:, 2], "phi": out[:, 3] if name == "phi without its sign" else -out[:, 3]}


def phi_sequential(state, points, precision):
    """phi(p) in T with one sequential sum over j ascending: what K_ref of the potential is measured on."""
    return restate(state, points, precision, one_split=True)["phi"]


# ---- one case, everything computed once -----------------------------------------------------------------------------------------------
_cases = {}


def case(oracle, precision, n, m, family):
    """{"state", "points", "truth", "gate_acc", "gate_phi", "kref_acc", "kref_phi"} of one (precision, n, m, family), cached."""
    key = (precision, n, m, family)
    if key not in _cases:
        state = make_state(precision, n, family)
        points = make_points(precision, state, m, family)
        tr = truth(state, points, precision)
        kref_acc = float(k_acc(oracle_acc(oracle, state, points), tr, precision).max())
        kref_phi = float(k_phi(phi_sequential(state, points, precision), tr, precision).max())
        _cases[key] = {"state": state, "points": points, "truth": tr, "kref_acc": kref_acc, "kref_phi": kref_phi,
                       "gate_acc": F.gate(kref_acc), "gate_phi": F.gate(kref_phi)}
    return _cases[key]


def worst(result, c, precision):
    """(largest K of the accelerations, largest K of phi) of a result dict over every point of case c."""
    ka = k_acc([result["acc_x"], result["acc_y"], result["acc_z"]], c["truth"], precision)
    kp = k_phi(result["phi"], c["truth"], precision)
    return float(ka.max()), float(kp.max())
