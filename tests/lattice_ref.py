"""Closed forms on the k^3 cubic lattice of neighbours_ref.lattice(k, precision, perm) with every mass 1.0: what the pair-work
kernels must return at sizes where an O(n^2) reference cannot be run.  Used by tests/test_large_shapes_cpu.py (which holds every
closed form against brute force and against the O(n^2) references at small k) and tests/test_large_shapes_gpu.py; numpy only.

Among the ORDERED pairs of the lattice the displacement (a, b, c) != 0, |a|, |b|, |c| < k, in lattice units of 1/8, occurs
(k - |a|)(k - |b|)(k - |c|) times.  shell_weights(k)[d] is the sum of those weights over the displacements of squared length d:
every sum over pairs of a function of the distance is a sum over at most 3 (k - 1)^2 + 1 shells, O(k^3) to set up, whatever the
order of the bodies.  The counts are Python integers; the potential is summed in 50-digit decimal.

The planted lattice of the timescale checks is the lattice at rest with one body moved 1/16 towards a face neighbour (+x where
it has one, else -x: the coordinate stays a multiple of 1/16), given PLANT_SPEED in y and PLANT_MASS times the common mass: the
extreme pair of all three values involves that body, so they follow from the 2 (n - 1) ordered pairs it is part of, O(n), and
the closed-form background.

The lattice in Hubble flow (hubble: v = H x, every mass 1 / G) gives the velocity-reading kernels, nbx_timescale and
nbx_binaries, closed forms in which EVERY velocity record counts: hubble_timescale_expected in O(1), hubble_binaries_expected in
O(offsets n).  restate_timescale restates the two-tile structure of nbx_timescale's kernels so that the pairing faults of
binaries_ref.VELOCITY_FAULTS may be planted in it.
"""
from decimal import Decimal, localcontext

import numpy as np

import binaries_ref as BR
import neighbours_ref as NB
from energy_ref import EPS2, G32, gm_as_uploaded
from potential_ref import diag_shape
from timescale_ref import PLANT_MASS, PLANT_SPEED

POS = NB.POS
VEL = ("vel_x", "vel_y", "vel_z")
SHIFT = 1.0 / 16  # of the planted body
FACE_R2 = 1.0 / 64 + EPS2  # the softened squared distance of face neighbours: exact in fp64


def shell_weights(k):
    """w[d] = the number of ordered pairs at squared lattice distance d, d = 0 ... 3 (k - 1)^2 (w[0] = k^3: the bodies), int64."""
    a = np.arange(-(k - 1), k)
    w1 = (k - np.abs(a)).astype(np.int64)
    d = (a * a)[:, None, None] + (a * a)[None, :, None] + (a * a)[None, None, :]
    w = w1[:, None, None] * w1[None, :, None] * w1[None, None, :]
    assert k ** 6 < 2 ** 53  # bincount's float64 weights are then exact: every partial sum is an integer below k^6
    out = np.rint(np.bincount(d.ravel(), weights=w.ravel().astype(np.float64), minlength=3 * (k - 1) ** 2 + 1)).astype(np.int64)
    assert int(out.sum()) == k ** 6 and int(out[0]) == k ** 3
    return out


def pair_counts(k, squared_lattice_radii):
    """[the unordered pairs at squared lattice distance <= m for m in squared_lattice_radii], Python integers; m may be
    fractional (m + 0.5 is the device radius sqrt(m + 0.5) / 8) or math.inf."""
    w = shell_weights(k)
    cum = np.cumsum(w[1:])  # ordered pairs at 1 <= d <= index + 1
    out = []
    for m in squared_lattice_radii:
        top = min(int(np.floor(m)), len(w) - 1) if m < len(w) else len(w) - 1
        ordered = int(cum[top - 1]) if top >= 1 else 0
        assert ordered % 2 == 0
        out.append(ordered // 2)
    return out


def radius_of(m):
    """The device radius of squared lattice radius m + 0.5: mid-way between the shells m and m + 1."""
    return float(np.sqrt(m + 0.5) / 8.0)


def inverse_distance_sum(k):
    """sum over ordered pairs of 1 / sqrt(|d|^2 / 64 + eps^2), a Decimal of 50 digits."""
    w = shell_weights(k)
    with localcontext() as ctx:
        ctx.prec = 50
        e2 = Decimal(EPS2)
        total = Decimal(0)
        for d in np.nonzero(w)[0].tolist():
            if d:
                total += Decimal(int(w[d])) / (Decimal(d) / 64 + e2).sqrt()
        return total


def potential(k, precision):
    """(hi, lo), hi + lo = -1/2 sum_i m_i sum_{j != i} G m_j / sqrt(r_ij^2 + eps^2) for m = 1.0 and G m as uploaded in T."""
    gm = float(gm_as_uploaded(np.ones(1, dtype=NB.DTYPE[precision]))[0])
    with localcontext() as ctx:
        ctx.prec = 50
        u = -inverse_distance_sum(k) * Decimal(gm) / 2
        hi = float(u)
        return hi, float(u - Decimal(hi))


def state(k, precision, perm=False, at_rest=False):
    """neighbours_ref.lattice(k, precision, perm) with every mass 1.0; at_rest: every velocity 0."""
    s = NB.lattice(k, precision, perm)
    s["mass"] = np.ones(k ** 3, dtype=NB.DTYPE[precision])
    if at_rest:
        for f in VEL:
            s[f] = np.zeros(k ** 3, dtype=NB.DTYPE[precision])
    return s


def plant(rest, planted):
    """A copy of the lattice at rest `rest` with body `planted` as the module docstring says."""
    s = {f: v.copy() for f, v in rest.items()}
    T = s["mass"].dtype.type
    x = s["pos_x"]
    sign = 1.0 if float(x[planted]) < float(x.max()) else -1.0
    x[planted] = T(float(x[planted]) + sign * SHIFT)
    s["vel_y"][planted] = T(PLANT_SPEED)
    s["mass"][planted] = T(PLANT_MASS)
    return s


# ---- the lattice in Hubble flow ------------------------------------------------------------------------------------------------------
# Every body of the lattice moves at v = H x, H a power of two, and has the mass 1 / G: every velocity is exact in both
# precisions, v_j - v_i = H (x_j - x_i) exactly, and every pair quantity is a function of the squared lattice radius
# s = 64 |x_j - x_i|^2 alone.  A velocity read from another record than the position's breaks that: the pair's |dv|^2 is then
# H^2 |x_j' - x_i|^2, and whenever j' lies farther from i than j the approach rate exceeds H^2, the supremum of every true pair,
# and the pair's energy changes sign, which the exact integer `bound` of body i shows.  A lattice at rest shows none of it.
HUBBLE_H = (16.0, 8.0)  # the values the device tests use
HUBBLE_MASS = 1.0 / float(G32)


def hubble(k, precision, perm=False, H=16.0):
    """neighbours_ref.lattice(k, precision, perm) with v = H x and every mass 1 / G, rounded to T."""
    assert H > 0 and np.log2(H) == np.rint(np.log2(H))
    s = NB.lattice(k, precision, perm)
    T = NB.DTYPE[precision]
    for p, w in zip(POS, VEL):
        s[w] = np.ascontiguousarray((s[p].astype(np.float64) * H).astype(T))
        assert np.array_equal(s[w].astype(np.float64), s[p].astype(np.float64) * H)  # exact
    s["mass"] = np.full(k ** 3, HUBBLE_MASS, dtype=T)
    return s


def hubble_gm(precision):
    """G m of a body of hubble(.), as uploaded: 1 to a rounding."""
    return float(gm_as_uploaded(np.full(1, HUBBLE_MASS, dtype=NB.DTYPE[precision]))[0])


def hubble_timescale_expected(k, H, precision):
    """{approach_rate2, freefall_rate2, min_r2} of hubble(k, precision, ., H), in fp64, O(1): |dv|^2 / r2 = H^2 D^2 / (D^2 + eps^2)
    grows with the distance D, so the corner-to-corner pair holds it; the other two are the face pairs', timescale_background's
    with the Hubble lattice's G m."""
    d2 = 3.0 * ((k - 1) / 8.0) ** 2
    return {"approach_rate2": H * H * d2 / (d2 + EPS2), "freefall_rate2": 2.0 * hubble_gm(precision) / (FACE_R2 * np.sqrt(FACE_R2)),
            "min_r2": FACE_R2}


def hubble_energy(s, H, precision):
    """(e, A + B) in fp64 of a pair at squared lattice radius s (an array or a number): A = H^2 s / 128, B = 2 G m / sqrt(s / 64 +
    eps^2).  A grows and B falls with s: e is strictly increasing."""
    s = np.asarray(s, dtype=np.float64)
    a = 0.5 * H * H * s / 64.0
    b = 2.0 * hubble_gm(precision) / np.sqrt(s / 64.0 + EPS2)
    return a - b, a + b


def hubble_shell(k, H, precision):
    """(s_max, margin): the pairs of squared lattice radius <= s_max are the bound ones (e < 0), and margin is the smallest
    |e| / (A + B) over all radii a k^3 lattice has -- how far the nearest shell stays from e = 0."""
    s = np.arange(1, 3 * (k - 1) ** 2 + 1)
    e, mag = hubble_energy(s, H, precision)
    assert (np.diff(e) > 0).all()
    return int((e < 0).sum()), float((np.abs(e) / mag).min())


def hubble_binaries_expected(k, H, precision, perm=False):
    """{"partner", "bound", "energy", "mag"} of hubble(k, precision, perm, H) from the geometry: e grows with the distance, so
    the most bound partner is the lowest-numbered face neighbour (neighbours_ref.lattice_expected) and energy is e(1), one
    value, with mag its A + B; bound[i] is the number of lattice sites within squared radius s_max of body i's, summed over the
    integer offsets of that ball -- O(offsets n)."""
    n = k ** 3
    s_max, _ = hubble_shell(k, H, precision)
    site = NB.lattice_order(k, perm)
    c = (site // (k * k), (site // k) % k, site % k)
    reach = int(np.floor(np.sqrt(s_max)))
    bound = np.zeros(n, dtype=np.int64)
    for a in range(-reach, reach + 1):
        for b in range(-reach, reach + 1):
            for d in range(-reach, reach + 1):
                if 0 < a * a + b * b + d * d <= s_max:
                    ok = np.ones(n, dtype=bool)
                    for x, o in zip(c, (a, b, d)):
                        ok &= (x + o >= 0) & (x + o < k)
                    bound += ok
    e, mag = hubble_energy(1.0, H, precision)
    return {"partner": NB.lattice_expected(k, perm)[0], "bound": bound.astype(np.int32), "energy": float(e), "mag": float(mag)}


TS_VELOCITY_FAULTS = BR.VELOCITY_FAULTS


def restate_timescale(state, fault=None, member0=None, rows=None, chunk=256):
    """nbx_timescale's three values by the structure its kernels share with nbx_binaries' -- per j tile TWO staged arrays, the
    position records (zero padding behind n) and the velocity records of the same j, the j range in the splits of
    diag_shape(n, n) -- so that the ways of pairing the two arrays wrongly may be planted: `fault`, one of TS_VELOCITY_FAULTS
    (binaries_ref.velocity_map), `member0` as binaries_ref.restate's.  Without a fault: timescale_ref.timescale.  rows: the i side
    is these bodies alone (each against all j)."""
    assert fault is None or fault in TS_VELOCITY_FAULTS, fault
    x = [np.asarray(state[f], dtype=np.float64) for f in POS]
    v = [np.asarray(state[f], dtype=np.float64) for f in VEL]
    gm = gm_as_uploaded(state["mass"])
    n = len(gm)
    _, tiles, _, per = diag_shape(n, n)
    n_rec = tiles * BR.TILE
    vp = [np.concatenate([c, np.zeros(n_rec - n)]) for c in v]
    if fault == "velocity offset of the member not applied":
        vp = [np.resize(np.concatenate([np.asarray(member0[f], dtype=np.float64), c]), n_rec) for f, c in zip(VEL, v)]
    vmap = BR.velocity_map(n_rec, per, fault)
    if vmap is not None:
        vp = [np.where(vmap >= 0, c[np.maximum(vmap, 0)], 0.0) for c in vp]
    out = {"approach_rate2": 0.0, "freefall_rate2": 0.0, "min_r2": np.inf}
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    for lo in range(0, len(rows), chunk):
        i = rows[lo:lo + chunk]
        d = [c[None, :] - c[i, None] for c in x]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
        w = [cj[None, :n] - c[i, None] for cj, c in zip(vp, v)]
        approach = (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) / r2
        freefall = (gm[None, :] + gm[i, None]) / (r2 * np.sqrt(r2))
        own = (np.arange(len(i)), i)
        approach[own], freefall[own], r2[own] = 0.0, 0.0, np.inf
        out = {"approach_rate2": max(out["approach_rate2"], float(approach.max())), "freefall_rate2": max(out["freefall_rate2"], float(freefall.max())),
               "min_r2": min(out["min_r2"], float(r2.min()))}
    return out


def timescale_background(precision):
    """The three values of the lattice at rest, every mass 1.0 (k >= 2)."""
    gm = float(gm_as_uploaded(np.ones(1, dtype=NB.DTYPE[precision]))[0])
    return {"approach_rate2": 0.0, "freefall_rate2": 2.0 * gm / (FACE_R2 * np.sqrt(FACE_R2)), "min_r2": FACE_R2}


def timescale_expected(k, planted, precision, perm=False):
    """{approach_rate2, freefall_rate2, min_r2} of plant(state(k, precision, perm, at_rest=True), planted), in fp64: the
    extreme of the pairs that involve the planted body (a pair's values do not depend on its order) and of the background."""
    s = plant(state(k, precision, perm, at_rest=True), planted)
    d = [s[f].astype(np.float64) - float(s[f][planted]) for f in POS]
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
    r2[planted] = np.inf
    gm = gm_as_uploaded(s["mass"])
    out = timescale_background(precision)
    out["approach_rate2"] = max(out["approach_rate2"], float((PLANT_SPEED * PLANT_SPEED / r2).max()))
    out["freefall_rate2"] = max(out["freefall_rate2"], float(((gm + gm[planted]) / (r2 * np.sqrt(r2))).max()))
    out["min_r2"] = min(out["min_r2"], float(r2.min()))
    return out
