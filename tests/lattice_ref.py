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
"""
from decimal import Decimal, localcontext

import numpy as np

import neighbours_ref as NB
from energy_ref import EPS2, gm_as_uploaded
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
