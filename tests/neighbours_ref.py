"""numpy reference, in fp64, of include/nbx_neighbours.h: per body the nearest neighbour (lowest index among equal r2), the softened
squared distance to it and the number of bodies within a radius -- from the state as stored, widened.

restate() walks the pairs the way the kernels do -- j splits of field_shape(n, n), a candidate per split, the splits combined in
ascending order -- so that the faults a kernel of this structure can have may be planted (FAULTS); without a fault the structure
does not show in the result, which test_neighbours_cpu.py checks against the plain argmin.

ambiguity() says whether a state can be held to EXACT equality of index and count on the device: u the unit round-off of T, a
body's nearest neighbour is ambiguous when its second-smallest r2 is within a relative 16 u of the smallest (the two r2 each
carry up to 5 u and a margin), its count when some r2 lies within a relative 8 u of h2 (the gate tests/test_timescale_gpu.py puts
on min_r2, the same arithmetic).  The states of the device tests have no ambiguous body at all (test_neighbours_cpu.py asserts it).
"""
import numpy as np

import kick_ref as K
from energy_ref import EPS2
from field_ref import field_shape

KEYS = ("index", "r2", "within")
POS = K.FIELDS[:3]
DTYPE = {32: np.float32, 64: np.float64}
U = {32: 2.0 ** -24, 64: 2.0 ** -53}
TILE = 256
R2_GATE = 8.0       # in u: r2 against the reference
RADIUS = 0.25       # box and shifted
LATTICE_RADIUS = 0.15  # between the face neighbours (1/8) and the edge neighbours (sqrt(2)/8)
LATTICE_TIE_RADIUS = 0.125  # h2 is bit for bit the face neighbours' r2
SEEDS = {257: 11, 2049: 12, 4097: 13}
SIZES = (257, 2049, 4097)
LATTICE_K = 13
FAULTS = ("self not masked", "padding record not masked", "ties to the highest j", "finish takes the last split on ties",
          "last tile of the last split skipped", "count includes self", "< instead of <=")


# ---- states ------------------------------------------------------------------------------------------------------------------------
def box(n, precision, seed=None):
    """kick_ref.make_state: positions uniform in [-1, 1]^3, stored in T."""
    return K.make_state(SEEDS[n] if seed is None else seed, n, DTYPE[precision])


def shifted(n, precision, seed=None):
    """box with 50 added to every coordinate: the origin, and the padding records that sit there, lie outside the system."""
    s = K.make_state(SEEDS[n] if seed is None else seed, n, np.float64)
    for k in POS:
        s[k] = s[k] + 50.0
    return {k: np.ascontiguousarray(v.astype(DTYPE[precision])) for k, v in s.items()}


def reversed_box(n, precision):
    """box(n) with the bodies in reverse order: another state -- other indices, other tiles -- of the same geometry."""
    return {k: np.ascontiguousarray(v[::-1]) for k, v in box(n, precision).items()}


RAGGED_SIZES = (1, 2, 255, 256, 257, 513, 1025, 2049)


def member(n, precision):
    """The state a ragged member of n bodies holds in the device tests: box(n) where it exists, else make_state(200 + n, n)."""
    return box(n, precision) if n in SEEDS else K.make_state(200 + n, n, DTYPE[precision])


def lattice_order(k, perm):
    """order[slot] = lattice site held by body `slot`: natural, or a fixed permutation."""
    return np.random.default_rng(5).permutation(k ** 3) if perm else np.arange(k ** 3)


def lattice(k, precision, perm=False):
    """k^3 cubic lattice of spacing 1/8 about the origin: every coordinate is exact in fp32, every interior body has six nearest
    neighbours with bit-identical r2.  Site (ix, iy, iz) is number (ix k + iy) k + iz; body `slot` sits on site order[slot]."""
    n = k ** 3
    s = K.make_state(100 + k, n, np.float64)
    site = lattice_order(k, perm)
    for name, c in zip(POS, (site // (k * k), (site // k) % k, site % k)):
        s[name] = (c - (k - 1) / 2.0) / 8.0
    return {k_: np.ascontiguousarray(v.astype(DTYPE[precision])) for k_, v in s.items()}


def lattice_expected(k, perm=False):
    """(index, within) of lattice(k, perm) from the geometry alone: the lowest-numbered body on a face-neighbour site, and the number
    of face neighbours (3 ... 6)."""
    n = k ** 3
    site = lattice_order(k, perm)
    body_of = np.empty(n, dtype=np.int64)
    body_of[site] = np.arange(n)
    ix, iy, iz = site // (k * k), (site // k) % k, site % k
    index = np.full(n, n, dtype=np.int64)
    within = np.zeros(n, dtype=np.int64)
    for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        jx, jy, jz = ix + dx, iy + dy, iz + dz
        ok = (jx >= 0) & (jx < k) & (jy >= 0) & (jy < k) & (jz >= 0) & (jz < k)
        cand = np.where(ok, body_of[np.where(ok, (jx * k + jy) * k + jz, 0)], n)
        index = np.minimum(index, cand)
        within += ok
    return index.astype(np.int32), within.astype(np.int32)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def h2_of(radius, precision):
    """fma(rT, rT, eps2) with rT = (T)radius, exactly (fp64 holds the product and the sum of the test radii without rounding
    in fp32; in fp64 it is the reference's own value)."""
    r = float(DTYPE[precision](radius))
    return r * r + EPS2


def _r2_rows(x, lo, hi):
    d = [x[c][None, :] - x[c][lo:hi, None] for c in range(3)]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2


def neighbours(state, radius, precision, chunk=512):
    """{"index", "r2", "within"} of the state as stored: the plain argmin (numpy's takes the first, i.e. lowest, index of equal
    values) and the plain count, in row chunks."""
    x = [np.asarray(state[k], dtype=np.float64) for k in POS]
    n = len(x[0])
    index = np.full(n, -1, dtype=np.int32)
    r2 = np.full(n, np.inf)
    within = np.zeros(n, dtype=np.int32)
    h2 = h2_of(radius, precision)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        m = _r2_rows(x, lo, hi)
        own = (np.arange(hi - lo), np.arange(lo, hi))
        within[lo:hi] = (m <= h2).sum(axis=1) - (m[own] <= h2)
        m[own] = np.inf
        if n > 1:
            j = m.argmin(axis=1)
            index[lo:hi] = j
            r2[lo:hi] = m[np.arange(hi - lo), j]
    return {"index": index, "r2": r2, "within": within}


def ambiguity(state, radius, precision, chunk=512):
    """(bodies whose nearest neighbour is ambiguous, bodies whose count is ambiguous) in the sense of the module's docstring."""
    x = [np.asarray(state[k], dtype=np.float64) for k in POS]
    n = len(x[0])
    u = U[precision]
    h2 = h2_of(radius, precision)
    bad_nn = bad_count = 0
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        m = _r2_rows(x, lo, hi)
        m[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        bad_count += int((np.abs(m - h2) <= 8 * u * h2).any(axis=1).sum())
        if n > 2:
            two = np.partition(m, 1, axis=1)[:, :2]
            bad_nn += int((two[:, 1] <= two[:, 0] * (1 + 16 * u)).sum())
    return bad_nn, bad_count


def restate(state, radius, precision, fault=None, chunk=512):
    """The same values by the kernels' structure: the j range in splits of field_shape(n, n), per split the lowest j of the
    smallest r2 (strict <, j ascending) and the count, the splits combined in ascending order on strict <.  `fault`: one of
    FAULTS, planted."""
    assert fault is None or fault in FAULTS, fault
    x = [np.asarray(state[k], dtype=np.float64) for k in POS]
    n = len(x[0])
    _, tiles, splits, per = field_shape(n, n)
    n_rec = tiles * TILE  # the records of the position buffer: zero padding behind n
    xp = [np.concatenate([c, np.zeros(n_rec - n)]) for c in x]
    h2 = h2_of(radius, precision)
    index = np.full(n, -1, dtype=np.int32)
    r2 = np.full(n, np.inf)
    within = np.zeros(n, dtype=np.int32)
    jj = np.arange(n_rec)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = [xp[c][None, :] - x[c][lo:hi, None] for c in range(3)]
        m = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
        ok = np.ones(m.shape, dtype=bool)
        own = (np.arange(hi - lo), np.arange(lo, hi))
        if fault != "self not masked":
            ok[own] = False
        ok[:, n:] = fault == "padding record not masked"
        inside = (m < h2) if fault == "< instead of <=" else (m <= h2)
        counted = ok.copy()
        if fault == "count includes self":
            counted[own] = True
        best = np.full(hi - lo, np.inf)
        bj = np.full(hi - lo, -1, dtype=np.int64)
        cnt = np.zeros(hi - lo, dtype=np.int64)
        for s in range(splits):
            j0, j1 = s * per * TILE, min(tiles, (s + 1) * per) * TILE
            if fault == "last tile of the last split skipped" and s == splits - 1:
                j1 -= TILE
            if j1 <= j0:
                continue
            part = np.where(ok[:, j0:j1], m[:, j0:j1], np.inf)
            if fault == "ties to the highest j":
                k = part.shape[1] - 1 - part[:, ::-1].argmin(axis=1)
            else:
                k = part.argmin(axis=1)
            cand = part[np.arange(hi - lo), k]
            take = (cand <= best) & np.isfinite(cand) if fault == "finish takes the last split on ties" else cand < best
            best = np.where(take, cand, best)
            bj = np.where(take, jj[j0:j1][k], bj)
            cnt += (inside[:, j0:j1] & counted[:, j0:j1]).sum(axis=1)
        index[lo:hi], r2[lo:hi], within[lo:hi] = bj, best, cnt
    return {"index": index, "r2": r2, "within": within}


def mutual_pairs(index):
    """The (i, j), i < j, with index[i] == j and index[j] == i, by the definition itself."""
    index = np.asarray(index)
    return np.array([(i, int(j)) for i, j in enumerate(index) if j > i and index[j] == i], dtype=np.int64).reshape(-1, 2)


def differs(got, want, precision):
    """What a comparison of the device tests sees between two results: index or within unequal anywhere, or an r2 beyond the gate."""
    if not np.array_equal(got["index"], want["index"]) or not np.array_equal(got["within"], want["within"]):
        return True
    fin = np.isfinite(want["r2"])
    if not np.array_equal(fin, np.isfinite(got["r2"])):
        return True
    return bool((np.abs(got["r2"][fin] - want["r2"][fin]) > R2_GATE * U[precision] * want["r2"][fin]).any())
