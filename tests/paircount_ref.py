"""numpy reference, in fp64, of include/nbx_paircount.h: the number of pairs i < j with r2(i, j) <= h2 for each of a list of radii
-- from the state as stored, widened.  The states, h2_of, U and SIZES are neighbours_ref's.

counts() is the plain count.  bracket() says what the device may return: the device's r2 carries up to 5 u and its h2 half a u,
u the unit round-off of T, so a pair whose fp64 r2 lies within a relative 8 u of h2 (neighbours_ref's window) may fall on either
side: lo counts the pairs surely inside, hi those possibly inside.  Where hi == lo the device is held to the exact count.

restate() walks the pairs the way the kernels do -- passes of at most 16 radii in slots of E = 4, 8 or 16, the unused slots at
h2 = -1; per pass the ORDERED pairs of every (split, column) of field_shape(n, n) against the zero-padded records; a finish that
adds a radius' records and halves -- so that the faults a kernel of this structure can have may be planted (FAULTS); without a
fault the structure does not show in the result, which test_paircount_cpu.py checks against counts().
"""
import numpy as np

from energy_ref import EPS2
from field_ref import field_shape
from neighbours_ref import (DTYPE, LATTICE_K, LATTICE_TIE_RADIUS, POS, RAGGED_SIZES, SIZES, TILE, U, box, h2_of, lattice,  # noqa: F401
                            member, reversed_box, shifted)

RADII = [0.03, 0.038, 0.049, 0.062, 0.079, 0.101, 0.128, 0.164, 0.209, 0.266, 0.339, 0.432, 0.55, 0.701, 0.893, 1.138, 1.45, 1.848,
         2.354, 3.0]  # twenty: two passes, E = 16 then E = 4
SLOTS = 16
COLUMN = 512
WINDOW = 8.0  # in u
LATTICE_RADII = [float(np.sqrt(m + 0.5) / 8.0) for m in range(1, 7)]  # between the shells of squared lattice distance m and m + 1
FAULTS = ("self counted", "padding record counted", "not halved", "< instead of <=", "last tile of the last split skipped",
          "second pass reuses the first pass's radii", "unused slot counted", "last column dropped by the finish")


def _x(state):
    return [np.asarray(state[k], dtype=np.float64) for k in POS]


def pair_r2(state, chunk=512):
    """The r2 of all pairs i < j of the state as stored, in fp64, sorted ascending."""
    x = _x(state)
    n = len(x[0])
    out = []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = [x[c][None, lo:] - x[c][lo:hi, None] for c in range(3)]
        m = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
        out.append(m[np.arange(lo, n)[None, :] > np.arange(lo, hi)[:, None]])
    r2 = np.concatenate(out) if out else np.zeros(0)
    r2.sort()
    return r2


def counts(state, radii, precision, r2=None):
    """counts[k] = #{i < j : r2(i, j) <= h2_k} as np.uint64; r2: pair_r2(state), where the caller has it already."""
    r2 = pair_r2(state) if r2 is None else r2
    return np.array([np.searchsorted(r2, h2_of(r, precision), side="right") for r in radii], dtype=np.uint64)


def bracket(state, radii, precision, r2=None):
    """Per radius (lo, hi), two np.uint64 arrays: lo = #{r2 < h2 (1 - 8 u)}, hi = #{r2 <= h2 (1 + 8 u)}."""
    r2 = pair_r2(state) if r2 is None else r2
    w = WINDOW * U[precision]
    lo = [np.searchsorted(r2, h2_of(r, precision) * (1.0 - w), side="left") for r in radii]
    hi = [np.searchsorted(r2, h2_of(r, precision) * (1.0 + w), side="right") for r in radii]
    return np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64)


def pass_slots(nradii):
    """[(first radius, radii held, E)] of the passes of a call: 16 per pass, the last in the smallest E that holds its remainder."""
    out = []
    for first in range(0, nradii, SLOTS):
        used = min(SLOTS, nradii - first)
        out.append((first, used, 4 if used <= 4 else 8 if used <= 8 else 16))
    return out


def restate(state, radii, precision, fault=None, finish_rows=None):
    """The same counts by the kernels' structure.  `fault`: one of FAULTS, planted.  "unused slot counted": the unused slots of a
    pass carry h2 = +inf and the finish folds every slot of the pass onto the radii the pass holds (slot s onto s mod used).
    finish_rows: a fault of its own -- the finish adds only the first finish_rows of the splits x columns records of a pass
    (record split * columns + column), as a strided loop that stops after its first round would."""
    assert fault is None or fault in FAULTS, fault
    x = _x(state)
    n = len(x[0])
    columns, tiles, splits, per = field_shape(n, n)
    n_rec = tiles * TILE  # the records of the position buffer: zero padding behind n
    xp = [np.concatenate([c, np.zeros(n_rec - n)]) for c in x]
    passes = pass_slots(len(radii))
    parts = np.zeros((len(passes), splits, columns, SLOTS), dtype=np.uint32)
    for p, (first, used, E) in enumerate(passes):
        src = 0 if (fault == "second pass reuses the first pass's radii" and p > 0) else first
        h2 = [h2_of(radii[src + s], precision) if s < used else (np.inf if fault == "unused slot counted" else -1.0) for s in range(E)]
        for col in range(columns):
            lo, hi = col * COLUMN, min(n, (col + 1) * COLUMN)
            d = [xp[c][None, :] - x[c][lo:hi, None] for c in range(3)]
            m = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
            ok = np.ones(m.shape, dtype=bool)
            if fault != "self counted":
                ok[np.arange(hi - lo), np.arange(lo, hi)] = False
            ok[:, n:] = fault == "padding record counted"
            for s in range(splits):
                j0, j1 = s * per * TILE, min(tiles, (s + 1) * per) * TILE
                if fault == "last tile of the last split skipped" and s == splits - 1:
                    j1 -= TILE
                v = np.sort(m[:, j0:j1][ok[:, j0:j1]]) if j1 > j0 else np.zeros(0)
                side = "left" if fault == "< instead of <=" else "right"
                parts[p, s, col, :E] = [np.searchsorted(v, h, side=side) for h in h2]
    out = np.zeros(len(radii), dtype=np.uint64)
    cols = columns - 1 if fault == "last column dropped by the finish" else columns
    for p, (first, used, E) in enumerate(passes):
        kept = parts[p, :, :cols, :].astype(np.uint64)
        if finish_rows is not None:
            kept = kept * (np.arange(splits)[:, None] * columns + np.arange(cols)[None, :] < finish_rows)[:, :, None].astype(np.uint64)
        total = kept.sum(axis=(0, 1))
        for s in range(E if fault == "unused slot counted" else used):
            out[first + s % used] += total[s]
    return out if fault == "not halved" else out >> np.uint64(1)


def lattice_counts(k, max_m):
    """counts[m - 1] = the pairs of a k^3 cubic lattice at squared lattice distance <= m, m = 1 ... max_m, from integer geometry
    alone: an offset (a, b, c) != 0 occurs (k - |a|)(k - |b|)(k - |c|) times among the ordered pairs."""
    r = int(np.sqrt(max_m))
    out = np.zeros(max_m, dtype=np.uint64)
    for a in range(-r, r + 1):
        for b in range(-r, r + 1):
            for c in range(-r, r + 1):
                d = a * a + b * b + c * c
                if 0 < d <= max_m:
                    out[d - 1:] += np.uint64(max(0, k - abs(a)) * max(0, k - abs(b)) * max(0, k - abs(c)))
    assert not (out & np.uint64(1)).any()
    return out >> np.uint64(1)


def lattice_face_pairs(k):
    """The face-neighbour pairs of a k^3 cubic lattice."""
    return 3 * k * k * (k - 1)
