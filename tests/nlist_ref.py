"""Numpy reference of the neighbour lists (include/nbx_nlist.h): for every body i of a system of n bodies the list of every j < n,
j != i with r2(i, j) = |x_j - x_i|^2 + eps^2 <= h2, ascending in j, with the r2; lists end to end behind offsets[].

nlist()        the plain definition in fp64, from the state as stored
restate()      the library's scheme, restated: per (split, body) counts under field_shape(n, n), the finish (per-split starts and
               within), the two-level exclusive scan over blocks of 2048 bodies, and the fill at offsets + the split's start, every
               store guarded by the end of its segment.  It takes the members of a batch call and has plantable FAULTS.
pick_radius()  fof_ref's chooser: a radius whose h2 lies in the middle of a gap of the pairs' r2 values, and ambiguous(), which
               says whether any pair -- or any body and a padding record -- has an r2 within WINDOW u of h2.  Where none has,
               every pair is decided the same way by the device's r2 (within 5 u of the exact value) and by the reference's, so
               the reference's lists are exact and the comparison leaves out nothing.

differs() is the comparison of the device tests: offsets, total and index EQUAL, every r2 within WINDOW u."""
import numpy as np

import fof_ref as F
import neighbours_ref as N
from energy_ref import EPS2

KEYS = ("offsets", "index", "r2", "total")
POS = N.POS
DTYPE = N.DTYPE
U = N.U
TILE = N.TILE
COLUMN = 512        # bodies per workgroup column: 256 lanes of two bodies
SCAN_BLOCK = 2048   # bodies per scan block (nbx_nlist_shape.hpp)
WINDOW = 8.0        # in u: nbx_neighbours' gate
SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1025, 2049, 4097)
DEGREES = (0.2, 6.0, 40.0)  # the expected number of neighbours per body of a uniform cloud: sparse, about 6, about 40
RAGGED_SIZES = N.RAGGED_SIZES
FAULTS = ("self not masked", "padding record not masked", "< instead of <=", "split starts in the wrong order",
          "a scan block's carry dropped", "inclusive scan", "global j in a batch", "offsets restarted per member",
          "the lane's second body writes at the first body's position")

h2_of = N.h2_of
pick_radius = F.pick_radius
target_radius = F.target_radius


def field_shape(m, n):
    """nbx_field_shape.hpp: (columns, tiles, splits, tiles per split)."""
    columns = (m + COLUMN - 1) // COLUMN
    tiles = (n + TILE - 1) // TILE
    s = max(1, min((1024 + columns - 1) // columns, tiles // 4))
    per = (tiles + s - 1) // s
    return columns, tiles, (tiles + per - 1) // per, per


def _xyz(state):
    return [np.asarray(state[c], dtype=np.float64) for c in POS]


def _r2_rows(x, lo, hi, xj=None):
    xj = x if xj is None else xj
    d = [xj[c][None, :] - x[c][lo:hi, None] for c in range(3)]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2


# ---- states ------------------------------------------------------------------------------------------------------------------------
def cloud(n, precision):
    """The uniform cloud the other analysis tests use (neighbours_ref.member)."""
    return N.member(n, precision)


def coincident(n, precision):
    """cloud(n) with the last body moved onto body 0 where there are two bodies or more: at radius 0 they list each other with
    r2 = eps2 and nobody else lists anybody (no other pair of a random cloud is at distance 0)."""
    s = {k: v.copy() for k, v in cloud(n, precision).items()}
    if n >= 2:
        for c in POS:
            s[c][n - 1] = s[c][0]
    return s


def radii_of(state):
    """The three chosen radii of a state: sparse, about 6 per body, about 40 per body."""
    n = len(state[POS[0]])
    return tuple(pick_radius(state, target_radius(n, d)) for d in DEGREES)


_cases = {}


def cases(precision, n):
    """The case table of one size: [(name, state, radius)] -- the cloud at its three chosen radii and at +inf (every list is all
    the others), and radius 0 on the state with two coincident bodies.  Computed once."""
    if (precision, n) not in _cases:
        st = cloud(n, precision)
        table = [("r%d" % q, st, r) for q, r in enumerate(radii_of(st))] + [("inf", st, float("inf")), ("zero", coincident(n, precision), 0.0)]
        _cases[(precision, n)] = table
    return _cases[(precision, n)]


ENSEMBLE = (3, 2049)
BATCH_DEGREE = 6.0


def ensemble_states(precision):
    """(the members' states of the 3 x 2049 ensemble, the one radius of its calls)."""
    S, n = ENSEMBLE
    states = [N.box(n, precision, seed=40 + k) for k in range(S)]
    return states, pick_radius(states, target_radius(n, BATCH_DEGREE))


def ragged_states(precision):
    """(the members' states of the ragged ensemble of RAGGED_SIZES, the one radius of its calls)."""
    states = [cloud(n, precision) for n in RAGGED_SIZES]
    return states, pick_radius(states, target_radius(1025, BATCH_DEGREE))


def ambiguous(state, radius, precision):
    """Whether any pair -- or any body and a padding record at the origin -- has an r2 within WINDOW u of h2."""
    if not np.isfinite(radius):
        return False
    h2 = h2_of(radius, precision)
    band = WINDOW * U[precision] * h2
    pairs, r2 = F.close_pairs(state, h2 + band)
    # two bodies at one position are not in question: every difference is 0 and r2 is eps2, exactly, in every precision
    x = _xyz(state)
    apart = np.zeros(len(pairs), dtype=bool)
    for c in range(3):
        apart |= x[c][pairs[:, 0]] != x[c][pairs[:, 1]]
    return bool((np.abs(r2[apart] - h2) <= band).any() or (np.abs(F._origin_r2(state) - h2) <= band).any())


# ---- the plain definition ----------------------------------------------------------------------------------------------------------
def nlist(state, radius, precision, chunk=512):
    x = _xyz(state)
    n = len(x[0])
    h2 = h2_of(radius, precision) if np.isfinite(radius) else np.inf
    counts = np.zeros(n, dtype=np.int64)
    idx, rr = [], []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        m = _r2_rows(x, lo, hi)
        hit = m <= h2
        hit[np.arange(hi - lo), np.arange(lo, hi)] = False
        counts[lo:hi] = hit.sum(axis=1)
        rows, cols = np.nonzero(hit)  # row-major: ascending j within a body
        idx.append(cols.astype(np.int32))
        rr.append(m[rows, cols])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return {"offsets": offsets, "index": np.concatenate(idx) if idx else np.zeros(0, np.int32),
            "r2": np.concatenate(rr) if rr else np.zeros(0), "total": int(offsets[-1])}


def concat(results):
    """The result of a batch call from its members' own: offsets continue, j stays member-local."""
    offsets, base = [np.zeros(1, dtype=np.int64)], 0
    for r in results:
        offsets.append(r["offsets"][1:] + base)
        base += r["total"]
    return {"offsets": np.concatenate(offsets), "index": np.concatenate([r["index"] for r in results]),
            "r2": np.concatenate([r["r2"] for r in results]), "total": base}


# ---- the library's scheme ----------------------------------------------------------------------------------------------------------
def scan(within, fault=None):
    """offsets[bodies + 1]: the exclusive prefix sum in two levels of SCAN_BLOCK."""
    within = np.asarray(within, dtype=np.int64)
    bodies = len(within)
    blocks = (bodies + SCAN_BLOCK - 1) // SCAN_BLOCK
    assert blocks <= SCAN_BLOCK
    padded = np.zeros(blocks * SCAN_BLOCK, dtype=np.int64)
    padded[:bodies] = within
    rows = padded.reshape(blocks, SCAN_BLOCK)
    sums = rows.sum(axis=1)                                   # launch one
    carry = np.cumsum(sums) - sums                            # launch two, one workgroup
    total = int(sums.sum())
    if fault == "a scan block's carry dropped":
        carry = np.zeros_like(carry)
    inside = np.cumsum(rows, axis=1)                          # launch three
    if fault != "inclusive scan":
        inside = inside - rows
    offsets = np.empty(bodies + 1, dtype=np.int64)
    offsets[:bodies] = (inside + carry[:, None]).reshape(-1)[:bodies]
    offsets[bodies] = total
    return offsets


def _hits(state, radius, precision, fault):
    """(hit [n, padded n] bool, r2 likewise) of one system under the masks, the padding records at the origin included."""
    x = _xyz(state)
    n = len(x[0])
    pad = (n + TILE - 1) // TILE * TILE
    xj = [np.concatenate([v, np.zeros(pad - n)]) for v in x]
    h2 = h2_of(radius, precision) if np.isfinite(radius) else np.inf
    m = _r2_rows(x, 0, n, xj)
    hit = (m < h2) if fault == "< instead of <=" else (m <= h2)
    if fault != "self not masked":
        hit[np.arange(n), np.arange(n)] = False
    if fault != "padding record not masked":
        hit[:, n:] = False
    return hit, m


def restate(states, radius, precision, fault=None):
    """The scheme over the members `states` of one call (a context: one state).  Unwritten entries stay -1 / NaN."""
    states = states if isinstance(states, (list, tuple)) else [states]
    per_member, within, first_body = [], [], [0]
    for st in states:
        n = len(st[POS[0]])
        _, tiles, splits, per = field_shape(n, n)
        hit, m = _hits(st, radius, precision, fault)
        bounds = [(s * per * TILE, min(tiles, (s + 1) * per) * TILE) for s in range(splits)]
        counts = np.stack([hit[:, lo:hi].sum(axis=1) for lo, hi in bounds])  # the count pass: [split][body]
        if fault == "split starts in the wrong order":
            starts = np.cumsum(counts[::-1], axis=0)[::-1] - counts            # the finish, walking the splits downwards
        else:
            starts = np.cumsum(counts, axis=0) - counts                        # the finish: ascending splits
        within.append(counts.sum(axis=0))
        per_member.append((n, hit, m, bounds, counts, starts))
        first_body.append(first_body[-1] + n)
    if fault == "offsets restarted per member":
        parts = [scan(w, fault) for w in within]
        offsets = np.concatenate([p[:-1] for p in parts] + [[sum(int(p[-1]) for p in parts)]]).astype(np.int64)
    else:
        offsets = scan(np.concatenate(within), fault)
    total = int(offsets[-1])
    index = np.full(total, -1, dtype=np.int32)
    r2 = np.full(total, np.nan)
    for k, (n, hit, m, bounds, counts, starts) in enumerate(per_member):
        off = offsets[first_body[k]:first_body[k] + n]
        body = np.arange(n)
        if fault == "the lane's second body writes at the first body's position":
            body = np.where(body % COLUMN >= COLUMN // 2, body - COLUMN // 2, body)
        for s, (lo, hi) in enumerate(bounds):
            rows, cols = np.nonzero(hit[:, lo:hi])  # a lane walks its body's pairs in ascending j
            if not len(rows):
                continue
            first_of_row = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])[rows]
            rank = np.arange(len(rows)) - first_of_row
            begin = off[body[rows]] + starts[s][body[rows]]
            end = begin + counts[s][body[rows]]
            pos = begin + rank
            ok = (pos < end) & (pos < total)  # the guard of every store
            j = lo + cols + (first_body[k] if fault == "global j in a batch" else 0)
            index[pos[ok]] = j[ok]
            r2[pos[ok]] = m[rows[ok], lo + cols[ok]]
    return {"offsets": offsets, "index": index, "r2": r2, "total": total}


# ---- the comparison of the device tests --------------------------------------------------------------------------------------------
def differs(got, want, precision):
    """What is wrong with `got` against `want`, as a list of texts (empty: nothing)."""
    out = []
    if int(got["total"]) != int(want["total"]):
        out.append("total %d != %d" % (got["total"], want["total"]))
    go, wo = np.asarray(got["offsets"]), np.asarray(want["offsets"])
    if go.shape != wo.shape or not np.array_equal(go, wo):
        out.append("offsets differ" + ("" if go.shape != wo.shape else " first at body %d" % int(np.nonzero(go != wo)[0][0])))
    gi, wi = np.asarray(got["index"]), np.asarray(want["index"])
    if gi.shape != wi.shape:
        out.append("index has %d entries, not %d" % (gi.size, wi.size))
    elif not np.array_equal(gi, wi):
        out.append("index differs first at entry %d" % int(np.nonzero(gi != wi)[0][0]))
    gr, wr = np.asarray(got["r2"], dtype=np.float64), np.asarray(want["r2"], dtype=np.float64)
    if gr.shape != wr.shape:
        out.append("r2 has %d entries, not %d" % (gr.size, wr.size))
    elif gr.size:
        bad = ~(np.abs(gr - wr) <= WINDOW * U[precision] * wr)
        if bad.any():
            out.append("r2 off at %d entries, first %d" % (int(bad.sum()), int(np.nonzero(bad)[0][0])))
    return out


def body_of_entry(offsets):
    """The body whose list entry e belongs to, for every entry."""
    offsets = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))


def components(nl, n):
    """Lowest-index labels of the connected components of the graph whose edges are the lists of one system."""
    i = body_of_entry(nl["offsets"])
    j = np.asarray(nl["index"], dtype=np.int64)
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, i, label[j])
        new = new[new]  # one hop of pointer jumping
        if np.array_equal(new, label):
            return label
        label = new


# ---- the lattice's closed form -----------------------------------------------------------------------------------------------------
def lattice_lists(k, m, precision, perm=False):
    """The lists of neighbours_ref.lattice(k, perm) at the radius lattice_ref.radius_of(m) from the geometry alone: every body on a
    site at squared lattice distance 1 ... m, ascending in the body index, r2 the bits of the distance class (knn_ref)."""
    import knn_ref
    n = k ** 3
    site = N.lattice_order(k, perm)
    body_of = np.empty(n, dtype=np.int64)
    body_of[site] = np.arange(n)
    ix, iy, iz = site // (k * k), (site // k) % k, site % k
    reach = int(np.floor(np.sqrt(m)))
    offs = [(a, b, c) for a in range(-reach, reach + 1) for b in range(-reach, reach + 1) for c in range(-reach, reach + 1)
            if 1 <= a * a + b * b + c * c <= m]
    body = np.empty((n, len(offs)), dtype=np.int64)
    d2 = np.empty((n, len(offs)), dtype=np.int64)
    for o, (a, b, c) in enumerate(offs):
        jx, jy, jz = ix + a, iy + b, iz + c
        ok = (jx >= 0) & (jx < k) & (jy >= 0) & (jy < k) & (jz >= 0) & (jz < k)
        body[:, o] = np.where(ok, body_of[np.where(ok, (jx * k + jy) * k + jz, 0)], n)
        d2[:, o] = a * a + b * b + c * c
    order = np.argsort(body, axis=1, kind="stable")
    body = np.take_along_axis(body, order, axis=1)
    d2 = np.take_along_axis(d2, order, axis=1)
    keep = body < n
    offsets = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    cls = d2[keep]
    r2 = np.zeros(cls.shape)
    for c in range(1, int(m) + 1):
        r2[cls == c] = knn_ref.lattice_class_r2(c, precision)
    return {"offsets": offsets, "index": body[keep].astype(np.int32), "r2": r2, "total": int(offsets[-1])}
