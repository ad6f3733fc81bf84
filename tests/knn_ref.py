"""numpy reference, in fp64, of include/nbx_knn.h: per body the k partners that are smallest under the order (r2, j), ascending,
and their softened squared distances -- from the state as stored, widened.

knn() is the plain definition.  restate() walks the pairs the way the kernels do -- j splits of field_shape(n, n), per split a
sorted list of the compiled capacity that a candidate enters by insertion on strict <, j ascending, the first k of every split's
list merged in ascending split order, again by insertion on strict < -- so that the faults a kernel of this structure can have
may be planted (FAULTS); without a fault the structure does not show in the result, which test_knn_cpu.py checks against knn().

Three comparisons hold a device result to the reference (differs()); the first two exclude nobody:
  (a) order statistics are stable: every r2[i, q] is within R2_GATE u of the reference's q-th value (u the unit round-off of T),
      and the fill (+inf) sits where the reference has it
  (b) every returned j is valid, differs from i and is distinct within its row (fill: j == -1 exactly where r2 is +inf), and its
      r2 recomputed in fp64 from the stored state is within R2_GATE u of the returned one
  (c) index is equal EXACTLY on the bodies ambiguous_mask() does not flag: a body is ambiguous when two consecutive values of
      its first k + 1 sorted r2 are within a relative 16 u (neighbours_ref.ambiguity's rule applied to every gap).  A test that
      relies on (c) asserts ambiguous() == 0 for its (state, k) first.  exact=True compares every index instead: for the lattice,
      whose r2 are exact and whose order among equal r2 is the rule under test.
"""
import numpy as np

import neighbours_ref as N
from energy_ref import EPS2
from field_ref import field_shape

KEYS = ("index", "r2")
POS = N.POS
DTYPE = N.DTYPE
U = N.U
TILE = N.TILE
R2_GATE = N.R2_GATE
RADIUS = N.RADIUS
SIZES = N.SIZES
RAGGED_SIZES = N.RAGGED_SIZES
KS = (1, 6, 8, 16)
KNN_MAX = 16
FAULTS = ("self not masked", "padding record not masked", "equal r2 displaces", "merge prefers the later split on ties",
          "displaced K-th entry lost", "last tile of the last split skipped", "no fill when n - 1 < k", "row not sorted after merge")

box, shifted, reversed_box, member, lattice, lattice_order = N.box, N.shifted, N.reversed_box, N.member, N.lattice, N.lattice_order


def capacity(k):
    """The compiled list capacity a call of width k runs with (knn_capacity of nbx_knn_kernels.hpp)."""
    return 4 if k <= 4 else 8 if k <= 8 else 16


def _xyz(state):
    return [np.asarray(state[c], dtype=np.float64) for c in POS]


def _r2_rows(x, lo, hi):
    d = [x[c][None, :] - x[c][lo:hi, None] for c in range(3)]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2


def _masked_rows(x, lo, hi):
    m = _r2_rows(x, lo, hi)
    m[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
    return m


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def knn(state, k, precision, chunk=512):
    """{"index": (n, k) int32, "r2": (n, k) float64} of the state as stored: the fp64 r2 matrix, np.lexsort on (j, r2), the first k
    partners of every row, fill where n - 1 < k; in row chunks."""
    x = _xyz(state)
    n = len(x[0])
    index = np.full((n, k), -1, dtype=np.int32)
    r2 = np.full((n, k), np.inf)
    have = min(k, n - 1)
    jj = np.arange(n)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        if have <= 0:
            break
        m = _masked_rows(x, lo, hi)
        order = np.lexsort((np.broadcast_to(jj, m.shape), m), axis=1)[:, :have]
        index[lo:hi, :have] = order
        r2[lo:hi, :have] = np.take_along_axis(m, order, axis=1)
    return {"index": index, "r2": r2}


def first_gap(state, precision, chunk=512):
    """Per body the first q at which its (q + 1)-th and (q + 2)-th smallest r2 are within a relative 16 u, KNN_MAX where there is
    none among its first KNN_MAX + 1: one pass that serves ambiguous_mask for every k."""
    x = _xyz(state)
    n = len(x[0])
    u = U[precision]
    gap = np.full(n, KNN_MAX, dtype=np.int64)
    have = min(KNN_MAX + 1, n - 1)
    if have < 2:
        return gap
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        m = _masked_rows(x, lo, hi)
        s = np.sort(np.partition(m, have - 1, axis=1)[:, :have], axis=1)
        close = s[:, 1:] <= s[:, :-1] * (1 + 16 * u)
        gap[lo:hi] = np.where(close.any(axis=1), close.argmax(axis=1), KNN_MAX)
    return gap


def ambiguous_mask(state, k, precision, gap=None):
    """Per body: two consecutive values of its first k + 1 sorted r2 are within a relative 16 u.  gap: first_gap's, if at hand."""
    return (first_gap(state, precision) if gap is None else gap) < k


def ambiguous(state, k, precision, gap=None):
    """The number of bodies ambiguous_mask flags."""
    return int(ambiguous_mask(state, k, precision, gap).sum())


# ---- the kernels' structure --------------------------------------------------------------------------------------------------------
def _insert(r, jx, c, jg, ties_displace=False, overwrite=False):
    """(c[i], jg[i]) into the ascending lists (r[i], jx[i]) of every row i whose candidate passes the compare against the row's
    last entry: behind every entry equal to it (strict <), the entries from there on shifted up, the last one falling out.
    ties_displace: <= instead of <, the candidate goes in front of its equals.  overwrite: no shift, the entry at the candidate's
    place is lost."""
    K = r.shape[1]
    last = r[:, K - 1]
    take = ((c <= last) & np.isfinite(c)) if ties_displace else (c < last)
    rows = np.nonzero(take)[0]
    if not len(rows):
        return
    cv = c[rows]
    jv = jg[rows] if isinstance(jg, np.ndarray) else np.full(len(rows), jg, dtype=np.int64)
    pos = ((r[rows] < cv[:, None]) if ties_displace else (r[rows] <= cv[:, None])).sum(axis=1)
    if not overwrite:
        for q in range(K - 1, 0, -1):
            sel = rows[pos < q]
            r[sel, q] = r[sel, q - 1]
            jx[sel, q] = jx[sel, q - 1]
    r[rows, pos] = cv
    jx[rows, pos] = jv


def restate(state, k, precision, fault=None):
    """The same values by the kernels' structure (the module's docstring).  `fault`: one of FAULTS, planted."""
    assert fault is None or fault in FAULTS, fault
    x = _xyz(state)
    n = len(x[0])
    K = capacity(k)
    _, tiles, splits, per = field_shape(n, n)
    n_rec = tiles * TILE  # the records of the position buffer: zero padding behind n
    xp = [np.concatenate([c, np.zeros(n_rec - n)]) for c in x]
    rows = []  # per split: the first k of every body's list
    for s in range(splits):
        j0, j1 = s * per * TILE, min(tiles, (s + 1) * per) * TILE
        if fault == "last tile of the last split skipped" and s == splits - 1:
            j1 -= TILE
        r = np.full((n, K), np.inf)
        jx = np.full((n, K), -1, dtype=np.int64)
        for j in range(j0, j1):
            d = [xp[c][j] - x[c] for c in range(3)]
            c = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
            if j >= n:
                if fault != "padding record not masked":
                    continue
            elif fault != "self not masked":
                c[j] = np.inf
            _insert(r, jx, c, j, ties_displace=fault == "equal r2 displaces", overwrite=fault == "displaced K-th entry lost")
        rows.append((r[:, :k].copy(), jx[:, :k].copy()))
    r = np.full((n, K), np.inf)
    jx = np.full((n, K), -1, dtype=np.int64)
    for rs, js in rows:  # ascending split order
        for q in range(k):
            _insert(r, jx, rs[:, q].copy(), js[:, q].copy(), ties_displace=fault == "merge prefers the later split on ties")
    r, jx = r[:, :k], jx[:, :k]
    if fault == "row not sorted after merge":  # the k best, but split after split instead of in one order
        key = np.where(jx >= 0, jx // (per * TILE), splits)
        order = np.argsort(key, axis=1, kind="stable")
        r, jx = np.take_along_axis(r, order, axis=1), np.take_along_axis(jx, order, axis=1)
    if fault == "no fill when n - 1 < k":  # the list's initial index is not -1
        jx = np.where(jx < 0, 0, jx)
    return {"index": jx.astype(np.int32), "r2": np.ascontiguousarray(r)}


# ---- the comparison of the device tests --------------------------------------------------------------------------------------------
def differs(got, want, state, precision, index=True, exact=False, gap=None):
    """What the device tests see between a result `got` and the reference `want` of the same (state, k): a list of findings,
    empty when comparisons (a), (b) and -- with index=True -- (c) of the module's docstring hold.  exact: (c) on every body.
    gap: first_gap's, if at hand."""
    out = []
    gi, gr = np.asarray(got["index"]), np.asarray(got["r2"], dtype=np.float64)
    wi, wr = np.asarray(want["index"]), np.asarray(want["r2"], dtype=np.float64)
    if gi.shape != wi.shape or gr.shape != wr.shape or gi.shape != gr.shape:
        return ["shapes %r %r against %r" % (gi.shape, gr.shape, wi.shape)]
    n, k = gi.shape
    u = U[precision]
    fin = np.isfinite(wr)
    # (a)
    if not np.array_equal(np.isfinite(gr), fin) or not np.array_equal(np.isposinf(gr), ~fin):
        out.append("(a) the fill is not where the reference has it")
    else:
        dev = np.abs(gr[fin] - wr[fin]) / wr[fin] / u
        if dev.size and dev.max() > R2_GATE:
            out.append("(a) r2 %.2f u from the reference's order statistic" % dev.max())
    # (b)
    fill = gi < 0
    if not np.array_equal(fill, ~np.isfinite(gr)) or (gi[fill] != -1).any():
        out.append("(b) index -1 and r2 +inf do not go together")
    if (gi >= n).any() or (gi == np.arange(n)[:, None]).any():
        out.append("(b) an index is no partner")
    else:
        s = np.sort(np.where(fill, -1 - np.arange(k)[None, :], gi), axis=1)
        if k > 1 and (s[:, 1:] == s[:, :-1]).any():
            out.append("(b) an index twice in a row")
        x = _xyz(state)
        j = np.clip(gi, 0, None)
        d = [x[c][j] - x[c][:, None] for c in range(3)]
        own = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
        ok = ~fill & np.isfinite(gr)
        dev = np.abs(gr[ok] - own[ok]) / own[ok] / u
        if dev.size and dev.max() > R2_GATE:
            out.append("(b) r2 %.2f u from the pair's own" % dev.max())
    # (c)
    if index:
        keep = np.ones(n, dtype=bool) if exact else ~ambiguous_mask(state, k, precision, gap)
        bad = np.nonzero((gi[keep] != wi[keep]).any(axis=1))[0]
        if len(bad):
            out.append("(c) %d bodies with another index, first %r" % (len(bad), np.nonzero(keep)[0][bad[:4]].tolist()))
    return out


# ---- the lattice's closed form -----------------------------------------------------------------------------------------------------
def lattice_class_r2(d2, precision):
    """The r2 of a lattice pair whose squared offset is d2 (in units of the spacing 1/8), as T evaluates it: the coordinates and
    the products are exact, so each fma rounds an exact sum once -- fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2))).  The offset is a
    permutation of the class's (a, b, c); every permutation gives the same bits (test_knn_cpu.py checks all of [-2, 2]^3)."""
    T = DTYPE[precision]
    best = None
    for a in range(3):
        for b in range(3):
            for c in range(3):
                if a * a + b * b + c * c == d2:
                    best = (a, b, c)
    t = T(EPS2)
    for o in best[::-1]:
        t = T((o / 8.0) * (o / 8.0) + float(t))
    return float(t)


def lattice_r2_of_offset(off, precision):
    """The same for one offset (dx, dy, dz), the fma chain in its own order."""
    T = DTYPE[precision]
    t = T(EPS2)
    for o in (off[2], off[1], off[0]):
        t = T((o / 8.0) * (o / 8.0) + float(t))
    return float(t)


def lattice_expected(kk, k, precision, perm=False):
    """{"index", "r2"} of lattice(kk, perm) for k <= 16 from the geometry alone: the partners within [-2, 2]^3 of a site -- enough
    at every site, corners included, where the 16th partner has d^2 = 5 -- sorted by (d^2, body index), r2 the class's bits."""
    assert 1 <= k <= 16 and kk >= 3
    n = kk ** 3
    site = lattice_order(kk, perm)
    body_of = np.empty(n, dtype=np.int64)
    body_of[site] = np.arange(n)
    ix, iy, iz = site // (kk * kk), (site // kk) % kk, site % kk
    offs = [(a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3) if (a, b, c) != (0, 0, 0)]
    d2 = np.empty((n, len(offs)), dtype=np.int64)
    body = np.empty((n, len(offs)), dtype=np.int64)
    for o, (a, b, c) in enumerate(offs):
        jx, jy, jz = ix + a, iy + b, iz + c
        ok = (jx >= 0) & (jx < kk) & (jy >= 0) & (jy < kk) & (jz >= 0) & (jz < kk)
        body[:, o] = np.where(ok, body_of[np.where(ok, (jx * kk + jy) * kk + jz, 0)], n)
        d2[:, o] = np.where(ok, a * a + b * b + c * c, 1 << 20)
    order = np.lexsort((body, d2), axis=1)[:, :k]
    index = np.take_along_axis(body, order, axis=1)
    cls = np.take_along_axis(d2, order, axis=1)
    assert (index < n).all() and cls.max() <= 5
    r2 = np.zeros(cls.shape)
    for c in range(1, 6):
        r2[cls == c] = lattice_class_r2(c, precision)
    return {"index": index.astype(np.int32), "r2": r2, "d2": cls}


# ---- the host helpers, restated as plain loops -------------------------------------------------------------------------------------
def local_density(res, mass):
    index, r2 = np.asarray(res["index"]), np.asarray(res["r2"], dtype=np.float64)
    n, k = index.shape
    rho = np.zeros(n)
    for i in range(n):
        if (index[i] < 0).any():
            continue
        d2 = max(r2[i, k - 1] - EPS2, 0.0)
        if d2 == 0.0:
            continue
        m = 0.0
        for q in range(k - 1):
            m += float(mass[index[i, q]])
        rho[i] = m / (4.0 / 3.0 * np.pi * d2 ** 1.5)
    return rho


def density_centre(x, y, z, rho):
    sw = 0.0
    c = [0.0, 0.0, 0.0]
    for i in range(len(rho)):
        sw += rho[i]
        for a, v in enumerate((x, y, z)):
            c[a] += rho[i] * float(v[i])
    c = [v / sw for v in c]
    num = den = 0.0
    for i in range(len(rho)):
        num += rho[i] ** 2 * sum((float(v[i]) - c[a]) ** 2 for a, v in enumerate((x, y, z)))
        den += rho[i] ** 2
    return np.array(c), float(np.sqrt(num / den))
