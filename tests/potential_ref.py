"""The heavy-body probe of the potential-energy kernels (csrc/nbx_diag_body.hpp: diag_tile, diag_body): states, a high-precision
truth, the K metric, a numpy restatement of the kernel's own arithmetic with plantable faults, and the positions worth probing.
Used by tests/test_potential_probe_cpu.py and tests/test_potential_probe_gpu.py; numpy only, no device.

nbx_diag_t has no per-body potential, so the probe makes one body matter.  In heavy_state(base, k) body k has mass 1 and every
other body a mass of 2^-40 (1 + r_i).  With s = sum_i m_i phi_i, the total is then, up to the light-light pairs (n 2^-40 of it,
present in the truth as well), the sum of two halves of equal size:

    the row of k     m_k sum_j G m_j / r_kj           the lane that holds body k reading every record
    the column of k  sum_{i != k} m_i G m_k / r_ik    every other lane reading record k

so ONE pair (k, j) dropped, doubled or wrongly masked moves the total by 1 / (2 n) of itself: 2^23 / n units of 2^-24, 2046 at
n = 4099 -- and an admitted self term, m_k G m_k / eps, by many orders more.  The gate below is 32 units.  r_i is a multiple of
2^-10, so that every sum of the masses is exact in fp64 whatever its order (mass is compared exactly).

truth_heavy() needs the inverse-distance matrix W of the base once (fp64 for fp32 states; np.longdouble, or force_ref's
double-double where long double is a double, for fp64 states): two matrix-vector products, then per k in O(1), with s the
light masses, g = G s as uploaded, O the owned rows and s_O = s on O, 0 elsewhere:

    Sigma_k = s_O . W g  +  [k in O] (m_k - s_k) (W g)_k  +  (G m_k - g_k) (W s_O)_k          U_k = -Sigma_k / 2

(the pair (k, k) carries W_kk = 0).  Every truth is a pair (hi, lo) of fp64 numbers, hi + lo the value.

Metric and gate are force_ref's: K = |U_got - U_true| / (u_T |U_true|) -- all terms have one sign, so |U_true| is the
sum-of-|terms| scale -- and K <= gate(K_ref) = 2 max(K_ref, 16), K_ref the K of Restatement, never a device value.
"""
import math
from concurrent.futures import ThreadPoolExecutor
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

import force_ref as R
from energy_ref import EPS2, gm_as_uploaded

TILE = 256           # records per LDS tile (kTile)
COL = 512            # bodies per workgroup column: kBlock * kDiagBodies, two bodies per lane in both precisions
LIGHT = 2.0 ** -40
POS = ("pos_x", "pos_y", "pos_z")
FIELDS = POS + ("vel_x", "vel_y", "vel_z", "mass")


def _pmap(fn, items):
    """[fn(x) for x in items] on force_ref's thread pool size (numpy releases the GIL inside its loops)."""
    items = list(items)
    if R._THREADS > 1 and len(items) > 1:
        with ThreadPoolExecutor(R._THREADS) as ex:
            return list(ex.map(fn, items))
    return [fn(x) for x in items]


def dtype_of(precision):
    return np.float32 if precision == 32 else np.float64


def diag_shape(i_count, n):
    """(cols, tiles, splits, tiles_per_split) of diag_kernel for i_count owned bodies of n: diag_splits of csrc/nbx_diag_shape.hpp
    written out again (tests/test_potential_probe_cpu.py holds it against the header through the planner's driver)."""
    cols, tiles = -(-i_count // COL), -(-n // TILE)
    s = max(1, min(-(-1024 // cols), tiles // 4))
    per = -(-tiles // s)
    return cols, tiles, -(-tiles // per), per


# ---- states ------------------------------------------------------------------------------------------------------------------------
def light_masses(n, precision, seed=7):
    r = np.random.default_rng([seed, n]).integers(0, 1024, n) / 1024.0
    return (LIGHT * (1.0 + r)).astype(dtype_of(precision))


def _blank(base, precision):
    T = dtype_of(precision)
    n = len(base["mass"])
    st = {f: np.zeros(n, dtype=T) for f in FIELDS}
    for f in POS:
        st[f] = np.asarray(base[f]).astype(T)
    return st


def heavy_state(base, k, precision):
    """The positions of `base`, at rest; m_k = 1, every other mass light_masses()."""
    st = _blank(base, precision)
    st["mass"] = light_masses(len(base["mass"]), precision)
    st["mass"][k] = 1.0
    return st


def heavy_states(base, ks, precision):
    """(k, heavy_state(base, k, precision)) for k in ks, one set of arrays reused: a state is valid until the next is drawn."""
    st = heavy_state(base, 0, precision)
    light = light_masses(len(base["mass"]), precision)
    for k in ks:
        st["mass"][:] = light
        st["mass"][int(k)] = 1.0
        yield int(k), st


def pair_state(base, k, j, precision, mk, mj, sep=None):
    """All masses 0 but m_k and m_j: the per-pair probe.  sep: body j is put at x_k + (sep, 0, 0), rounded in T (0: coincident)."""
    st = _blank(base, precision)
    if sep is not None:
        for f in POS:
            st[f][j] = st[f][k]
        st["pos_x"][j] = st["pos_x"][k] + st["pos_x"].dtype.type(sep)
    st["mass"][k], st["mass"][j] = mk, mj
    return st


def pair_truth(st, k, j):
    """(hi, lo) of U = -1/2 (m_k G m_j + m_j G m_k) / sqrt(r^2 + eps^2) for the state's T values, in 60-digit decimal."""
    gm = gm_as_uploaded(st["mass"])
    with localcontext() as ctx:
        ctx.prec = 60
        D = lambda v: Decimal(float(v))
        r2 = sum(((D(st[f][j]) - D(st[f][k])) ** 2 for f in POS), D(EPS2))
        u = -(D(st["mass"][k]) * D(gm[j]) + D(st["mass"][j]) * D(gm[k])) / (2 * r2.sqrt())
        hi = float(u)
        return hi, float(u - D(hi))


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
def weighted_inverse_distances(pos, vecs, precision, force_dd=False):
    """[(hi, lo), ...], one per vector v of `vecs`: hi_i + lo_i = sum_j W_ij v_j with W_ij = 1 / sqrt(|x_j - x_i|^2 + eps^2), W_ii = 0,
    for every body i.  fp32 positions: fp64 (lo = 0).  fp64 positions: np.longdouble, or double-double (force_dd)."""
    n = len(np.asarray(pos[0]))
    wide = precision == 64
    dd = wide and (force_dd or not R.HAVE_LONGDOUBLE)
    out = [(np.zeros(n), np.zeros(n)) for _ in vecs]

    def chunk(ab):
        rows = np.arange(*ab)
        if dd:
            c3 = [np.asarray(c, dtype=np.float64) for c in pos]
            d = [R._two_sum(c[None, :], -c[rows, None]) for c in c3]
            zero = np.zeros_like(d[0][0])
            r2 = (zero + EPS2, zero)
            for c in d:
                r2 = R._dd_add(r2, R._dd_mul(c, c))
            y0 = 1.0 / np.sqrt(r2[0])  # then one Newton step carried in double-double, as force_ref._dd_term_rows
            e = R._dd_add((zero + 1.0, zero), tuple(-v for v in R._dd_mul(r2, R._two_prod(y0, y0))))
            w = list(R._two_sum(y0, y0 * (e[0] + e[1]) * 0.5))
            for part in w:
                part[rows - ab[0], rows] = 0.0
            for (hi, lo), v in zip(out, vecs):
                hi[rows], lo[rows] = R._dd_rowsum(R._dd_mul(tuple(w), (np.asarray(v, dtype=np.float64)[None, :] + zero, zero)))
            return
        dtype = np.longdouble if wide else np.float64
        x, y, z = (np.asarray(c).astype(dtype) for c in pos)
        dx, dy, dz = x[None, :] - x[rows, None], y[None, :] - y[rows, None], z[None, :] - z[rows, None]
        w = 1.0 / np.sqrt(dx * dx + dy * dy + dz * dz + dtype(EPS2))
        w[rows - ab[0], rows] = 0.0
        for (hi, lo), v in zip(out, vecs):
            s = (w * np.asarray(v).astype(dtype)[None, :]).sum(axis=1)  # pairwise in numpy: far below u_T in `dtype`
            hi[rows] = s.astype(np.float64)
            lo[rows] = (s - hi[rows].astype(dtype)).astype(np.float64)

    _pmap(chunk, R._row_chunks(n, n))
    return out


def _F(hi, lo=0.0):
    return Fraction(float(hi)) + Fraction(float(lo))


def _hi_lo(f):
    hi = float(f)
    return hi, float(f - Fraction(hi))


def _dot(m, hl):
    """sum_i m_i (hi_i + lo_i) as a Fraction: exact products (two_prod), exactly rounded sums (fsum)."""
    m = np.asarray(m, dtype=np.float64)
    p, e = R._two_prod(m, hl[0])
    v = np.concatenate([p, e, m * hl[1]]).tolist()
    hi = math.fsum(v)
    return _F(hi, math.fsum(v + [-hi]))


def truth_total(state, precision, i_begin=0, i_count=None, force_dd=False):
    """(hi, lo) of the potential partial of the bodies [i_begin, i_begin + i_count) of any state, masses as uploaded."""
    n = len(state["mass"])
    own = slice(i_begin, n if i_count is None else i_begin + i_count)
    (wg,) = weighted_inverse_distances([state[f] for f in POS], [gm_as_uploaded(state["mass"])], precision, force_dd)
    return _hi_lo(-_dot(np.asarray(state["mass"])[own], (wg[0][own], wg[1][own])) / 2)


def truth_heavy(base, ks, precision, i_begin=0, i_count=None, force_dd=False):
    """(hi, lo), arrays over ks: the potential partial of the owned bodies for heavy_state(base, k, precision)."""
    n = len(base["mass"])
    T = dtype_of(precision)
    own = slice(i_begin, n if i_count is None else i_begin + i_count)
    s = light_masses(n, precision).astype(np.float64)
    g = gm_as_uploaded(light_masses(n, precision))
    s_own = np.zeros(n)
    s_own[own] = s[own]
    wg, ws = weighted_inverse_distances([np.asarray(base[f]).astype(T) for f in POS], [g, s_own], precision, force_dd)
    B = _dot(s[own], (wg[0][own], wg[1][own]))
    mk, gmk = Fraction(1), _F(gm_as_uploaded(np.ones(1, dtype=T))[0])
    hi, lo = np.zeros(len(ks)), np.zeros(len(ks))
    for a, k in enumerate(ks):
        k = int(k)
        sigma = B + (gmk - _F(g[k])) * _F(ws[0][k], ws[1][k])
        if own.start <= k < own.stop:
            sigma += (mk - _F(s[k])) * _F(wg[0][k], wg[1][k])
        hi[a], lo[a] = _hi_lo(-sigma / 2)
    return hi, lo


def k_metric(got, truth, precision):
    """K of potentials `got` against truth = (hi, lo); got - hi is exact wherever K is small (Sterbenz).  A truth of 0 (no owned
    pair has two masses) must be met exactly: K = 0 if so, inf if not."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    hi, lo = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in truth)
    err = np.abs((got - hi) - lo)
    K = np.where(err == 0, 0.0, np.inf)
    nz = hi != 0
    K[nz] = err[nz] / (R.U[precision] * np.abs(hi[nz]))
    return K


# ---- the kernel's own arithmetic, restated in numpy --------------------------------------------------------------------------------
FAULTS = ("dropped pair", "doubled record", "self term admitted", "mask on the lane's other body", "neighbour masked in place of self",
          "padding record with mass", "last tile of the last split skipped", "velm read at the global index")


class Restatement:
    """The arithmetic csrc/nbx_diag_kernels.hpp documents, in T = the state's precision, for the owned bodies of one set of
    positions: differences, ((eps^2 + dz^2) + dy^2) + dx^2 and 1 / sqrt in T; G m_j * inv in T with j == i an exact 0 and the
    padding records (j >= n, at the origin, G m = 0) included; the 256 terms of a tile added one after the other in T, in
    record order; tile sums and everything after them in fp64.  numpy has no FMA and its 1 / sqrt is not v_rsq: this is a
    second correct evaluation of the same sums, which is what K_ref stands for, not the device's bits.

    fault = (name of FAULTS, k, j) plants one index fault of the kind diag_tile / diag_body could have, at body k (and record j)."""

    def __init__(self, base, precision, i_begin=0, i_count=None):
        T = self.T = dtype_of(precision)
        self.precision, self.n, self.i_begin = precision, len(base["mass"]), i_begin
        self.i_count = self.n - i_begin if i_count is None else i_count
        self.tiles = -(-self.n // TILE)
        npad = self.tiles * TILE
        own = np.arange(i_begin, i_begin + self.i_count)
        p = [np.zeros(npad, dtype=T) for _ in POS]
        for c, f in zip(p, POS):
            c[:self.n] = base[f]
        self.inv = np.empty((self.i_count, npad), dtype=T)

        def fill(c0):
            dx, dy, dz = (c[None, c0:c0 + TILE] - c[own, None] for c in p)
            self.inv[:, c0:c0 + TILE] = T(1) / np.sqrt(((T(EPS2) + dz * dz) + dy * dy) + dx * dx)

        _pmap(fill, range(0, npad, TILE))

    def _gm(self, mass):
        gm = np.zeros(self.tiles * TILE, dtype=self.T)
        gm[:self.n] = gm_as_uploaded(np.asarray(mass, dtype=self.T)).astype(self.T)  # exact: the product was rounded in T
        return gm

    def _tile(self, t, gm, fault=None):
        """The T sums of tile t for every owned body."""
        c0 = t * TILE
        terms = self.inv[:, c0:c0 + TILE] * gm[None, c0:c0 + TILE]
        li = np.arange(max(c0 - self.i_begin, 0), min(c0 + TILE - self.i_begin, self.i_count))
        terms[li, self.i_begin + li - c0] = 0  # j == i
        extra = None
        if fault:
            name, k, j = fault
            lk = k - self.i_begin
            owned = 0 <= lk < self.i_count

            def remask(row, masked):  # `row` masks record `masked` where it should have masked itself
                me = self.i_begin + row
                if c0 <= me < c0 + TILE:
                    terms[row, me - c0] = self.inv[row, me] * gm[me]
                if c0 <= masked < c0 + TILE:
                    terms[row, masked - c0] = 0

            if name == "dropped pair" and owned and c0 <= j < c0 + TILE:
                terms[lk, j - c0] = 0
            elif name == "doubled record" and owned and c0 <= j < c0 + TILE:
                extra = (lk, terms[lk, j - c0])
            elif name == "self term admitted" and owned:
                remask(lk, -1)
            elif name == "mask on the lane's other body" and owned:  # ig[2h] <-> ig[2h + 1]: bodies li and li +- 256 of one lane
                lp = lk + TILE if (lk % COL) < TILE else lk - TILE
                remask(lk, self.i_begin + lp)
                if lp < self.i_count:
                    remask(lp, k)
            elif name == "neighbour masked in place of self" and owned:
                remask(lk, j)
        s = np.add.accumulate(terms, axis=1, dtype=self.T)[:, -1]
        if extra:
            s[extra[0]] = self.T(s[extra[0]] + extra[1])
        return s

    def _finish(self, ts, m_own):
        return -0.5 * float(np.sum(m_own * ts.sum(axis=1)))

    def total(self, mass, fault=None, finish_rows=None):
        """The potential partial of the owned bodies for these masses (T values of all n bodies).  finish_rows: a fault of its
        own -- the reduce adds only the first finish_rows of the splits x cols partial rows (row split * cols + column of
        diag_shape), as a strided loop that stops after its first round would."""
        mass = np.asarray(mass, dtype=self.T)
        gm = self._gm(mass)
        name = fault[0] if fault else None
        assert name is None or name in FAULTS, name
        if name == "padding record with mass":
            assert self.n < self.tiles * TILE
            gm[self.n] = gm_as_uploaded(np.array([1.5 * LIGHT], dtype=self.T))[0]
        ts = np.stack(_pmap(lambda t: self._tile(t, gm, fault), range(self.tiles)), axis=1).astype(np.float64)
        if name == "last tile of the last split skipped":
            ts[:, -1] = 0.0
        if finish_rows is not None:
            cols, _, _, per = diag_shape(self.i_count, self.n)
            row = (np.arange(self.tiles) // per)[None, :] * cols + (np.arange(self.i_count) // COL)[:, None]
            ts = np.where(row < finish_rows, ts, 0.0)
        m_own = mass[self.i_begin:self.i_begin + self.i_count].astype(np.float64)
        if name == "velm read at the global index":  # velm is indexed locally; beyond its end the read finds no mass
            at = self.i_begin + np.arange(self.i_begin, self.i_begin + self.i_count)
            m_own = np.where(at < self.n, mass[np.minimum(at, self.n - 1)], 0).astype(np.float64)
        return self._finish(ts, m_own)

    def heavy_totals(self, ks):
        """total(heavy_state(base, k)["mass"]) for k in ks, the same bits: only the tile that holds record k differs from the
        all-light state, so only that tile's sums are evaluated again."""
        light = light_masses(self.n, self.precision)
        gm = self._gm(light)
        gm1 = gm_as_uploaded(np.ones(1, dtype=self.T)).astype(self.T)[0]
        ts0 = np.stack(_pmap(lambda t: self._tile(t, gm), range(self.tiles)), axis=1).astype(np.float64)
        m0 = light[self.i_begin:self.i_begin + self.i_count].astype(np.float64)

        def one(k):
            k = int(k)
            g = gm.copy()
            g[k] = gm1
            ts = ts0.copy()
            ts[:, k // TILE] = self._tile(k // TILE, g)
            m_own = m0.copy()
            if 0 <= k - self.i_begin < self.i_count:
                m_own[k - self.i_begin] = 1.0
            return self._finish(ts, m_own)

        return np.array(_pmap(one, ks), dtype=np.float64)


def restated(state, precision, i_begin=0, i_count=None, fault=None):
    return Restatement(state, precision, i_begin, i_count).total(state["mass"], fault)


# ---- where to probe ----------------------------------------------------------------------------------------------------------------
def edge_positions(n, i_begin=0, i_count=None, cols_bodies=COL, per_tiles=None):
    """Bodies 0 and n - 1, both sides of every tile edge, of every column edge, of the b = 0 / b = 1 seam inside a column, of
    every j-split edge and of both slice ends (so the neighbours just outside the slice are there)."""
    i_count = n - i_begin if i_count is None else i_count
    per_tiles = diag_shape(i_count, n)[3] if per_tiles is None else per_tiles
    cuts = {n, i_begin, i_begin + i_count}
    cuts.update(range(TILE, n, TILE))
    cuts.update(range(per_tiles * TILE, n, per_tiles * TILE))
    for c0 in range(0, i_count, cols_bodies):
        cuts.update((i_begin + c0, i_begin + c0 + cols_bodies // 2))
    e = {0, n - 1}
    for c in cuts:
        e.update((c - 1, c))
    for c in (i_begin, i_begin + i_count):  # at and next to both slice ends, inside and outside
        e.update((c - 2, c + 1))
    return np.array(sorted(i for i in e if 0 <= i < n), dtype=np.int64)


def sample_positions(n, i_begin=0, i_count=None, cols_bodies=COL, per_tiles=None, count=160, seed=11):
    """edge_positions(), then seeded random bodies of the whole system up to `count`."""
    s = set(edge_positions(n, i_begin, i_count, cols_bodies, per_tiles).tolist())
    rng = np.random.default_rng([seed, n, i_begin])
    while len(s) < min(count, n):
        s.update(int(i) for i in rng.integers(0, n, count - len(s)))
    return np.array(sorted(s), dtype=np.int64)
