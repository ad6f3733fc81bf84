"""numpy reference, in fp64, of include/nbx_fof.h: the friends-of-friends groups of a state as stored, widened -- per body the
lowest index of its group and the group's size, per system the number of groups and the largest.

fof() is the plain definition: a union-find over the pairs with r2 <= h2.  restate() runs the library's pass scheme step for step
-- labels L[i] = i; per pass the minimum over a body's friends per j split of field_shape(n, n) (the self pair and the padding
records at the origin included, as the kernels meet them), the finish over the split rows, the hook N[L[i]] = min(N[L[i]], m[i]),
the shortcut N[i] = N[N[i]] to its fixed point, the test N != L -- and returns the labels AND the number of passes, which the
library reports and the device tests compare.  The faults a kernel chain of this structure can have may be planted (FAULTS);
without a fault the scheme does not show in the labels, which test_fof_cpu.py checks against fof().

The device decides r2 <= h2 in T, the reference in fp64: a (state, radius) may be held to EXACT equality where no pair has an r2
within AMBIGUITY u of h2 (u the unit round-off of T; r2 carries up to 5 u), which ambiguous() says.  pick_radius() chooses a
radius near a target whose h2 lies in the middle of the widest gap between the pairs' r2 values, so that every radius of the
device tests can be shown unambiguous (test_fof_cpu.py shows it for every one of them).
"""
import numpy as np

import neighbours_ref as N
from energy_ref import EPS2
from field_ref import field_shape

KEYS = ("label", "size", "groups", "largest")
POS = N.POS
DTYPE = N.DTYPE
U = N.U
TILE = N.TILE
NONE = 0x7fffffff  # the label of a padding record
AMBIGUITY = 64.0   # in u
SIZES = (1, 2, 257, 513, 1025, 2049, 4097)
RAGGED_SIZES = (5, 8192, 257, 1, 2049)
DEGREES = (0.15, 1.2, 4.5)  # the expected number of friends per body of a uniform cloud: mostly singletons, many groups, one giant group plus debris
CHAIN_N = 4097
CHAIN_SPACING = 1.0 / 64
CHAIN_RADIUS = 0.02       # between the spacing and twice the spacing
CHAIN_ORDERS = ("random", "ascending", "descending", "zigzag")
LATTICE_BELOW, LATTICE_ABOVE = 0.124, 0.126  # the spacing is 1/8
LATTICE_TIE = N.LATTICE_TIE_RADIUS           # h2 is bit for bit the face neighbours' r2, in both precisions
FAULTS = ("no hook", "no shortcut", "padding label 0", "< instead of <=", "a split row dropped in the finish",
          "label is any member, not the lowest", "size without the body itself", "labels offset by the member's place in the range")

lattice, lattice_order, h2_of = N.lattice, N.lattice_order, N.h2_of


# ---- states ------------------------------------------------------------------------------------------------------------------------
def cloud(n, precision):
    """The uniform cloud of n bodies the other analysis tests use: neighbours_ref.member (box(n) where it exists)."""
    return N.member(n, precision)


def clustered(n, precision, seed=None):
    """n bodies in [-1, 1]^3: a third uniform, the others in clumps of 32 (Gaussian, sigma 0.03) about uniform centres."""
    rng = np.random.default_rng(700 + n if seed is None else seed)
    s = N.K.make_state(300 + n, n, np.float64)
    back = n - 2 * (n // 3)
    centres = rng.uniform(-0.8, 0.8, (max((n - back + 31) // 32, 1), 3))
    pos = np.concatenate([rng.uniform(-1.0, 1.0, (back, 3)), centres[np.arange(n - back) // 32] + 0.03 * rng.standard_normal((n - back, 3))])
    pos = pos[rng.permutation(n)]
    for c, name in enumerate(POS):
        s[name] = pos[:, c]
    return {k: np.ascontiguousarray(v.astype(DTYPE[precision])) for k, v in s.items()}


def chain_order(n, order):
    """site[body]: the place on the line of body `body`."""
    if order == "ascending":
        return np.arange(n)
    if order == "descending":
        return np.arange(n)[::-1].copy()
    if order == "zigzag":  # 0, n - 1, 1, n - 2, ...
        z = np.empty(n, dtype=np.int64)
        z[0::2] = np.arange((n + 1) // 2)
        z[1::2] = n - 1 - np.arange(n // 2)
        return z
    assert order == "random", order
    return np.random.default_rng(9).permutation(n)


def chain(n, precision, order, cut=None):
    """n bodies on the x axis at spacing 1/64 about the origin (every coordinate exact in fp32), body b at site chain_order[b].
    cut: the link between sites cut - 1 and cut is removed -- the sites from `cut` on are moved one more spacing out."""
    s = N.K.make_state(500 + n, n, np.float64)
    site = chain_order(n, order)
    for name in POS:
        s[name] = np.zeros(n)
    s["pos_x"] = (site - (n - 1) // 2 + (0 if cut is None else (site >= cut))) * CHAIN_SPACING
    return {k: np.ascontiguousarray(v.astype(DTYPE[precision])) for k, v in s.items()}


def lattice_pairs(k, perm=False):
    """The face-neighbour pairs (i, j), i < j, of lattice(k, perm) from the geometry alone."""
    n = k ** 3
    site = lattice_order(k, perm)
    body_of = np.empty(n, dtype=np.int64)
    body_of[site] = np.arange(n)
    c = np.stack([site // (k * k), (site // k) % k, site % k], axis=1)
    out = []
    for axis, step in ((0, k * k), (1, k), (2, 1)):
        ok = c[:, axis] < k - 1
        a, b = np.nonzero(ok)[0], body_of[site[ok] + step]
        out.append(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1))
    return np.concatenate(out)


# ---- the pairs ---------------------------------------------------------------------------------------------------------------------
def _xyz(state):
    return [np.asarray(state[c], dtype=np.float64) for c in POS]


def close_pairs(state, r2_max, chunk=512):
    """(pairs (m, 2) with i < j, their r2 (m,)) of every pair with r2 <= r2_max, fp64 from the state as stored, in row chunks."""
    x = _xyz(state)
    n = len(x[0])
    ii, jj, rr = [], [], []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = [x[c][None, lo:] - x[c][lo:hi, None] for c in range(3)]
        m = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
        a, b = np.nonzero(m <= r2_max)
        keep = b > a  # j = lo + b > i = lo + a
        ii.append(lo + a[keep]); jj.append(lo + b[keep]); rr.append(m[a[keep], b[keep]])
    if not ii:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    return np.stack([np.concatenate(ii), np.concatenate(jj)], axis=1).astype(np.int64), np.concatenate(rr)


def _origin_r2(state):
    x = _xyz(state)
    return x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + EPS2


def target_radius(n, degree):
    """The radius at which a body of n uniform in [-1, 1]^3 has `degree` friends on average."""
    return float((degree * 8.0 * 3.0 / (4.0 * np.pi * max(n, 2))) ** (1.0 / 3))


def pick_radius(state, target, close=None):
    """The radius whose h2 lies in the middle of the widest gap between consecutive distinct pair r2 values -- the window's ends
    and the bodies' r2 to the origin, where the padding records sit, count as values -- with radius^2 within [0.8, 1.25] x
    target^2.  state: one state, or a list of states that one call serves with one radius (the values of all of them count).
    close: close_pairs(state, at least 1.25 target^2 + EPS2), if at hand (one state)."""
    lo, hi = 0.8 * target * target + EPS2, 1.25 * target * target + EPS2
    states = state if isinstance(state, (list, tuple)) else [state]
    v = np.concatenate([a for s in states for a in ((close_pairs(s, hi)[1] if close is None else close[1]), _origin_r2(s))])
    v = np.unique(np.concatenate([[lo, hi], v[(v > lo) & (v < hi)]]))
    k = int(np.argmax(np.diff(v)))
    return float(np.sqrt(0.5 * (v[k] + v[k + 1]) - EPS2))


def ambiguous(state, radius, precision=32, close=None):
    """Whether any pair -- or any body and a padding record at the origin -- has an r2 within AMBIGUITY u of h2."""
    h2 = h2_of(radius, precision)
    band = AMBIGUITY * U[precision] * h2
    r2 = close_pairs(state, h2 + band)[1] if close is None else close[1]
    return bool((np.abs(r2 - h2) <= band).any() or (np.abs(_origin_r2(state) - h2) <= band).any())


def median_neighbour_distance(states, chunk=1024):
    """The median over the bodies of all `states` of the unsoftened distance to the nearest neighbour."""
    out = []
    for s in states:
        x = [np.asarray(s[c], dtype=np.float32) for c in POS]  # a target for pick_radius: fp32 will do
        n = len(x[0])
        for lo in range(0, n if n > 1 else 0, chunk):
            hi = min(n, lo + chunk)
            d = x[0][None, :] - x[0][lo:hi, None]
            m = d * d
            for c in (1, 2):
                d = x[c][None, :] - x[c][lo:hi, None]
                m += d * d
            m[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
            out.append(np.sqrt(m.min(axis=1)))
    return float(np.median(np.concatenate(out)))


def lattice_ambiguous(k, radius, precision):
    """ambiguous() of lattice(k) from the geometry: every r2, the padding records' included, is d / 64 + EPS2 for an integer d."""
    h2 = h2_of(radius, precision)
    v = np.arange(3 * (k - 1) ** 2 + 1) / 64.0 + EPS2
    return bool((np.abs(v - h2) <= AMBIGUITY * U[precision] * h2).any())


def friend_pairs(state, radius, precision, close=None, strict=False):
    """The (i, j), i < j, that are friends."""
    h2 = h2_of(radius, precision)
    pairs, r2 = close_pairs(state, h2) if close is None else close
    return pairs[(r2 < h2) if strict else (r2 <= h2)]


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def summary(label):
    """{"label", "size", "groups", "largest"} of lowest-index labels."""
    label = np.asarray(label, dtype=np.int64)
    counts = np.bincount(label, minlength=len(label))
    return {"label": label.astype(np.int32), "size": counts[label].astype(np.int32), "groups": int((label == np.arange(len(label))).sum()),
            "largest": int(counts.max())}


def fof(state, radius, precision, pairs=None, close=None):
    """The plain definition: union-find (the lower root wins, paths halved) over the friend pairs, then every body's root.
    pairs: the friend pairs, if at hand (a closed form)."""
    n = len(state[POS[0]])
    if pairs is None:
        pairs = friend_pairs(state, radius, precision, close)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in pairs.tolist():
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return summary([find(i) for i in range(n)])


# ---- the library's scheme ----------------------------------------------------------------------------------------------------------
def restate(state, radius, precision, fault=None, pairs=None, close=None, offset=0):
    """{"label", "size", "groups", "largest", "passes"} by the pass scheme of the module's docstring.  `fault`: one of FAULTS,
    planted.  pairs: the friend pairs, if at hand.  offset: the bodies of the range before this member (it shows only under
    the fault that forgets to take it off)."""
    assert fault is None or fault in FAULTS, fault
    n = len(state[POS[0]])
    h2 = h2_of(radius, precision)
    if pairs is None:
        pairs = friend_pairs(state, radius, precision, close, strict=fault == "< instead of <=")
    _, tiles, splits, per = field_shape(n, n)
    # directed (i, j): both directions of every pair, the self pair, and -- one stands for all, they are equal -- the padding
    # record at index n where the buffer has one and the body is within h2 of the origin
    o2 = _origin_r2(state)
    near = np.nonzero((o2 < h2) if fault == "< instead of <=" else (o2 <= h2))[0] if tiles * TILE > n else np.zeros(0, dtype=np.int64)
    own = np.arange(n) if fault != "< instead of <=" or EPS2 < h2 else np.zeros(0, dtype=np.int64)
    ei = np.concatenate([pairs[:, 0], pairs[:, 1], own, near]).astype(np.int64)
    ej = np.concatenate([pairs[:, 1], pairs[:, 0], own, np.full(len(near), n)]).astype(np.int64)
    row = ej // (per * TILE)  # the split that meets record j
    rows_used = splits - 1 if fault == "a split row dropped in the finish" and splits > 1 else splits
    L = np.arange(n, dtype=np.int64)
    passes = 0
    while True:
        passes += 1
        assert passes <= n + 1, "the guard of the library"
        lab = np.concatenate([L, [0 if fault == "padding label 0" else NONE]])
        parts = np.full((splits, n), NONE, dtype=np.int64)
        np.minimum.at(parts, (row, ei), lab[ej])
        m = parts[:rows_used].min(axis=0)
        nxt = L.copy()
        np.minimum.at(nxt, np.arange(n), m)
        if fault != "no hook":
            np.minimum.at(nxt, L, m)
        while fault != "no shortcut":
            up = nxt[nxt]
            if np.array_equal(up, nxt):
                break
            nxt = up
        changed = not np.array_equal(nxt, L)
        L = nxt
        if not changed:
            break
    out = summary(L)
    if fault == "label is any member, not the lowest":
        high = np.zeros(n, dtype=np.int64)
        np.maximum.at(high, L, np.arange(n))
        out["label"] = high[L].astype(np.int32)
    if fault == "size without the body itself":
        out["size"] = out["size"] - 1
        out["largest"] -= 1
    if fault == "labels offset by the member's place in the range":
        out["label"] = out["label"] + np.int32(offset)
    out["passes"] = passes
    return out


def differs(got, want, passes=True):
    """What the device tests see between a result and the reference's: a list of findings, empty when label, size, groups and
    largest are equal -- and, with passes, the number of passes."""
    out = []
    for key in ("label", "size"):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if a.shape != b.shape:
            out.append("%s: shape %r against %r" % (key, a.shape, b.shape))
        elif not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            out.append("%s: %d bodies differ, first %r" % (key, len(bad), bad[:4].tolist()))
    for key in ("groups", "largest") + (("passes",) if passes else ()):
        if int(got[key]) != int(want[key]):
            out.append("%s: %d against %d" % (key, int(got[key]), int(want[key])))
    return out


def catalogue(label, mass, x, y, z, min_members=2):
    """nbx.fof_catalogue as a plain loop: [(label, members, mass, (cx, cy, cz))] ordered by (-members, label)."""
    groups = {}
    for i, l in enumerate(np.asarray(label).tolist()):
        g = groups.setdefault(l, [0, 0.0, 0.0, 0.0, 0.0])
        m = float(mass[i])
        g[0] += 1
        g[1] += m
        for a, v in enumerate((x, y, z)):
            g[2 + a] += m * float(v[i])
    rows = [(l, g[0], g[1], (g[2] / g[1], g[3] / g[1], g[4] / g[1])) for l, g in groups.items() if g[0] >= min_members]
    return sorted(rows, key=lambda r: (-r[1], r[0]))


# ---- the cases of the device tests -------------------------------------------------------------------------------------------------
FAMILIES = {"cloud": cloud, "clustered": clustered}
ENSEMBLE_N, ENSEMBLE_MEMBERS = 2049, 6
_cache = {}


def sized(precision, family, n):
    """(state, close pairs up to the largest radius, the three radii of DEGREES) of a family at size n, made once."""
    key = (precision, family, n)
    if key not in _cache:
        st = FAMILIES[family](n, precision)
        close = close_pairs(st, 1.25 * target_radius(n, DEGREES[-1]) ** 2 + EPS2 + 1e-9)
        _cache[key] = (st, close, tuple(pick_radius(st, target_radius(n, d), close) for d in DEGREES))
    return _cache[key]


def ensemble_states(precision):
    """The members of the device tests' ensemble, and the one radius they are asked with (many groups in the clouds)."""
    key = (precision, "ensemble")
    if key not in _cache:
        n = ENSEMBLE_N
        sts = [cloud(n, precision), clustered(n, precision), chain(n, precision, "random"), N.reversed_box(n, precision)]
        sts += [N.K.make_state(600 + m, n, DTYPE[precision]) for m in range(len(sts), ENSEMBLE_MEMBERS)]
        _cache[key] = (sts, pick_radius(sts, target_radius(n, DEGREES[1])))
    return _cache[key]


def ragged_states(precision):
    """The members of the device tests' ragged ensemble (RAGGED_SIZES: 5 and 8192 bodies side by side), and their one radius."""
    key = (precision, "ragged")
    if key not in _cache:
        sts = [N.K.make_state(800 + n, n, DTYPE[precision]) if n == 8192 else cloud(n, precision) for n in RAGGED_SIZES]
        _cache[key] = (sts, pick_radius(sts, target_radius(2049, DEGREES[1])))
    return _cache[key]


def reference_cases(precision):
    """Every (name, state, radius, close pairs or None) the device tests compare with fof() and restate() computed from the
    state: each must be unambiguous."""
    out = []
    for family in FAMILIES:
        for n in SIZES:
            st, close, radii = sized(precision, family, n)
            out += [("%s(%d) r%d" % (family, n, q), st, r, close) for q, r in enumerate(radii)]
    for order in CHAIN_ORDERS:
        out.append(("chain %s" % order, chain(CHAIN_N, precision, order), CHAIN_RADIUS, None))
        out.append(("chain %s cut" % order, chain(CHAIN_N, precision, order, cut=CHAIN_N // 3), CHAIN_RADIUS, None))
    for perm in (False, True):
        for r in (LATTICE_BELOW, LATTICE_ABOVE):
            out.append(("lattice(13) perm=%d r=%g" % (perm, r), lattice(N.LATTICE_K, precision, perm), r, None))
    for name, (sts, r) in (("ensemble", ensemble_states(precision)), ("ragged", ragged_states(precision))):
        out += [("%s member %d" % (name, m), st, r, None) for m, st in enumerate(sts)]
    return out
