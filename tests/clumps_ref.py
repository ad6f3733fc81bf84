"""Clumps under a caller-supplied label (include/nbx_clumps.h): truth, the scales, the K metric and its gate, a numpy restatement
of the kernel's own order with plantable faults, the label families, the states and the planted unbinding case the clump tests
share.  Used by tests/test_clumps_cpu.py and tests/test_clumps_gpu.py; numpy only, no device.

Truth, per body, from the state as stored in T and gm_as_uploaded, evaluated in fp64 for fp32 objects and in np.longdouble for
fp64 objects (plain fp64 where the platform's long double is a double): the header's definition, c(i) found by comparing the
labels as integers.

Scales, per body: phi: sum gm_j / sqrt(r2) over the other members; gm: itself; centre_a: sum gm_j |x_ja| / gm; velocity_a:
W_a = sum gm_j |v_ja| / gm; energy: sum_a (|v_ia| + W_a)^2 / 2 + the scale of phi.  K = |got - truth| / (u scale); where the scale
is 0 the value must be 0 exactly (K = 0, else inf).

Gate, per quantity: force_ref.M * max(K_ref, floor, force_ref.K_TERM).  K_ref is the K of sequential(): the header's arithmetic
restated in T with a correctly rounded 1 / sqrt and ONE sequential sum over j ascending -- never a device value.  floor is the
first-order bound of one term that include/nbx_clumps.h derives: 4.5 u (fp32) and 53.5 u (fp64) for phi and for energy, which
carries phi; nothing for gm, centre and velocity, whose terms are not rounded before they are added.

Restatement: restate() follows the kernel's order -- columns and splits from field_shape(n, n), the records of a split in T, j
ascending, the sentinels (a staged record at or beyond n or with a negative label: -1; an i-side body with a negative label:
-2), the self mask of phi alone, the splits added in fp64 in split order, the quotients and the energy in fp64 rounded once, the
one-body and gm == 0 cases.  numpy has no FMA and its 1 / sqrt is not v_rsq: a second correct evaluation, not the device's bits.
"""
import numpy as np

import field_ref as FR
import fof_ref as FOF
import force_ref as F
import neighbours_ref as NB
from energy_ref import EPS2, G32, gm_as_uploaded

TILE, COL, DTYPE, U = FR.TILE, FR.COL, FR.DTYPE, F.U
POS, VEL = ("pos_x", "pos_y", "pos_z"), ("vel_x", "vel_y", "vel_z")
FIELDS = POS + VEL + ("mass",)
KEYS = ("members", "gm", "centre_x", "centre_y", "centre_z", "velocity_x", "velocity_y", "velocity_z", "phi", "energy")
FLOAT_KEYS = KEYS[1:]
GROUP_KEYS = KEYS[:8]  # what every member of a clump returns the same bits of
CENTRE, VELOCITY = KEYS[2:5], KEYS[5:8]
FLOOR = {"phi": {32: 4.5, 64: 53.5}, "energy": {32: 4.5, 64: 53.5}}  # include/nbx_clumps.h, "Error of one term"
G = float(G32)
CONTEXT_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1025, 2049, 4097)
FAMILIES = ("one", "fof", "stripes", "blocks", "huge")
ENSEMBLE = (3, 2049)
LATTICE_K = 33  # 35 937 bodies: 71 columns x 15 splits
NONE_J, NONE_I = -1, -2
FAULTS = ("the self term kept in phi", "self left out of gm", "padding counted", "labels compared after conversion to float32",
          "negative labels matching each other", "a split dropped", "the lane's second body using the first one's label",
          "the scale not undone", "an unweighted mean velocity", "v in place of v - V", "the one-body case missing")


def gate(k_ref, key, precision):
    return F.M * max(float(k_ref), FLOOR.get(key, {}).get(precision, 0.0), F.K_TERM)


def _wide(precision):
    return np.longdouble if precision == 64 and F.HAVE_LONGDOUBLE else np.float64


# ---- states and labels --------------------------------------------------------------------------------------------------------------
def cloud(n, precision, seed=None):
    """n bodies of G m in [0.5, 1.5] (masses of order 1 / G), uniform in [-1, 1]^3, velocity components uniform in [-4, 4]: of the
    order of the virial speed of a few hundred such bodies, so that members of both signs of energy occur."""
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    m = rng.uniform(0.5, 1.5, n) / G
    pos = rng.uniform(-1.0, 1.0, (3, n))
    vel = 4.0 * rng.uniform(-1.0, 1.0, (3, n))
    return {k: np.ascontiguousarray(v.astype(DTYPE[precision])) for k, v in zip(FIELDS, list(pos) + list(vel) + [m])}


def lattice(precision):
    """LATTICE_K^3 bodies on a cubic lattice of spacing 1/8, G m = 1, velocities a smooth function of the index."""
    k = LATTICE_K
    i = np.arange(k ** 3)
    pos = [(i // k ** 2) / 8.0, ((i // k) % k) / 8.0, (i % k) / 8.0]
    vel = [np.sin(0.37 * i), np.cos(0.11 * i), np.sin(0.05 * i + 1.0)]
    return {f: np.ascontiguousarray(np.asarray(v).astype(DTYPE[precision])) for f, v in zip(FIELDS, pos + vel + [np.full(k ** 3, 1.0 / G)])}


def labels(family, state, precision):
    """The int32 labels of one family for a state."""
    n = len(state["mass"])
    i = np.arange(n, dtype=np.int64)
    if family == "one":
        lab = np.zeros(n, dtype=np.int64)
    elif family == "fof":  # a radius at which a body has one friend on average: singletons and groups
        lab = FOF.fof(state, FOF.target_radius(n, 1.0), precision)["label"].astype(np.int64)
    elif family == "stripes":  # every clump crosses every tile, column and split; every 11th body is in no clump
        lab = np.where(i % 11 == 10, -1, i % 7)
    elif family == "blocks":  # seams that never fall on a tile
        lab = i // 300
    elif family == "huge":
        lab = 2 ** 31 - 1 - (i % 5)
    else:
        raise ValueError(family)
    return lab.astype(np.int32)


def renamed(label):
    """A bijective renaming of the labels >= 0 (negative ones stay): other values, other order, still int32."""
    label = np.asarray(label, dtype=np.int64)
    names = np.unique(label[label >= 0])
    new = 2 ** 31 - 1 - 3 * np.arange(len(names), dtype=np.int64)  # ascending names to descending values
    out = label.copy()
    ok = label >= 0
    out[ok] = new[np.searchsorted(names, label[ok])]
    return out.astype(np.int32)


def _arrays(state, dtype):
    x = np.stack([np.asarray(state[f]).astype(dtype) for f in POS])
    v = np.stack([np.asarray(state[f]).astype(dtype) for f in VEL])
    return x, v, gm_as_uploaded(state["mass"]).astype(dtype)


# ---- truth, metric ------------------------------------------------------------------------------------------------------------------
def truth(state, label, precision, rows=None):
    """{"members": (n,) int64, "rows": the bodies phi and energy are given for (default: all), key: (value, scale)}: the group
    keys for all n bodies, phi and energy for `rows`; values in the wide type, scales fp64."""
    W = _wide(precision)
    x, v, g = _arrays(state, W)
    n = len(g)
    label = np.asarray(label, dtype=np.int64)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    ok = label >= 0
    at = np.nonzero(ok)[0]
    names, inv = np.unique(label[at], return_inverse=True)
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(len(names)))

    def gsum(values):  # per clump, spread back to the bodies (0 for bodies in no clump)
        out = np.zeros(n, dtype=W)
        if len(at):
            out[at] = np.add.reduceat(values[at][order], starts)[inv]
        return out

    members = gsum(np.ones(n, dtype=W)).astype(np.int64)
    gm = gsum(g)
    single = members == 1
    out = {"members": members, "rows": rows, "gm": (gm, gm.astype(np.float64))}
    have = gm != 0
    safe = np.where(have, gm, W(1))
    cen, vel, wscale = [], [], []
    for a in range(3):
        for src, keys, keep in ((x, CENTRE, cen), (v, VELOCITY, vel)):
            val = np.where(have, gsum(g * src[a]) / safe, W(0))
            val = np.where(single, src[a], val)  # the body alone: its own value, exactly
            val = np.where(ok, val, W(0))
            scale = np.where(have, gsum(g * np.abs(src[a])) / safe, W(0))
            scale = np.where(single, np.abs(src[a]), scale)
            scale = np.where(ok, scale, W(0))
            keep.append(val)
            out[keys[a]] = (val, scale.astype(np.float64))
            if src is v:
                wscale.append(scale)
    phi, pscale = np.zeros(len(rows), dtype=W), np.zeros(len(rows), dtype=W)
    for a, b in F._row_chunks(len(rows), n):
        r = rows[a:b]
        d = [x[c][None, :] - x[c][r, None] for c in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + W(EPS2)
        same = (label[None, :] == label[r, None]) & ok[r, None]
        same[np.arange(b - a), r] = False
        t = np.where(same, g[None, :] / np.sqrt(r2), W(0)).sum(axis=1)
        phi[a:b], pscale[a:b] = -t, t
    kin = sum((v[c][rows] - vel[c][rows]) ** 2 for c in range(3)) / 2
    kscale = sum((np.abs(v[c][rows]) + wscale[c][rows]) ** 2 for c in range(3)) / 2
    many = members[rows] > 1
    out["phi"] = (phi, pscale.astype(np.float64))
    out["energy"] = (np.where(many, kin + phi, W(0)), np.where(many, kscale + pscale, W(0)).astype(np.float64))
    return out


def k_metric(got, tr, precision):
    """{key: K per body (phi and energy: per body of tr["rows"])}."""
    out = {}
    for key in FLOAT_KEYS:
        val, scale = tr[key]
        g = np.asarray(got[key])
        if key in ("phi", "energy") and len(g) != len(val):
            g = g[tr["rows"]]
        err = np.abs(g.astype(val.dtype) - val).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[key] = np.where(scale > 0, err / (U[precision] * scale), np.where(g == 0, 0.0, np.inf))
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def restate(state, label, precision, fault=None, one_split=False, rows=None):
    """The ten KEYS in T (members int32) in the kernel's own order (see the module docstring); rows: phi and energy of these
    bodies only.  fault: one of FAULTS, planted.  one_split: one sequential sum over all j (sequential())."""
    assert fault is None or fault in FAULTS, fault
    T = DTYPE[precision]
    x, v, g = _arrays(state, T)
    n = len(g)
    label = np.asarray(label, dtype=np.int64)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    _, tiles, splits, per = FR.field_shape(n, n)
    if one_split:
        splits, per = 1, tiles
    npad = tiles * TILE
    key = (lambda l: l.astype(np.float32)) if fault == "labels compared after conversion to float32" else (lambda l: l)
    negative = fault == "negative labels matching each other"
    labi = label.copy() if negative else np.where(label >= 0, label, NONE_I)
    if fault == "the lane's second body using the first one's label":  # bodies l and l + 256 of one column sit in one lane
        i = np.arange(n)
        labi = np.where(i % COL >= TILE, labi[np.maximum(i - TILE, 0)], labi)
    labj = np.full(npad, NONE_J, dtype=np.int64)
    labj[:n] = label if negative else np.where(label >= 0, label, NONE_J)
    rx, rv, rg = np.zeros((3, npad), dtype=T), np.zeros((3, npad), dtype=T), np.zeros(npad, dtype=T)
    rx[:, :n], rv[:, :n], rg[:n] = x, v, g
    if fault == "padding counted":
        assert n < npad
        labj[n:], rg[n:] = labi[0], g.max()
    labi, labj = key(labi), key(labj)
    bounds = [(s * per * TILE, min(tiles, (s + 1) * per) * TILE) for s in range(splits)]
    # the clump sums, once per distinct i-side label: every member sees the same sequence of g
    names, which = np.unique(labi, return_inverse=True)
    parts = np.zeros((splits, len(names), 7), dtype=T)
    count = np.zeros((splits, len(names)), dtype=np.int64)
    for lo in range(0, len(names), 256):
        hit = labj[None, :] == names[lo:lo + 256, None]
        gsel = np.where(hit, rg[None, :], T(0))
        for s, (j0, j1) in enumerate(bounds):
            terms = [gsel[:, j0:j1]] + [gsel[:, j0:j1] * rv[c][None, j0:j1] for c in range(3)] + [gsel[:, j0:j1] * rx[c][None, j0:j1] for c in range(3)]
            for c, t in enumerate(terms):
                parts[s, lo:lo + 256, c] = np.add.accumulate(t, axis=1, dtype=T)[:, -1]
            count[s, lo:lo + 256] = hit[:, j0:j1].sum(axis=1)
    sparts = np.zeros((splits, len(rows)), dtype=T)
    step = max(1, (1 << 21) // npad)
    for a in range(0, len(rows), step):
        r = rows[a:a + step]
        for s, (j0, j1) in enumerate(bounds):
            d = [rx[c][None, j0:j1] - x[c][r, None] for c in range(3)]
            inv = FR._inv_sqrt(((T(EPS2) + d[2] * d[2]) + d[1] * d[1]) + d[0] * d[0], T)
            gs = np.where(labj[None, j0:j1] == labi[r, None], rg[None, j0:j1], T(0))
            if fault != "the self term kept in phi":
                own = (r >= j0) & (r < j1)
                gs[np.nonzero(own)[0], r[own] - j0] = 0
            sparts[s, a:a + step] = np.add.accumulate(gs * inv, axis=1, dtype=T)[:, -1]
    used = range(splits - 1) if fault == "a split dropped" and splits > 1 else range(splits)
    tot = sum(parts[s].astype(np.float64) for s in used)[which]          # (n, 7)
    members = sum(count[s] for s in used)[which]
    ssum = sum(sparts[s].astype(np.float64) for s in used)
    m = tot[:, 0].copy()
    if fault == "self left out of gm":
        m = m - g.astype(np.float64)
    live = (label >= 0) | negative
    have = (m != 0) & live
    safe = np.where(have, m, 1.0)
    vel64 = np.where(have[:, None], tot[:, 1:4] / safe[:, None], 0.0)
    cen64 = np.where(have[:, None], tot[:, 4:7] / safe[:, None], 0.0)
    if fault == "an unweighted mean velocity":
        for c in range(3):
            sums = np.zeros(n)
            for l in np.unique(label[label >= 0]):
                sums[label == l] = v[c][label == l].astype(np.float64).mean()
            vel64[:, c] = sums
    single = (members == 1) & live
    if fault == "the one-body case missing":
        single = np.zeros(n, dtype=bool)
    phi64 = -ssum
    w = v.astype(np.float64)[:, rows].T - (0.0 if fault == "v in place of v - V" else vel64[rows])
    e64 = 0.5 * (w * w).sum(axis=1) + phi64
    gm64 = m.copy()
    if fault == "the scale not undone":
        phi64, gm64 = phi64 * 0.25, gm64 * 0.125
    out = {"members": np.where(live, members, 0).astype(np.int32), "gm": np.where(live, gm64, 0.0).astype(T)}
    for c in range(3):
        out[CENTRE[c]] = np.where(single, x[c], np.where(live, cen64[:, c], 0.0).astype(T))
        out[VELOCITY[c]] = np.where(single, v[c], np.where(live, vel64[:, c], 0.0).astype(T))
    quiet = single[rows] | ~live[rows]
    out["phi"] = np.where(quiet, 0.0, phi64).astype(T)
    out["energy"] = np.where(quiet, 0.0, e64).astype(T)
    return out


def sequential(state, label, precision, rows=None):
    return restate(state, label, precision, one_split=True, rows=rows)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def same_bits_problems(got, label):
    """Where the members of one clump differ in a bit of members, gm, centre or velocity."""
    label = np.asarray(label, dtype=np.int64)
    at = np.nonzero(label >= 0)[0]
    if not len(at):
        return []
    _, first, inv = np.unique(label[at], return_index=True, return_inverse=True)
    lead = at[first][inv]
    bad = []
    for k in GROUP_KEYS:
        a = np.ascontiguousarray(got[k])
        bits = a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)
        if (bits[at] != bits[lead]).any():
            bad.append("%s differs within a clump" % k)
    return bad


def compare(got, tr, gates, state, label, precision):
    """(problems, {key: the largest K}): what the device tests hold a result to."""
    label = np.asarray(label, dtype=np.int64)
    problems = []
    if not np.array_equal(np.asarray(got["members"], dtype=np.int64), tr["members"]):
        problems.append("members differ at %d bodies" % int((np.asarray(got["members"]) != tr["members"]).sum()))
    ks = {k: float(v.max()) if len(v) else 0.0 for k, v in k_metric(got, tr, precision).items()}
    for k in FLOAT_KEYS:
        if not ks[k] <= gates[k]:
            problems.append("%s: K = %.1f above the gate %.1f" % (k, ks[k], gates[k]))
    problems += same_bits_problems(got, label)
    rows = tr["rows"]
    single, out = tr["members"] == 1, label < 0
    for c in range(3):
        if not (np.array_equal(got[CENTRE[c]][single], state[POS[c]][single]) and np.array_equal(got[VELOCITY[c]][single], state[VEL[c]][single])):
            problems.append("a clump of one body is not at the body itself, axis %d" % c)
    full = len(got["phi"]) != len(rows)
    for k in ("phi", "energy"):
        val = np.asarray(got[k])[rows] if full else np.asarray(got[k])
        if (val[single[rows] | out[rows]] != 0).any():
            problems.append("%s is not 0 for a body alone or in no clump" % k)
    for k in FLOAT_KEYS[:7]:
        if (np.asarray(got[k])[out] != 0).any():
            problems.append("%s is not 0 for a body in no clump" % k)
    return problems, ks


# ---- one case, everything computed once ---------------------------------------------------------------------------------------------
_cases = {}


def case(precision, n, family, state=None, rows=None, name=None):
    """{"state", "label", "truth", "kref", "gates"} of one (precision, n, family), cached.  state: another state than cloud(n)."""
    key = (precision, n, family, name)
    if key not in _cases:
        st = cloud(n, precision) if state is None else state
        lab = labels(family, st, precision)
        tr = truth(st, lab, precision, rows=rows)
        kref = {k: float(v.max()) if len(v) else 0.0 for k, v in k_metric(sequential(st, lab, precision, rows=rows), tr, precision).items()}
        _cases[key] = {"state": st, "label": lab, "truth": tr, "kref": kref, "gates": {k: gate(kref[k], k, precision) for k in FLOAT_KEYS}}
    return _cases[key]


def context_cases():
    """(n, family) of the device tests' contexts: every size under every label family."""
    return [(n, fam) for n in CONTEXT_SIZES for fam in FAMILIES]


def lattice_rows():
    """About 1000 bodies of the lattice: both sides of every column seam and of every split seam, and an even sample."""
    n = LATTICE_K ** 3
    columns, tiles, splits, per = FR.field_shape(n, n)
    seams = [c * COL for c in range(1, columns)] + [s * per * TILE for s in range(1, splits)]
    rows = {0, n - 1}
    for s in seams:
        rows.update((s - 1, s))
    rows.update(range(7, n, n // 800))
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


# ---- unbinding ----------------------------------------------------------------------------------------------------------------------
UNBIND_N = 66  # 64 clump bodies, the interloper, its companion


def unbind_state(precision, seed=5):
    """A virialised clump of 64 bodies of G m = 1 in the unit ball, a fast interloper of G m = 8 at its edge, and a companion 0.04
    from the interloper whose speed the clump alone cannot hold: bound only while the interloper counts."""
    rng = np.random.default_rng(seed)
    k = 64
    p = rng.normal(size=(3, k))
    p = p / np.linalg.norm(p, axis=0) * rng.uniform(0, 1, k) ** (1 / 3)
    w = rng.normal(size=(3, k))
    w -= w.mean(axis=1, keepdims=True)
    d = p[:, :, None] - p[:, None, :]
    r = np.sqrt((d * d).sum(axis=0) + EPS2)
    np.fill_diagonal(r, np.inf)
    pot = 0.5 * (1.0 / r).sum()
    w *= np.sqrt(pot / (w * w).sum())  # 2 K = |W| with unit G m
    pos = np.concatenate([p, [[1.2, 1.2], [0.0, 0.04], [0.0, 0.0]]], axis=1)
    vel = np.concatenate([w, [[0.0, 0.0], [20.0, 0.0], [0.0, 14.0]]], axis=1)
    gm = np.concatenate([np.ones(k), [8.0, 1.0]])
    return {f: np.ascontiguousarray(a.astype(DTYPE[precision])) for f, a in zip(FIELDS, list(pos) + list(vel) + [gm / G])}


def unbind(state, label, precision, max_iter=32):
    """(final labels, iterations, margin): nbx.unbind from truth.  margin: the smallest, over the iterations and the bodies in
    clumps of several, of |energy| / (u scale) divided by the iteration's energy gate -- above 1, no reference energy lies within
    the gate's window of 0 and a device within its gate takes the same decisions."""
    label = np.array(label, dtype=np.int32)
    margin, iterations = np.inf, 0
    while iterations < max_iter:
        tr = truth(state, label, precision)
        iterations += 1
        e, scale = tr["energy"]
        many = tr["members"] > 1
        if many.any():
            kref = float(k_metric(sequential(state, label, precision), tr, precision)["energy"].max())
            k0 = float((np.abs(e[many]).astype(np.float64) / (U[precision] * scale[many])).min())
            margin = min(margin, k0 / gate(kref, "energy", precision))
        leave = (label >= 0) & (e >= 0)
        if not leave.any():
            break
        label[leave] = -1
    return label, iterations, margin


def catalogue(label, result, mass, min_members=2):
    """nbx.clump_catalogue as a plain loop: rows (label, members, gm, centre, velocity, kinetic, potential, virial, bound)."""
    label = np.asarray(label, dtype=np.int64)
    rows = []
    for l in sorted(set(label[label >= 0].tolist())):
        idx = np.nonzero(label == l)[0]
        if len(idx) < min_members:
            continue
        i0 = idx[0]
        kin = sum(float(mass[i]) * (float(result["energy"][i]) - float(result["phi"][i])) for i in idx)
        pot = 0.5 * sum(float(mass[i]) * float(result["phi"][i]) for i in idx)
        rows.append((l, len(idx), float(result["gm"][i0]), [float(result[k][i0]) for k in CENTRE], [float(result[k][i0]) for k in VELOCITY],
                     kin, pot, 2 * kin / abs(pot) if pot != 0 else float("inf"), sum(1 for i in idx if result["energy"][i] < 0)))
    return sorted(rows, key=lambda r: (-r[1], r[0]))
