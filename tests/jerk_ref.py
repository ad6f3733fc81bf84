"""The acceleration of every body and its time derivative (include/nbx_jerk.h): truth, the K metrics and their gates, a numpy
restatement of the kernel's own order with plantable faults, the states the jerk tests share and a numpy Hermite P(EC)
integrator.  Used by tests/test_jerk_cpu.py and tests/test_jerk_gpu.py; numpy only, no device.

Truth per component, from the definition: fp64 for fp32 objects, np.longdouble for fp64 objects (fp64 where long double is no
wider), with G m as uploaded, summed pairwise by numpy: far below u_T in that type.
    a_i    = sum_j gm_j d / r2^(3/2)
    adot_i = sum_j gm_j [ u / r2^(3/2) - 3 (d.u) d / r2^(5/2) ],  d = x_j - x_i, u = v_j - v_i, r2 = |d|^2 + eps^2
Scales: the acceleration's is the field reference's, A_i = max_c sum_j |d_c| gm_j r2^(-3/2); the jerk's is per component,
    B_c = sum_j gm_j r2^(-3/2) (|u_c| + 3 (|dx ux| + |dy uy| + |dz uz|) |d_c| / r2).
K = |value - truth| / (u_T scale); where the scale is 0 the value must be an exact zero (K = 0 if so, inf if not).  The gate is
the project's own with the header's first-order bound of one term as a floor: K <= 2 max(K_ref, floor, 16), K_ref the
restatement's K on the same state -- never a device value.

Restatement: the kernel's own order -- columns, splits and tiles per split from field_shape(n, n), the six sums in T over a
split, j ascending, the splits added in fp64 in split order and rounded once to T; fp32 with a correctly rounded 1 / sqrt and
every fma evaluated in fp64 and rounded once; fp64 with a seed of 24 bits, its residual and the header's two polynomials, the
fma as a multiply and an add.  A second correct evaluation of the same sums, not the device's bits.
"""
import numpy as np

import field_ref as FR
import force_ref as F
import kick_ref as KR
import neighbours_ref as NB
import potential_ref as P
from energy_ref import EPS2, G32, gm_as_uploaded

TILE, COL = FR.TILE, FR.COL
POS = ("pos_x", "pos_y", "pos_z")
VEL = ("vel_x", "vel_y", "vel_z")
KEYS = ("acc_x", "acc_y", "acc_z", "jerk_x", "jerk_y", "jerk_z")
ACC, JERK = KEYS[:3], KEYS[3:]
DTYPE = {32: np.float32, 64: np.float64}
U = F.U
FLOOR = {"acc": {32: 17.5, 64: 13.5}, "jerk": {32: 35.5, 64: 29.5}}  # include/nbx_jerk.h, "Error of one term"
_ROWS = 256  # bodies per chunk


def gate(k_ref, floor):
    return F.M * max(float(k_ref), float(floor), F.K_TERM)


# ---- states ------------------------------------------------------------------------------------------------------------------------
CONTEXT_SIZES = (1, 2, 3, 5, 257, 513, 2049, 4097)  # 5: the ragged ensemble's smallest member but one
ENSEMBLE = (3, 2049)                                 # members, n: cloud, clustered, rotation
ENSEMBLE_FAMILIES = ("cloud", "clustered", "rotation")
RAGGED_SIZES = (5, 2049, 257, 1, 513)                # every member a cloud
FAMILIES = ("cloud", "clustered", "rest", "rotation", "grid")
OMEGA = 2.0          # of the rigid rotation about z
PAIR_SPEED = (-20.0, 30.0, 10.0)  # of the planted close pair's passage
GRID = 1024.0        # the "grid" family's velocities are multiples of 1 / GRID
GRID_SHIFT = (0.5, -0.25, 2.0)


def families_of(n):
    out = ["cloud"]
    if n in (257, 2049):
        out.append("clustered")
    if n == 513:
        out += ["rest", "rotation"]
    if n == 2049:
        out += ["rotation", "grid"]
    return out


def context_cases():
    return [(n, fam) for n in CONTEXT_SIZES for fam in families_of(n)]


def make_state(precision, n, family):
    """n bodies in T: masses uniform in [0.5, 1.5] / G (G m of order 1), positions in [-1, 1]^3, velocities of order 1.
    cloud: uniform; clustered: eight Gaussian clumps of width 0.05, bodies 0 and 1 a pair 0.0046 apart passing at PAIR_SPEED;
    rest: every velocity 0; rotation: v = OMEGA e_z x x of the rounded positions, exact; grid: velocities on a 1 / GRID grid."""
    T = DTYPE[precision]
    rng = np.random.default_rng([9100, n, FAMILIES.index(family)])
    m = rng.uniform(0.5, 1.5, n) / float(G32)
    pos = rng.uniform(-1.0, 1.0, (3, n))
    vel = rng.uniform(-1.0, 1.0, (3, n))
    if family == "clustered":
        centres = rng.uniform(-1.0, 1.0, (3, 8))
        pos = centres[:, rng.integers(0, 8, n)] + 0.05 * rng.standard_normal((3, n))
        if n >= 2:
            pos[:, 1] = pos[:, 0] + np.array([0.004, 0.002, -0.001])
            vel[:, 1] = vel[:, 0] + np.array(PAIR_SPEED)
    pos = pos.astype(T)
    if family == "rest":
        vel[:] = 0.0
    elif family == "rotation":
        vel = np.stack([-OMEGA * pos[1].astype(np.float64), OMEGA * pos[0].astype(np.float64), np.zeros(n)])
    elif family == "grid":
        vel = np.rint(vel * GRID) / GRID
    s = dict(zip(POS + VEL + ("mass",), list(pos) + list(vel.astype(T)) + [m.astype(T)]))
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def shifted(state, shift=GRID_SHIFT):
    """The state with `shift` added to every velocity: exact for the "grid" family, so no difference of velocities changes."""
    out = {k: v.copy() for k, v in state.items()}
    for f, w in zip(VEL, shift):
        out[f] = (state[f].astype(np.float64) + w).astype(state[f].dtype)
        assert np.array_equal(out[f].astype(np.float64), state[f].astype(np.float64) + w)
    return out


LATTICE_K = 33  # 35 937 bodies: 71 columns x 15 splits
LATTICE_H, LATTICE_OMEGA = 4.0, 8.0


def lattice(precision, perm=False, k=LATTICE_K):
    """neighbours_ref.lattice(k, precision, perm) -- coordinates multiples of 1/8 -- in v = H x + Omega e_z x x, H and Omega powers
    of two, every mass 1 / G: every velocity, and every difference of two, is exact in both precisions."""
    s = NB.lattice(k, precision, perm)
    T = DTYPE[precision]
    x, y, z = (s[f].astype(np.float64) for f in POS)
    for f, v in zip(VEL, (LATTICE_H * x - LATTICE_OMEGA * y, LATTICE_H * y + LATTICE_OMEGA * x, LATTICE_H * z)):
        s[f] = np.ascontiguousarray(v.astype(T))
        assert np.array_equal(s[f].astype(np.float64), v)
    s["mass"] = np.full(k ** 3, 1.0 / float(G32), dtype=T)
    return s


def lattice_rows(k=LATTICE_K):
    """About 1000 bodies of the lattice: the first and the last, both sides of every column seam and of every split seam, and
    an even sample."""
    n = k ** 3
    columns, tiles, splits, per = FR.field_shape(n, n)
    rows = {0, n - 1}
    for s in [c * COL for c in range(1, columns)] + [s * per * TILE for s in range(1, splits)]:
        rows.update((s - 1, s))
    rows.update(range(7, n, max(1, n // 800)))
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


# ---- truth, metrics ----------------------------------------------------------------------------------------------------------------
def truth(state, precision, rows=None):
    """{"rows", "acc": (hi, lo, A (rows,)), "jerk": (hi, lo, B (rows, 3))}: hi + lo the sums of the module docstring for the
    bodies `rows` (all if None), (rows, 3) each."""
    wide = precision == 64 and F.HAVE_LONGDOUBLE
    dtype = np.longdouble if wide else np.float64
    n = len(state["mass"])
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    x = [np.asarray(state[f]).astype(dtype) for f in POS]
    v = [np.asarray(state[f]).astype(dtype) for f in VEL]
    g = gm_as_uploaded(state["mass"]).astype(dtype)
    m = len(rows)
    out = {k: (np.zeros((m, 3)), np.zeros((m, 3))) for k in ("acc", "jerk")}
    A, B = np.zeros(m), np.zeros((m, 3))

    def split(s):
        h = s.astype(np.float64)
        return h, (s - h.astype(dtype)).astype(np.float64)

    def chunk(ab):
        a, b = ab
        r = rows[a:b]
        d = [x[c][None, :] - x[c][r, None] for c in range(3)]
        u = [v[c][None, :] - v[c][r, None] for c in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + dtype(EPS2)
        w3 = g[None, :] / (r2 * np.sqrt(r2))
        rv = (d[0] * u[0] + d[1] * u[1] + d[2] * u[2]) * 3 / r2
        arv = (np.abs(d[0] * u[0]) + np.abs(d[1] * u[1]) + np.abs(d[2] * u[2])) * 3 / r2
        for c in range(3):
            t = d[c] * w3
            out["acc"][0][a:b, c], out["acc"][1][a:b, c] = split(t.sum(axis=1))
            A[a:b] = np.maximum(A[a:b], np.abs(t).sum(axis=1).astype(np.float64))
            out["jerk"][0][a:b, c], out["jerk"][1][a:b, c] = split(((u[c] - rv * d[c]) * w3).sum(axis=1))
            B[a:b, c] = ((np.abs(u[c]) + arv * np.abs(d[c])) * w3).sum(axis=1).astype(np.float64)

    P._pmap(chunk, F._row_chunks(m, n))
    return {"rows": rows, "acc": out["acc"] + (A,), "jerk": out["jerk"] + (B,)}


def at_rows(result, rows):
    """A result of all bodies restricted to `rows`."""
    return {k: np.asarray(result[k])[rows] for k in KEYS}


def k_values(got, tr, precision):
    """(K of the accelerations (rows,), K of the jerk (rows, 3)) of `got`, the six arrays at tr["rows"]."""
    wide = np.longdouble if (precision == 64 and F.HAVE_LONGDOUBLE) else np.float64
    k_acc = F.k_metric(np.stack([np.asarray(got[k]) for k in ACC], axis=1), tr["acc"], precision)
    hi, lo, B = tr["jerk"]
    j = np.stack([np.asarray(got[k]) for k in JERK], axis=1).astype(wide)
    err = np.abs((j - hi.astype(wide)) - lo.astype(wide)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        k_jerk = np.where(B > 0, err / (U[precision] * B), np.where(err == 0, 0.0, np.inf))
    k_jerk = np.where(np.isnan(k_jerk), np.inf, k_jerk)
    return np.where(np.isnan(k_acc), np.inf, k_acc), k_jerk


def compare(got, tr, gates, precision):
    """(problems, {"acc": largest K, "jerk": largest K}) of `got` (the six arrays at tr["rows"]) against truth and gates
    {"acc", "jerk"}: the comparison the device tests make."""
    k_acc, k_jerk = k_values(got, tr, precision)
    ks = {"acc": float(k_acc.max()), "jerk": float(k_jerk.max())}
    problems = []
    for key, k in (("acc", k_acc), ("jerk", k_jerk)):
        if not ks[key] <= gates[key]:
            at = np.unravel_index(int(np.argmax(k)), k.shape)
            problems.append("%s: K = %.3g > %.3g at row %d" % (key, ks[key], gates[key], int(tr["rows"][at[0]])))
    return problems, ks


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
FAULTS = ("the factor 3", "the sign of the second term", "r2^(-3/2) used for r2^(-5/2)", "u taken from the wrong j record",
          "the lane's second body using the first one's velocity", "a split dropped", "padding velocities read as the next system's",
          "the fp64 scale not undone", "1/r2 left at the raw seed in fp64")
FP64_FAULTS = FAULTS[7:]


def _fma(a, b, c, T):
    """a * b + c rounded once to T (fp32: evaluated in fp64; fp64: a multiply and an add)."""
    if T == np.float32:
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(T)
    return a * b + c


def restate(state, precision, fault=None, rows=None):
    """The six arrays in T at `rows` (all bodies if None), in the kernel's own order (see the module docstring), with one of
    FAULTS planted if asked for."""
    assert fault is None or fault in FAULTS, fault
    assert fault not in FP64_FAULTS or precision == 64, fault
    T = DTYPE[precision]
    n = len(state["mass"])
    columns, tiles, splits, per = FR.field_shape(n, n)
    npad = tiles * TILE
    pos = [np.zeros(npad, dtype=T) for _ in range(3)]
    vel = [np.zeros(npad, dtype=T) for _ in range(3)]
    gm = np.zeros(npad, dtype=T)
    for c in range(3):
        pos[c][:n] = state[POS[c]]
        vel[c][:n] = state[VEL[c]]
    gm[:n] = gm_as_uploaded(np.asarray(state["mass"], dtype=T)).astype(T)
    if precision == 64:
        gm = gm * T(0.125)  # the records' prescale, exact
    jvel = vel
    if fault == "padding velocities read as the next system's":
        assert n < npad
        jvel = [v.copy() for v in vel]
        for v in jvel:
            v[n:] = np.inf  # what the device tests put behind the system: a velocity that is not finite
    elif fault == "u taken from the wrong j record":
        jvel = [np.roll(v, -1) for v in vel]
    idx = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    src = idx
    if fault == "the lane's second body using the first one's velocity":  # bodies l and l + 256 of one column sit in one lane
        src = np.where(idx % COL >= TILE, idx - TILE, idx)
    xi = [p[idx] for p in pos]
    vi = [v[src] for v in vel]
    m = len(idx)
    use = splits - 1 if fault == "a split dropped" else splits
    assert use >= 1
    parts = np.zeros((use, m, 6), dtype=T)
    three = {"the factor 3": T(-1), "the sign of the second term": T(3)}.get(fault, T(-3))

    def chunk(ab):
        a, b = ab
        for s in range(use):
            j0, j1 = s * per * TILE, min(tiles, (s + 1) * per) * TILE
            d = [pos[c][None, j0:j1] - xi[c][a:b, None] for c in range(3)]
            u = [jvel[c][None, j0:j1] - vi[c][a:b, None] for c in range(3)]
            r2 = _fma(d[0], d[0], _fma(d[1], d[1], _fma(d[2], d[2], T(EPS2), T), T), T)
            with np.errstate(invalid="ignore"):
                rv = _fma(d[0], u[0], _fma(d[1], u[1], d[2] * u[2], T), T)
                g = gm[None, j0:j1]
                if precision == 32:
                    inv = FR._inv_sqrt(r2, T)
                    inv2 = inv * inv
                    sf = (g * inv) * inv2
                else:
                    y = (1.0 / np.sqrt(r2)).astype(np.float32).astype(T)  # a seed of 24 bits, as the hardware's
                    y2 = y * y
                    h = _fma(-r2, y2, T(1), T)
                    q = _fma(h, _fma(h, T(15), T(12), T), T(8), T)
                    if fault == "the fp64 scale not undone":
                        q = q * T(0.125)
                    sf = ((g * y) * y2) * q
                    inv2 = y2 if fault == "1/r2 left at the raw seed in fp64" else _fma(y2, _fma(h, h, h, T), y2, T)
                c_ = (rv * T(-3) if fault == "r2^(-3/2) used for r2^(-5/2)" else (rv * inv2) * three)
                terms = [d[c] * sf for c in range(3)] + [_fma(c_, d[c], u[c], T) * sf for c in range(3)]
                for c, t in enumerate(terms):
                    parts[s, a:b, c] = np.add.accumulate(t, axis=1, dtype=T)[:, -1]

    step = max(1, min(_ROWS, (1 << 20) // (per * TILE)))  # a chunk's temporaries stay at a few megabytes each
    P._pmap(chunk, [(a, min(a + step, m)) for a in range(0, m, step)])
    tot = np.zeros((m, 6))
    with np.errstate(invalid="ignore"):
        for s in range(use):
            tot += parts[s].astype(np.float64)
    out = tot.astype(T)
    return {k: out[:, c] for c, k in enumerate(KEYS)}


# ---- one case, everything computed once --------------------------------------------------------------------------------------------
_cases = {}


def case(precision, n, family, state=None, rows=None, name=None):
    """{"state", "truth", "kref", "gates"} of one (precision, n, family), cached; state, rows, name: another state under `name`
    at sampled rows (the lattice)."""
    key = (precision, n, name or family)
    if key not in _cases:
        st = make_state(precision, n, family) if state is None else state
        tr = truth(st, precision, rows)
        k_acc, k_jerk = k_values(restate(st, precision, rows=rows), tr, precision)
        kref = {"acc": float(k_acc.max()), "jerk": float(k_jerk.max())}
        _cases[key] = {"state": st, "truth": tr, "kref": kref, "gates": {k: gate(kref[k], FLOOR[k][precision]) for k in kref}}
    return _cases[key]


def lattice_case(precision, perm):
    n = LATTICE_K ** 3
    return case(precision, n, "lattice", state=lattice(precision, perm), rows=lattice_rows(), name="lattice perm=%d" % perm)


LARGE_K = 81  # 531 441 bodies: 1038 columns of one split
LARGE_ROWS = {32: 256, 64: 64}


def large_rows(precision):
    """LARGE_ROWS[precision] bodies of the large lattice: the first and the last, both sides of the first, a middle and the last
    column seam, and an even sample."""
    n = LARGE_K ** 3
    columns = FR.field_shape(n, n)[0]
    rows = {0, n - 1}
    for c in (1, columns // 2, columns - 1):
        rows.update((c * COL - 1, c * COL))
    want = LARGE_ROWS[precision]
    rows.update(np.linspace(1, n - 2, want - len(rows)).astype(np.int64).tolist())
    return np.array(sorted(rows), dtype=np.int64)


def large_case(precision):
    n = LARGE_K ** 3
    return case(precision, n, "lattice", state=lattice(precision, False, LARGE_K), rows=large_rows(precision), name="large lattice")


# ---- Hermite P(EC) in numpy --------------------------------------------------------------------------------------------------------
HERMITE_SEEDS = (307, 119)  # kick_ref's systems of 96 bodies: the members of the device test's ensemble
HERMITE_T = 0.25
HERMITE_STEPS = 16          # dt = T / 16 and T / 32 are compared, against T / 256 (dt / 16)


def hermite_state(seed=HERMITE_SEEDS[0]):
    return KR.make_state(seed, KR.N, np.float64)


def direct(state, fault=None):
    """(a, adot), each (3, n): the plain definition in fp64 with G m as uploaded; fault: one of the first three FAULTS."""
    x = np.stack([state[f].astype(np.float64) for f in POS])
    v = np.stack([state[f].astype(np.float64) for f in VEL])
    g = gm_as_uploaded(state["mass"]).astype(np.float64)
    d = x[:, None, :] - x[:, :, None]
    u = v[:, None, :] - v[:, :, None]
    r2 = (d * d).sum(axis=0) + EPS2
    w3 = g[None, :] / (r2 * np.sqrt(r2))
    rv = (d * u).sum(axis=0)
    c = {"the factor 3": -1.0 * rv / r2, "the sign of the second term": 3.0 * rv / r2, "r2^(-3/2) used for r2^(-5/2)": -3.0 * rv}.get(fault, -3.0 * rv / r2)
    return (d * w3).sum(axis=2), ((u + c * d) * w3).sum(axis=2)


def hermite(state, dt, nsteps, fault=None, evaluate=None):
    """nsteps Hermite P(EC) steps of dt in fp64, nbx.hermite's formulas: the state after them.  evaluate(state) -> (a, adot)
    (default: direct with `fault`)."""
    ev = evaluate or (lambda s: direct(s, fault))
    x = np.stack([state[f].astype(np.float64) for f in POS])
    v = np.stack([state[f].astype(np.float64) for f in VEL])
    mk = lambda x_, v_: dict(zip(POS + VEL + ("mass",), list(x_) + list(v_) + [state["mass"]]))
    a, j = ev(mk(x, v))
    for _ in range(nsteps):
        xp = x + dt * (v + dt * (a / 2.0 + dt * j / 6.0))
        vp = v + dt * (a + dt * j / 2.0)
        a1, j1 = ev(mk(xp, vp))
        v1 = v + dt * ((a + a1) / 2.0 + dt * (j - j1) / 12.0)
        x = x + dt * ((v + v1) / 2.0 + dt * (a - a1) / 12.0)
        v, a, j = v1, a1, j1
    return mk(x, v)


def state_error(a, b):
    """max |a - b| over positions and velocities."""
    return max(float(np.abs(np.asarray(a[f], dtype=np.float64) - np.asarray(b[f], dtype=np.float64)).max()) for f in POS + VEL)
