"""numpy reference, in fp64, of include/nbx_binaries.h: per body the most bound partner (lowest index among equal energies), the
specific two-body energy of that pair and the number of partners of negative energy -- from the state as stored: positions and
velocities as given (fp32 or fp64) and widened, G*m rounded as nbx_upload rounds it (energy_ref.gm_as_uploaded), eps^2 = 1e-3f
widened.  Every pair is evaluated as  e = A - B,  A = |v_j - v_i|^2 / 2,  B = (gm_i + gm_j) / sqrt(|x_j - x_i|^2 + eps^2).

The gate.  e cancels, so a device value is held to  |e_dev - e| <= GATE u (A + B)  of its pair, u the unit round-off of the
object's precision and GATE the project's own timescale gates, 32 in fp32 and 128 in fp64 (tests/test_timescale_gpu.py): each
term of e is a strict subset of the operations of nbx_timescale.h's approach and freefall; the header derives 6.5 u and, for a
reciprocal square root seed within 2^-24, 55.5 u to first order.  window(pair) = GATE u (A + B) is also what decides the rest:
    bound[i] must lie in [the pairs with e + window < 0, the pairs with e - window < 0] -- paircount's method: exact wherever the
        reference shows no pair inside the window around 0 (a pair of window 0 -- both massless, at one velocity -- is exact);
    partner[i] must EQUAL the reference's: ambiguity() counts the bodies whose runner-up, taken at the bottom of its window,
        reaches the top of the winner's window.  The states of the device tests have no such body at all
        (test_binaries_cpu.py asserts it for every (state, precision)): the seeds below were picked for that, here on the CPU.

restate() walks the pairs the way the kernels do -- j splits of field_shape(n, n), a candidate per split, the splits combined in
ascending order on strict < -- so that the faults a kernel of this structure can have may be planted (FAULTS); without a fault
the structure does not show in the result.  VELOCITY_FAULTS are the ways of pairing the second staged tile, the velocity records,
with the wrong position record; they show only where the velocities differ from record to record (lattice_ref.hubble).

binaries(), ambiguity(), restate() and compare() take rows=: only those bodies, each against ALL j, O(rows n) -- the reference
of the cloud of 35 937 bodies of tests/test_large_shapes_gpu.py.

The demo's own initial conditions have G m of about 1e-11: nothing there is bound.  The states here have masses of order 1/G.
"""
import numpy as np

import kick_ref as K
import neighbours_ref as NB
import timescale_ref as TS
from energy_ref import EPS2, G32, gm_as_uploaded
from field_ref import field_shape

KEYS = ("partner", "energy", "bound")
POS, VEL = K.FIELDS[:3], K.FIELDS[3:6]
DTYPE = {32: np.float32, 64: np.float64}
U = {32: 2.0 ** -24, 64: 2.0 ** -53}
GATE = {32: 32.0, 64: 128.0}
TILE = 256
G = float(G32)
CONTEXT_SIZES = (1, 2, 255, 256, 257, 513, 1025, 2049, 4097)
RAGGED_SIZES = NB.RAGGED_SIZES
ENSEMBLE_N = 2049
LATTICE_K = NB.LATTICE_K
FAULTS = ("self not masked", "padding record not masked", "padding velocity read", "ties to the highest j",
          "finish takes a later split on ties", "a split row dropped", "<= instead of < in the count", "m_j alone instead of m_i + m_j",
          "indices offset by the member's place")
# what a kernel that stages a SECOND tile, the velocity records of the same j, can get wrong in pairing the two; kept apart from
# FAULTS: on a state at rest every one of them changes nothing (tests/test_large_shapes_cpu.py shows it), which is why the large
# shapes carry velocities that are a function of the position (lattice_ref.hubble)
VELOCITY_FAULTS = ("velocity of record j + 1 read for record j", "velocity tile of the first split read in every split",
                   "velocity offset of the member not applied", "velocity index wraps at 65 536")
VELOCITY_WRAP = 65536
# seed of cloud(n) and of clustered(n): the first, counting up from 100 + n % 97 and 300 + n % 97, whose state has no ambiguous
# body in either precision
CLOUD_SEEDS = {1: 101, 2: 102, 255: 161, 256: 162, 257: 163, 513: 128, 1025: 155, 2049: 112, 4097: 123}
# cloud(35937), the large shapes' (tests/test_large_shapes_gpu.py): the first, counting up from 100 + n % 97, whose SAMPLED rows
# (test_large_shapes_gpu.cloud_rows) hold no ambiguous body in either precision and no body bound to nobody or to everybody
CLOUD_SEEDS[35937] = 147
CLUSTERED_SEEDS = {513: 328, 2049: 312}
SPEED = 1.4  # a component of a cloud velocity is uniform in [-SPEED, SPEED]: |dv|^2 / 2 is about 2, what G (m_i + m_j) / r is at r = 1


# ---- states ------------------------------------------------------------------------------------------------------------------------
def _cast(s, precision):
    return {k: np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(DTYPE[precision])) for k, v in s.items()}


def _cloud64(seed, n):
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.5, 1.5, n) / G
    pos = rng.uniform(-1.0, 1.0, (3, n))
    vel = SPEED * rng.uniform(-1.0, 1.0, (3, n))
    return dict(zip(K.FIELDS, list(pos) + list(vel) + [m]))


def cloud(n, precision, seed=None):
    """n bodies of G m in [0.5, 1.5], uniform in [-1, 1]^3, sub-virial (the system's virial speed grows as sqrt(n); a pair's
    own kinetic and potential terms are both about 2): every body has bound and unbound partners."""
    return _cast(_cloud64(CLOUD_SEEDS[n] if seed is None else seed, n), precision)


def reversed_cloud(n, precision):
    """cloud(n) with the bodies in reverse order: other indices, other tiles, the same physics."""
    return {k: np.ascontiguousarray(v[::-1]) for k, v in cloud(n, precision).items()}


def circular_pair(s, i, j, sep, axis=0):
    """Body j put `sep` from body i along `axis`, on the circular orbit of the unsoftened two-body problem about their common
    velocity (body i's, kept): relative speed sqrt(G (m_i + m_j) / sep), across the separation.  In place."""
    for c in range(3):
        s[POS[c]][j] = s[POS[c]][i] + (sep if c == axis else 0.0)
    speed = np.sqrt(G * (s["mass"][i] + s["mass"][j]) / sep)
    for c in range(3):
        s[VEL[c]][j] = s[VEL[c]][i] + (speed if c == (axis + 1) % 3 else 0.0)
    return s


BINARY_SEP, TRIPLE_INNER, TRIPLE_OUTER = 1.0 / 16, 1.0 / 16, 0.5


def planted(n):
    """What clustered(n) plants: tight binaries (i, j) whose members sit in different tiles where n allows, the triple
    (a, b, c) -- c on a circular orbit of TRIPLE_OUTER about a, which has b TRIPLE_INNER away --, two massless bodies moving
    as one, whose pair energy is 0 exactly, and two escapers, fast enough to be bound to nobody."""
    last = n - 1
    pairs = [(3, last - 2), (n // 2, n // 2 + 1), (last - 7, 5)]
    return {"binaries": pairs, "triple": (7, last - 11, n // 3), "massless": (11, last - 4), "escapers": (17, last - 20)}


def clustered(n, precision, seed=None):
    """cloud(n) spread over a box five times as wide (so that the planted systems are far tighter than their surroundings),
    with planted(n) in it.  n >= 64."""
    s = _cloud64(CLUSTERED_SEEDS[n] if seed is None else seed, n)
    for k in POS:
        s[k] = s[k] * 5.0
    p = planted(n)
    for axis, (i, j) in enumerate(p["binaries"]):
        circular_pair(s, i, j, BINARY_SEP, axis)
    a, b, c = p["triple"]
    circular_pair(s, a, b, TRIPLE_INNER, 0)
    s["mass"][c] = s["mass"][a] / 8.0
    circular_pair(s, a, c, TRIPLE_OUTER, 2)
    i, j = p["massless"]
    s["mass"][i] = s["mass"][j] = 0.0
    for k in VEL:
        s[k][j] = s[k][i]
    for sign, i in zip((1.0, -1.0), p["escapers"]):
        for k, speed in zip(VEL, (40.0, -30.0, 20.0)):
            s[k][i] = sign * speed
    return _cast(s, precision)


def encounter(precision):
    """timescale_ref's planted encounter (96 bodies, two heavy ones head-on), its masses scaled to order 1/G."""
    s = TS.encounter_state(TS.ENCOUNTER_SEEDS[0])
    s["mass"] = s["mass"] * len(s["mass"])
    return _cast(s, precision)


def lattice(precision, perm=False):
    """neighbours_ref.lattice(13, .) at rest with equal masses of 1/G: a body's energies are -2 / sqrt(r2), one value per
    distance class, and its most bound partners are its face neighbours, tied exactly."""
    s = NB.lattice(LATTICE_K, 64, perm)
    n = len(s["mass"])
    for k in VEL:
        s[k] = np.zeros(n)
    s["mass"] = np.full(n, 1.0 / G)
    return _cast(s, precision)


def member(n, precision):
    """The state a context or a ragged member of n bodies holds in the device tests."""
    return cloud(n, precision)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _arrays(state):
    x = [np.asarray(state[k], dtype=np.float64) for k in POS]
    v = [np.asarray(state[k], dtype=np.float64) for k in VEL]
    return x, v, gm_as_uploaded(state["mass"])


def _terms(x, v, gm, i, xj=None, vj=None, gmj=None, alone=False):
    """(A, B) of the bodies i (an index array) against all records j (default: the bodies themselves)."""
    xj, vj, gmj = x if xj is None else xj, v if vj is None else vj, gm if gmj is None else gmj
    d = [xj[c][None, :] - x[c][i, None] for c in range(3)]
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + EPS2
    w = [vj[c][None, :] - v[c][i, None] for c in range(3)]
    a = 0.5 * (w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    s = gmj[None, :] + (0.0 if alone else gm[i, None])
    return a, s / np.sqrt(r2)


def _row_chunks(n, rows, chunk):
    """The bodies asked for -- all n, or `rows` -- in chunks: (where the chunk's values go, the bodies)."""
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    assert rows.ndim == 1 and (rows.size == 0 or (0 <= rows.min() and rows.max() < n))
    return rows, [(slice(lo, min(len(rows), lo + chunk)), rows[lo:lo + chunk]) for lo in range(0, len(rows), chunk)]


def binaries(state, precision, chunk=512, rows=None):
    """{"partner", "energy", "bound"} of the state as stored -- the plain argmin (numpy's takes the first, i.e. lowest, index of
    equal values) and the plain count, in row chunks -- and what the comparison needs: "mag", A + B of the winning pair, and
    "bound_lo", "bound_hi", the bracket of the count.  rows: only these bodies, each against ALL j -- O(rows n); entry k of every
    array is body rows[k]'s."""
    x, v, gm = _arrays(state)
    n = len(gm)
    g = GATE[precision] * U[precision]
    rows, chunks = _row_chunks(n, rows, chunk)
    r = len(rows)
    out = {"partner": np.full(r, -1, dtype=np.int32), "energy": np.full(r, np.inf), "bound": np.zeros(r, dtype=np.int32),
           "mag": np.zeros(r), "bound_lo": np.zeros(r, dtype=np.int32), "bound_hi": np.zeros(r, dtype=np.int32)}
    for at, i in chunks:
        a, b = _terms(x, v, gm, i)
        e, win = a - b, g * (a + b)
        own = (np.arange(len(i)), i)
        e[own] = np.inf
        out["bound"][at] = (e < 0).sum(axis=1)
        out["bound_lo"][at] = (e + win < 0).sum(axis=1)
        out["bound_hi"][at] = (e - win < 0).sum(axis=1)
        if n > 1:
            j = e.argmin(axis=1)
            out["partner"][at] = j
            out["energy"][at] = e[own[0], j]
            out["mag"][at] = (a + b)[own[0], j]
    return out


def pair_energy(state, i, j):
    """(e, A + B) in fp64 of the pairs (i[k], j[k])."""
    x, v, gm = _arrays(state)
    i, j = np.asarray(i), np.asarray(j)
    r2 = sum((x[c][j] - x[c][i]) ** 2 for c in range(3)) + EPS2
    a = 0.5 * sum((v[c][j] - v[c][i]) ** 2 for c in range(3))
    b = (gm[i] + gm[j]) / np.sqrt(r2)
    return a - b, a + b


def ambiguity(state, precision, chunk=512, rows=None):
    """The number of bodies (of `rows`, where given) whose partner is ambiguous in the sense of the module's docstring."""
    x, v, gm = _arrays(state)
    n = len(gm)
    if n < 3:
        return 0
    g = GATE[precision] * U[precision]
    bad = 0
    for _, i in _row_chunks(n, rows, chunk)[1]:
        a, b = _terms(x, v, gm, i)
        e, win = a - b, g * (a + b)
        k = np.arange(len(i))
        e[k, i] = np.inf
        j = e.argmin(axis=1)
        top = e[k, j] + win[k, j]
        low = e - win
        low[k, j] = np.inf
        bad += int((low.min(axis=1) <= top).sum())
    return bad


def velocity_map(n_rec, per, fault):
    """Which velocity record a kernel with `fault` pairs with position record j, j < n_rec (-1: a zero record), per = the
    tiles of a split.  None: no velocity fault, record j."""
    j = np.arange(n_rec)
    if fault == "velocity of record j + 1 read for record j":
        return np.where(j + 1 < n_rec, j + 1, -1)
    if fault == "velocity tile of the first split read in every split":
        return j % (per * TILE)
    if fault == "velocity index wraps at 65 536":
        return j % VELOCITY_WRAP
    return None


def restate(state, precision, fault=None, offset=0, chunk=512, rows=None, member0=None):
    """The same values by the kernels' structure: the j range in splits of field_shape(n, n) over the padded records (zero
    position, zero mass; the velocity buffer has NO padding: what lies behind n is somebody else's), per split the lowest j of
    the smallest e (strict <, j ascending) and the count, the splits combined in ascending order on strict <.  `fault`: one of
    FAULTS or VELOCITY_FAULTS, planted; `offset`: the member's place, for the fault that adds it; `member0`: the state of the
    batch object's first member, whose velocity records a kernel that does not apply the member's velocity offset reads (behind
    its last one: the next member's, i.e. this state's own); `rows`: as binaries()."""
    assert fault is None or fault in FAULTS + VELOCITY_FAULTS, fault
    x, v, gm = _arrays(state)
    n = len(gm)
    _, tiles, splits, per = field_shape(n, n)
    n_rec = tiles * TILE
    pad = np.zeros(n_rec - n)
    xp = [np.concatenate([c, pad]) for c in x]
    gmp = np.concatenate([gm, pad])
    behind = [np.resize(c[::-1], n_rec - n) for c in v]  # what a read behind the last velocity finds: other bodies' velocities
    vp = [np.concatenate([c, b if fault == "padding velocity read" else pad]) for c, b in zip(v, behind)]
    if fault == "velocity offset of the member not applied":
        v0 = [np.asarray(member0[k], dtype=np.float64) for k in VEL]
        vp = [np.resize(np.concatenate([c0, c]), n_rec) for c0, c in zip(v0, v)]  # the j side alone: the i side is the column's own read
    vmap = velocity_map(n_rec, per, fault)
    if vmap is not None:
        vp = [np.where(vmap >= 0, c[np.maximum(vmap, 0)], 0.0) for c in vp]
    rows_all, chunks = _row_chunks(n, rows, chunk)
    r = len(rows_all)
    out = {"partner": np.full(r, -1, dtype=np.int32), "energy": np.full(r, np.inf), "bound": np.zeros(r, dtype=np.int32)}
    jj = np.arange(n_rec)
    for at, i in chunks:
        a, b = _terms(x, v, gm, i, xp, vp, gmp, alone=fault == "m_j alone instead of m_i + m_j")
        e = a - b
        rows = np.arange(len(i))
        ok = np.ones(e.shape, dtype=bool)
        if fault != "self not masked":
            ok[rows, i] = False
        ok[:, n:] = fault in ("padding record not masked", "padding velocity read")
        neg = (e <= 0) if fault == "<= instead of < in the count" else (e < 0)
        best = np.full(len(i), np.inf)
        bj = np.full(len(i), -1, dtype=np.int64)
        cnt = np.zeros(len(i), dtype=np.int64)
        for s in range(splits):
            if fault == "a split row dropped" and s == splits - 1 and splits > 1:
                continue
            j0, j1 = s * per * TILE, min(tiles, (s + 1) * per) * TILE
            part = np.where(ok[:, j0:j1], e[:, j0:j1], np.inf)
            if fault == "ties to the highest j":
                k = part.shape[1] - 1 - part[:, ::-1].argmin(axis=1)
            else:
                k = part.argmin(axis=1)
            cand = part[rows, k]
            take = (cand <= best) & np.isfinite(cand) if fault == "finish takes a later split on ties" else cand < best
            best = np.where(take, cand, best)
            bj = np.where(take, jj[j0:j1][k], bj)
            cnt += (neg[:, j0:j1] & ok[:, j0:j1]).sum(axis=1)
        if fault == "indices offset by the member's place":
            bj = np.where(bj >= 0, bj + offset, bj)
        out["partner"][at], out["energy"][at], out["bound"][at] = bj, best, cnt
    return out


def compare(got, want, state, precision, bound=True, rows=None):
    """What the device tests ask of a result `got` against the reference `want` = binaries(state): (problems, the largest energy
    error in units of u (A + B)).  partner equal on every body; energy within the gate of the reference value of ITS OWN pair
    and of the reference minimum; bound inside the bracket.  rows: `want` = binaries(state, rows=rows) and `got`, a result over
    all bodies, is held to it on those bodies alone."""
    problems = []
    n = len(want["partner"])
    total = len(state["mass"])
    body = np.arange(total) if rows is None else np.asarray(rows, dtype=np.int64)
    if rows is not None:
        full = all(np.asarray(got[k]).shape == (total,) for k in (KEYS if bound else KEYS[:2]))
        got = {k: np.asarray(got[k])[body] if full else np.zeros(0) for k in (KEYS if bound else KEYS[:2])}
    gp = np.asarray(got["partner"])
    if gp.shape != (n,) or not np.array_equal(gp, want["partner"]):
        problems.append("partner differs on %d bodies" % ((gp != want["partner"]).sum() if gp.shape == (n,) else n))
    ge = np.asarray(got["energy"], dtype=np.float64)
    fin = np.isfinite(want["energy"])
    worst = 0.0
    if not np.array_equal(fin, np.isfinite(ge)) or not (ge[~fin] == np.inf).all():
        problems.append("energy is finite where the reference is not, or the reverse")
    elif fin.any():
        u = U[precision]
        err_min = np.abs(ge[fin] - want["energy"][fin]) / (u * want["mag"][fin])
        worst = float(err_min.max())
        idx = np.nonzero(fin)[0]
        valid = (gp.shape == (n,)) and ((gp[idx] >= 0) & (gp[idx] < total) & (gp[idx] != body[idx])).all()
        if valid:
            e_own, mag_own = pair_energy(state, body[idx], gp[idx])
            worst = max(worst, float((np.abs(ge[fin] - e_own) / (u * mag_own)).max()))
        if not valid or worst > GATE[precision]:
            problems.append("energy is %.1f u (A + B) from the reference" % worst)
    if bound:
        gb = np.asarray(got["bound"])
        if gb.shape != (n,) or ((gb < want["bound_lo"]) | (gb > want["bound_hi"])).any():
            problems.append("bound leaves the bracket")
    return problems, worst


def differs(got, want, state, precision):
    """What the comparison of the device tests sees between a result and the reference."""
    return bool(compare(got, want, state, precision)[0])


def identities(res):
    """The Consequences of the header on one system's result, as a list of the ones that fail."""
    p, e, b = np.asarray(res["partner"]), np.asarray(res["energy"]), np.asarray(res["bound"])
    bad = []
    if len(p) > 1:
        if not (e[p] <= e).all():
            bad.append("partner[i] == j but energy[j] > energy[i]")
        mutual = p[p] == np.arange(len(p))
        if not np.array_equal(e[mutual], e[p][mutual]):
            bad.append("a mutual pair with two energies")
    if not np.array_equal(b > 0, e < 0):
        bad.append("(bound > 0) != (energy < 0)")
    if int(b.astype(np.int64).sum()) % 2:
        bad.append("the sum of bound is odd")
    return bad


def catalogue(partner, energy, mass, x, y, z, vx, vy, vz):
    """nbx.binary_catalogue as a plain loop: rows (i, j, energy, a, ecc, period, binding), by binding energy, descending."""
    rows = []
    for i in range(len(partner)):
        j = int(partner[i])
        if j > i and int(partner[j]) == i and energy[i] < 0:
            d = np.array([float(x[j]) - float(x[i]), float(y[j]) - float(y[i]), float(z[j]) - float(z[i])])
            w = np.array([float(vx[j]) - float(vx[i]), float(vy[j]) - float(vy[i]), float(vz[j]) - float(vz[i])])
            gm = G * (float(mass[i]) + float(mass[j]))
            e = 0.5 * float(w @ w) - gm / float(np.sqrt(d @ d))
            a = -gm / (2.0 * e)
            h = np.cross(d, w)
            ecc = float(np.sqrt(max(1.0 + 2.0 * e * float(h @ h) / gm ** 2, 0.0)))
            mu = float(mass[i]) * float(mass[j]) / (float(mass[i]) + float(mass[j]))
            rows.append((i, j, e, a, ecc, 2.0 * np.pi * float(np.sqrt(a ** 3 / gm)), mu * abs(e)))
    return sorted(rows, key=lambda r: (-r[6], r[0]))
