"""The pair-work analysis kernels -- the potential of nbx_diagnostics, nbx_timescale, nbx_field, nbx_neighbours, nbx_paircount and
their ensemble and ragged forms -- at the launch shapes the other device modules never reach (they stop at n = 4099: nine
columns, four splits), against references that do not cost O(n^2): the closed forms of tests/lattice_ref.py on a cubic lattice
of equal masses, and row-sampled high-precision sums.

Shapes (REGIMES; tests/test_large_shapes_cpu.py holds the table against the headers' rule): k = 33, 35 937 bodies, the target
regime, 71 columns x 15 splits of 10 tiles, the last split one tile; k = 81, 531 441 bodies, 1038 columns of ONE split walking
2076 tiles; k = 25 (fp32) and 23 (fp64), the largest lattices a batch member holds, 13 x 5 and 12 x 4 tiles, alone in an ensemble
and among members of 5 and 8192 bodies in a ragged ensemble, where the workgroups of the small members return early from a grid
sized for the large one; nbx_field at (m, n) = (300, 262 657): one column of 206 splits, (524 289, 257): 1025 columns of one
split, the last column one point, (32 769, 32 769): 65 x 15, and (65 537 points, one member).  Every reduce that walks partial
rows in strides of 256 -- the potential's, the timescale's, the pair counts' finish -- meets more than 256 rows here
(test_every_kernel_family_meets_more_than_256_partial_rows).

What is asked.  neighbours: index and within EQUAL neighbours_ref.lattice_expected, every r2 one bit pattern within 8 u of
1/64 + eps^2 and its minimum bit for bit nbx_timescale's min_r2; the tie radius gives the same.  paircount: twenty radii -- the
six shells of paircount_ref.LATTICE_RADII, +inf, 0 and twelve mid-shell values up to squared lattice radius 1500.5 -- EQUAL
lattice_ref.pair_counts; at k = 81 the radius sqrt(291.5) / 8 counts 4 312 359 684 > 2^32 pairs and +inf 141 214 502 520, which a
finish that added in 32 bits would not return.  timescale: a lattice at rest with one planted body, at the first and last body
and both sides of a column and a split seam, rates within 32 u (fp32) / 128 u (fp64), min_r2 within 8 u of
lattice_ref.timescale_expected.  potential: (a) the total within (256 + 16) u |U| of lattice_ref.potential -- all terms have one
sign, a lane adds one 256-record tile in T (255 additions, csrc/nbx_diag_body.hpp: diag_tile starts every tile from 0 and
diag_body widens each tile sum to fp64) and force_ref.K_TERM = 16 u covers a term; (b) one heavy body, mass 1 among masses of
2^-40, at the seams: the total is then the row plus the column of that body, known in O(n) on the lattice because the all-light
total is the closed form, held to the potential probe's floor gate of 32 u (2 max(K_ref, 16) with K_ref not evaluated: never
wider than the probe's).  field: K <= 2 max(K_ref, 16) on both quantities against field_ref.truth_at, on every point of the
first two shapes and on about 1000 points of the others (first, last, both sides of every column seam, seeded random ones);
K_ref is the CPU oracle's (acceleration) and the sequential sum's (potential) on a subsample of those points, which can only
narrow the gate; and with the k = 33 lattice as bodies and its own sites as points, 1/2 sum m phi_i plus the self terms is
lattice_ref.potential within (256 t + 17) u, t = 10 the tiles of a split that field_body adds in T.

Every case's shape, worst deviation, gate, largest count and time go to large_shapes.json in the GPU suite's report directory
(OUT of tests/test_parity_gpu.py).

Measured on an MI355X when this module was written (no value of these kernels above n = 4099 had been held against a reference
before): nothing failed, no kernel was changed.  neighbours and paircount: every index, count and pair count equal at every
shape, r2 0.12 u from 1/64 + eps^2 in fp32 and exact in fp64; the largest count 141 214 502 520.  potential (a): 0.27 u (fp32) and
2.3 u (fp64) of 272 on the contexts, 3.5 u on a member; (b): K_max 0.73 in fp32 and 12.1 in fp64 (k = 81) of 32, where one lost
256-record tile of one lane is 2^23 * 256 / n = 4041 u at k = 81 in fp32 (one pair: 15.8 u there, 233 u at k = 33).  timescale:
rates 0.15 u of 32 (fp32) and 1.8 u of 128 (fp64), min_r2 0.4 u of 8.  field: closest to its gate at (524 289, 257), where a
point's sum has 512 terms and K_ref stays under the floor: K 21.1 (acceleration) and 19.6 (potential) of 32 in fp32, 19.8 and
19.0 in fp64; elsewhere K <= 25.1 under gates of 84 and more; the lattice's own sites 4.3 u (fp32) and 18.4 u (fp64) of 2577.  One call at k = 81,
fp32 / fp64: neighbours 0.11 / 0.15 s, potential 0.064 / 0.134 s, timescale 0.12 / 0.29 s, paircount of twenty radii 0.59 / 0.60 s
-- no case needed the drop to k = 80; the slowest tests, the heavy-body sweep and paircount at k = 81 in fp64, take 3.7 s, the
module about a minute.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import field_ref as FR
import force_ref as F
import lattice_ref as L
import neighbours_ref as NB
import paircount_ref as PC
import potential_ref as P
from conftest import PKG, ROOT
from energy_ref import EPS2, gm_as_uploaded

pytestmark = pytest.mark.gpu

U = NB.U
CONTEXT_K = (33, 81)
MEMBER_K = {32: 25, 64: 23}
SMALL_MEMBERS = (5, 8192)  # the ragged members either side of the lattice
RATE_GATE = {32: 32.0, 64: 128.0}  # tests/test_timescale_gpu.py
R2_GATE = NB.R2_GATE
POTENTIAL_GATE = 256.0 + F.K_TERM  # bound (a), in u |U|
PROBE_GATE = F.gate(0.0)  # bound (b): 2 max(0, 16)
STEP_DT = 1.0 / 16  # the lattice's velocities are about 0.3: a step moves a body across a shell gap

# (columns, tiles, splits, tiles per split) of field_shape(m, n) / diag_shape(n, n), tiles of the last split, records of the last tile
REGIMES = {
    "k33": ((35937, 35937), (71, 141, 15, 10), 1, 97),
    "k81": ((531441, 531441), (1038, 2076, 1, 2076), 2076, 241),
    "k25": ((15625, 15625), (31, 62, 13, 5), 2, 9),
    "k23": ((12167, 12167), (24, 48, 12, 4), 4, 135),
    "field one column": ((300, 262657), (1, 1027, 206, 5), 2, 1),
    "field one split": ((524289, 257), (1025, 2, 1, 2), 2, 1),
    "field target": ((32769, 32769), (65, 129, 15, 9), 3, 1),
    "field member fp32": ((65537, 15625), (129, 62, 8, 8), 6, 9),
    "field member fp64": ((65537, 12167), (129, 48, 8, 6), 6, 135),
}

SHELLS = (9, 14, 20, 27, 38, 50, 75, 110, 170, 291, 600, 1500)  # squared lattice radii m: the device radius is sqrt(m + 0.5) / 8
SQUARED = [m + 0.5 for m in range(1, 7)] + [math.inf, 0.0] + [m + 0.5 for m in SHELLS]
RADII = PC.LATTICE_RADII + [math.inf, 0.0] + [L.radius_of(m) for m in SHELLS]
assert len(RADII) == 20 and PC.pass_slots(len(RADII)) == [(0, 16, 16), (16, 4, 4)]

RECORDS = []
_cache = {}


def record(**kw):
    RECORDS.append(kw)
    print(json.dumps(kw))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    from test_parity_gpu import OUT  # where the GPU suite leaves its reports
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "large_shapes.json"), "w") as f:
        json.dump({"u": "2^-24 (fp32) or 2^-53 (fp64)", "cases": RECORDS}, f, indent=1)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def lattice(k, precision, perm):
    return cached(("lattice", k, precision, perm), lambda: L.state(k, precision, perm))


def expected(k, perm):
    return cached(("expected", k, perm), lambda: NB.lattice_expected(k, perm))


def counts_expected(k, squared=None):
    return cached(("counts", k), lambda: L.pair_counts(k, SQUARED)) if squared is None else L.pair_counts(k, squared)


def shape_of(k):
    return FR.field_shape(k ** 3, k ** 3)


# ---- the comparisons (tests/test_large_shapes_cpu.py plants faults against these same functions) -------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def same(a, b):
    return all(np.array_equal(bits(a[f]), bits(b[f])) for f in NB.KEYS)


def check_neighbours(got, tie, k, perm, precision):
    """index and within EQUAL the geometry's at the mid-shell radius and at the tie radius, one r2 bit pattern inside the gate.
    Returns the deviation of r2 in u."""
    index, faces = expected(k, perm)
    for res, what in ((got, "mid-shell"), (tie, "tie")):
        bad = np.flatnonzero(np.asarray(res["index"]) != index)
        assert bad.size == 0, (what, "index", bad.size, bad[:8].tolist())
        bad = np.flatnonzero(np.asarray(res["within"]) != faces)
        assert bad.size == 0, (what, "within", bad.size, bad[:8].tolist())
    r2 = np.asarray(got["r2"])
    assert (bits(r2) == bits(r2)[0]).all(), ("r2 bits differ", np.flatnonzero(bits(r2) != bits(r2)[0])[:8].tolist())
    assert np.array_equal(bits(np.asarray(tie["r2"])), bits(r2))
    dev = abs(float(r2[0]) - L.FACE_R2) / (U[precision] * L.FACE_R2)
    assert dev <= R2_GATE, dev
    return dev


def check_counts(got, k, squared=None):
    """Every count EQUALS the closed form.  Returns the largest count."""
    want = counts_expected(k, squared)
    got = [int(v) for v in np.asarray(got).tolist()]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    return max(got)


def potential_deviation(u, k, precision):
    """|U - truth| in u |truth| against lattice_ref.potential."""
    hi, lo = cached(("potential", k, precision), lambda: L.potential(k, precision))
    return abs((u - hi) - lo) / (U[precision] * abs(hi))


def check_potential(u, k, precision):
    dev = potential_deviation(u, k, precision)
    assert dev <= POTENTIAL_GATE, (k, precision, u, dev)
    return dev


def check_timescale(got, want, precision):
    """The rates inside 32 u / 128 u, min_r2 inside 8 u; a rate of 0 must be exactly 0.  Returns the three deviations in u."""
    devs = {}
    for f in ("approach_rate2", "freefall_rate2", "min_r2"):
        if want[f] == 0.0:
            assert got[f] == 0.0, (f, got[f])
            devs[f] = 0.0
            continue
        devs[f] = abs(got[f] - want[f]) / want[f] / U[precision]
        assert devs[f] <= (R2_GATE if f == "min_r2" else RATE_GATE[precision]), (f, got[f], want[f], devs[f])
    return devs


def check_field(result, case, precision):
    """field_ref's two gates on the points of `case` ({"truth", "gate_acc", "gate_phi"}).  Returns (K acc, K phi)."""
    ka = float(FR.k_acc([result["acc_x"], result["acc_y"], result["acc_z"]], case["truth"], precision).max())
    kp = float(FR.k_phi(result["phi"], case["truth"], precision).max())
    assert ka <= case["gate_acc"], ("acc", ka, case["gate_acc"])
    assert kp <= case["gate_phi"], ("phi", kp, case["gate_phi"])
    return ka, kp


# ---- the heavy body on the lattice -----------------------------------------------------------------------------------------------------
def heavy_lattice_state(k, precision, perm, body):
    """The lattice at rest, every mass 2^-40 but mass 1 at `body`."""
    s = dict(lattice(k, precision, perm))
    n = k ** 3
    T = NB.DTYPE[precision]
    for f in L.VEL:
        s[f] = np.zeros(n, dtype=T)
    s["mass"] = np.full(n, P.LIGHT, dtype=T)
    s["mass"][body] = 1.0
    return s


def heavy_lattice_truth(k, precision, perm, bodies):
    """(hi, lo) per body: with s = 2^-40, g = G s and g1 = G 1 as uploaded, S the sum of W over all ordered pairs and S_k that
    over the partners of k, sum_i m_i sum_j W_ij G m_j = s g S + (1 - s) g S_k + (g1 - g) s S_k, and U = -1/2 of it.  S is the closed form; S_k is one
    row, in np.longdouble."""
    from decimal import Decimal, localcontext
    T = NB.DTYPE[precision]
    g = float(gm_as_uploaded(np.full(1, P.LIGHT, dtype=T))[0])
    g1 = float(gm_as_uploaded(np.ones(1, dtype=T))[0])
    st = lattice(k, precision, perm)
    x = [st[f].astype(np.longdouble) for f in NB.POS]
    S = L.inverse_distance_sum(k)
    hi, lo = np.zeros(len(bodies)), np.zeros(len(bodies))
    for a, b in enumerate(bodies):
        r2 = sum((c - c[b]) ** 2 for c in x) + np.longdouble(EPS2)
        w = 1.0 / np.sqrt(r2)
        w[b] = 0.0
        sk = w.sum()
        sk_hi = float(sk)
        with localcontext() as ctx:
            ctx.prec = 50
            Sk = Decimal(sk_hi) + Decimal(float(sk - np.longdouble(sk_hi)))
            s = Decimal(P.LIGHT)
            total = -(s * Decimal(g) * S + (1 - s) * Decimal(g) * Sk + (Decimal(g1) - Decimal(g)) * s * Sk) / 2
            hi[a] = float(total)
            lo[a] = float(total - Decimal(hi[a]))
    return hi, lo


def seam_bodies(n, shape, count=24):
    """Bodies 0 and n - 1, both sides of column seams and of split seams (first, middle and last of each), then seeded random
    ones up to `count`."""
    columns, tiles, splits, per = shape
    cuts = set()
    for c in {1, columns // 2, columns - 1}:
        cuts.add(c * 512)
        cuts.add(c * 512 - 256)  # the lane's second body
    for s in {1, splits // 2, splits - 1}:
        if 0 < s < splits:
            cuts.add(s * per * 256)
    out = {0, n - 1}
    for c in cuts:
        if 0 < c < n:
            out.update((c - 1, c))
    rng = np.random.default_rng([13, n])
    while len(out) < count:
        out.add(int(rng.integers(0, n)))
    return sorted(out)


# ---- contexts ----------------------------------------------------------------------------------------------------------------------------
CONTEXT_CASES = [(k, precision, perm) for k in CONTEXT_K for precision in (32, 64) for perm in (False, True)]
case_name = lambda c: "k%d-fp%d-%s" % (c[0], c[1], "permuted" if c[2] else "natural")


def context_neighbours(nbx, k, precision, perm):
    """What a default context holding the lattice returns at the mid-shell radius, asked once: the bits the members are held to."""
    def ask():
        with nbx.Context(k ** 3, precision) as c:
            c.upload(lattice(k, precision, perm))
            return c.neighbours(NB.LATTICE_RADIUS)
    return cached(("ctx neighbours", k, precision, perm), ask)


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=case_name)
def test_neighbours_of_a_context(nbx, case):
    k, precision, perm = case
    n = k ** 3
    t0 = time.perf_counter()
    with nbx.Context(n, precision) as c:
        c.upload(lattice(k, precision, perm))
        got = c.neighbours(NB.LATTICE_RADIUS)
        seconds = time.perf_counter() - t0
        assert same(c.neighbours(NB.LATTICE_RADIUS), got)  # the same call twice: the same bits
        tie = c.neighbours(NB.LATTICE_TIE_RADIUS)
        ts = c.timescale()
        dev = check_neighbours(got, tie, k, perm, precision)
        assert float(got["r2"].min()) == ts["min_r2"]  # bit for bit
        _cache.setdefault(("ctx neighbours", k, precision, perm), got)
        c.step(1, STEP_DT, kenergy=False)
        moved = c.neighbours(NB.LATTICE_RADIUS)
        assert not np.array_equal(bits(moved["r2"]), bits(got["r2"]))  # not a stale answer
        assert same(c.neighbours(NB.LATTICE_RADIUS), moved)
    record(kernel="neighbours", case=case_name(case), shape=shape_of(k), r2_u=dev, gate_u=R2_GATE, upload_and_call_s=seconds)


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=case_name)
def test_paircount_of_a_context(nbx, case):
    k, precision, perm = case
    n = k ** 3
    with nbx.Context(n, precision) as c:
        c.upload(lattice(k, precision, perm))
        c.sync()
        t0 = time.perf_counter()
        got = c.paircount(RADII)
        seconds = time.perf_counter() - t0
        largest = check_counts(got, k)
        assert np.array_equal(c.paircount(RADII), got)
        assert int(got[6]) == n * (n - 1) // 2
        if k == 81:
            assert n * (n - 1) // 2 == 141214502520 and 2 ** 32 < int(got[RADII.index(L.radius_of(291))]) < 2 ** 33  # a FINITE radius above 2^32
        check_counts(c.paircount(RADII[:19]), k, SQUARED[:19])  # a last pass with an unused slot
        check_counts(c.paircount([NB.LATTICE_TIE_RADIUS]), k, [1.0])  # h2 is bit for bit the face neighbours' r2: <= counts them
        within = c.neighbours(RADII[0])["within"].sum(dtype=np.int64)
        assert int(within) == 2 * int(got[0]) == 6 * k * k * (k - 1)
        c.step(1, STEP_DT, kenergy=False)
        moved = c.paircount(RADII)
        assert not np.array_equal(moved, got) and int(moved[6]) == n * (n - 1) // 2 and int(moved[7]) == 0
        assert np.array_equal(c.paircount(RADII), moved)
    record(kernel="paircount", case=case_name(case), shape=shape_of(k), radii=len(RADII), largest_count=largest, call_s=seconds)


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=case_name)
def test_the_total_potential_of_a_context(nbx, case):
    k, precision, perm = case
    with nbx.Context(k ** 3, precision) as c:
        c.upload(lattice(k, precision, perm))
        c.sync()
        t0 = time.perf_counter()
        d = c.diagnostics()
        seconds = time.perf_counter() - t0
        dev = check_potential(d["potential"], k, precision)
        assert d["mass"] == float(k ** 3) and c.diagnostics() == d
        c.step(1, STEP_DT, kenergy=False)
        moved = c.diagnostics()
        assert moved["potential"] != d["potential"] and c.diagnostics() == moved
    record(kernel="potential", case=case_name(case), shape=shape_of(k), total_u=dev, gate_u=POTENTIAL_GATE, call_s=seconds)


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=case_name)
def test_one_heavy_body_at_the_seams(nbx, case):
    k, precision, perm = case
    n = k ** 3
    bodies = seam_bodies(n, shape_of(k))
    hi, lo = heavy_lattice_truth(k, precision, perm, bodies)
    got = np.zeros(len(bodies))
    with nbx.Context(n, precision) as c:
        for a, b in enumerate(bodies):
            c.upload(heavy_lattice_state(k, precision, perm, b))
            got[a] = c.diagnostics()["potential"]
    K = P.k_metric(got, (hi, lo), precision)
    record(kernel="potential, heavy body", case=case_name(case), shape=shape_of(k), bodies=len(bodies), K_max=float(K.max()),
           K_median=float(np.median(K)), gate=PROBE_GATE, one_pair_in_u=float(2.0 ** (23 if precision == 32 else 52) / n))
    bad = np.flatnonzero(~(K <= PROBE_GATE))
    assert bad.size == 0, [(bodies[i], float(K[i])) for i in bad[:10]]


def timescale_sites(n, shape):
    columns, tiles, splits, per = shape
    seam = per * 256 if splits > 1 else (tiles // 2) * 256  # one split: a tile seam in the middle of its walk
    return [0, n - 1, 511, 512, seam - 1, seam]


@pytest.mark.parametrize("case", CONTEXT_CASES, ids=case_name)
def test_timescale_of_a_context_with_one_planted_body(nbx, case):
    k, precision, perm = case
    n = k ** 3
    rest = L.state(k, precision, perm, at_rest=True)
    worst = {}
    with nbx.Context(n, precision) as c:
        c.upload(rest)
        c.sync()
        t0 = time.perf_counter()
        plain = c.timescale()
        seconds = time.perf_counter() - t0
        check_timescale(plain, L.timescale_background(precision), precision)
        assert c.timescale() == plain
        for body in timescale_sites(n, shape_of(k)):
            c.upload(L.plant(rest, body))
            got = c.timescale()
            devs = check_timescale(got, L.timescale_expected(k, body, precision, perm), precision)
            assert got["min_r2"] < 0.5 * plain["min_r2"] and got["approach_rate2"] > 0.0
            worst = {f: max(v, worst.get(f, 0.0)) for f, v in devs.items()}
        c.step(1, STEP_DT / 4, kenergy=False)  # the planted body moves 1/32 in y, not onto the next site's 1/8
        moved = c.timescale()
        assert moved["steps_done"] == 1 and moved["min_r2"] != got["min_r2"] and c.timescale() == moved
    record(kernel="timescale", case=case_name(case), shape=shape_of(k), worst_u=worst, rate_gate_u=RATE_GATE[precision], r2_gate_u=R2_GATE, call_s=seconds)


# ---- members -------------------------------------------------------------------------------------------------------------------------------
def small_member(n, precision):
    return cached(("small", n, precision), lambda: NB.member(n, precision))


def context_of(nbx, state, precision, what, radii=None):
    """What a context of the state's size returns for it."""
    with nbx.Context(len(state["mass"]), precision) as c:
        c.upload(state)
        if what == "neighbours":
            return c.neighbours(NB.LATTICE_RADIUS)
        if what == "paircount":
            return c.paircount(radii)
        if what == "timescale":
            return c.timescale()
        return c.diagnostics()


@pytest.mark.parametrize("precision", [32, 64])
def test_members_of_an_ensemble(nbx, precision):
    k = MEMBER_K[precision]
    n = k ** 3
    states = [lattice(k, precision, False), lattice(k, precision, True)]
    with nbx.Ensemble(n, 2, precision) as e:
        e.upload(states)
        nb, tie, pc, d, ts = e.neighbours(NB.LATTICE_RADIUS), e.neighbours(NB.LATTICE_TIE_RADIUS), e.paircount(RADII), e.diagnostics(), e.timescale()
        assert np.array_equal(e.paircount(RADII), pc) and e.diagnostics() == d
        for m, perm in enumerate((False, True)):
            got = {f: nb[f][m] for f in NB.KEYS}
            dev = check_neighbours(got, {f: tie[f][m] for f in NB.KEYS}, k, perm, precision)
            assert same(got, context_of(nbx, states[m], precision, "neighbours"))
            assert float(got["r2"].min()) == ts[m]["min_r2"]
            largest = check_counts(pc[m], k)
            assert np.array_equal(pc[m], context_of(nbx, states[m], precision, "paircount", RADII))
            pdev = check_potential(d[m]["potential"], k, precision)
            assert d[m] == context_of(nbx, states[m], precision, "diagnostics")
            record(kernel="ensemble member", case=case_name((k, precision, perm)), shape=shape_of(k), r2_u=dev, largest_count=largest,
                   potential_u=pdev, potential_gate_u=POTENTIAL_GATE)
        e.step(1, STEP_DT, kenergy=False)
        assert not np.array_equal(e.paircount(RADII), pc) and not np.array_equal(bits(e.neighbours(NB.LATTICE_RADIUS)["r2"]), bits(nb["r2"]))


@pytest.mark.parametrize("precision", [32, 64])
def test_members_of_a_ragged_ensemble_among_small_ones(nbx, precision):
    k = MEMBER_K[precision]
    n = k ** 3
    sizes = (SMALL_MEMBERS[0], n, SMALL_MEMBERS[1], n)
    rest = L.state(k, precision, True, at_rest=True)
    planted = L.plant(rest, shape_of(k)[3] * 256)  # the first body behind the first split seam
    states = [small_member(sizes[0], precision), lattice(k, precision, False), small_member(sizes[2], precision), planted]
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        nb, tie, pc, d, ts = r.neighbours(NB.LATTICE_RADIUS), r.neighbours(NB.LATTICE_TIE_RADIUS), r.paircount(RADII), r.diagnostics(), r.timescale()
        assert np.array_equal(r.paircount(RADII), pc) and r.diagnostics() == d and r.timescale() == ts
        dev = check_neighbours(nb[1], tie[1], k, False, precision)
        largest = check_counts(pc[1], k)
        pdev = check_potential(d[1]["potential"], k, precision)
        tdev = check_timescale(ts[3], L.timescale_expected(k, shape_of(k)[3] * 256, precision, True), precision)
        for m in range(4):  # every member, the small ones that leave the grid early included, has the bits of a context of its size
            assert same(nb[m], context_of(nbx, states[m], precision, "neighbours")), m
            assert np.array_equal(pc[m], context_of(nbx, states[m], precision, "paircount", RADII)), m
            assert d[m] == context_of(nbx, states[m], precision, "diagnostics"), m
            assert ts[m] == context_of(nbx, states[m], precision, "timescale"), m
        assert np.array_equal(r.paircount(RADII, 0, 1), pc[:1]) and np.array_equal(r.paircount(RADII, 2, 1), pc[2:3])  # a grid of the small member's own
        r.step(1, STEP_DT, kenergy=False)
        assert not np.array_equal(r.paircount(RADII), pc)
    record(kernel="ragged member", case=case_name((k, precision, False)), shape=shape_of(k), r2_u=dev, largest_count=largest, potential_u=pdev,
           potential_gate_u=POTENTIAL_GATE, timescale_u=tdev)


CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import nbx, lattice_ref as L, test_large_shapes_gpu as G
out = {}
for precision in (32, 64):
    with nbx.Context(33 ** 3, precision) as c:
        c.upload(L.state(33, precision, True))
        out[str(precision)] = c.paircount(G.RADII).tolist()
print(json.dumps(out))
""" % (PKG, os.path.join(ROOT, "tests"))


def test_both_counting_schemes_give_the_closed_form_in_the_target_regime():
    """NBX_PAIRCOUNT_SCHEME=lane and =wave, each in a fresh child process, k = 33, the permuted lattice, both precisions."""
    for scheme in ("lane", "wave"):
        res = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, NBX_PAIRCOUNT_SCHEME=scheme), capture_output=True, text=True,
                             timeout=120)
        assert res.returncode == 0, (scheme, res.stderr[-2000:])
        got = json.loads(res.stdout.strip().splitlines()[-1])
        for precision in ("32", "64"):
            check_counts(got[precision], 33)


# ---- the field ---------------------------------------------------------------------------------------------------------------------------
FIELD_CASES = [(name, family, precision) for name in ("field one column", "field one split", "field target") for family in ("box", "heavy")
               for precision in (32, 64)]
KREF_POINTS = {"acc": 256, "phi": 64}  # of the checked points: the first and last and every stride-th between


def field_sample(m, columns, every, count=1000):
    """All m points, or the first and last, both sides of every column seam and seeded random ones up to `count`."""
    if every:
        return np.arange(m)
    s = {0, m - 1}
    for c in range(1, columns):
        s.update((c * 512 - 1, c * 512))
    rng = np.random.default_rng([17, m])
    while len(s) < count:
        s.add(int(rng.integers(0, m)))
    return np.array(sorted(i for i in s if 0 <= i < m), dtype=np.int64)


def field_case(oracle, precision, m, n, family, every):
    """{"state", "points", "rows", "truth", "gate_acc", "gate_phi", ...}: the truth and the gates on the checked rows."""
    def make():
        state = FR.make_state(precision, n, family)
        points = FR.make_points(precision, state, m, family)
        rows = field_sample(m, FR.field_shape(m, n)[0], every)
        sub = tuple(p[rows] for p in points)
        tr = FR.truth_at(state, sub, precision)
        pick = lambda count: np.unique(np.linspace(0, len(rows) - 1, min(count, len(rows))).astype(np.int64))
        ia, ip = pick(KREF_POINTS["acc"]), pick(KREF_POINTS["phi"])
        part = lambda t, i: {"acc": tuple(v[i] for v in t["acc"]), "phi": tuple(v[i] for v in t["phi"])}
        kref_acc = float(FR.k_acc(FR.oracle_acc(oracle, state, tuple(p[ia] for p in sub)), part(tr, ia), precision).max())
        kref_phi = float(FR.k_phi(FR.phi_sequential(state, tuple(p[ip] for p in sub), precision), part(tr, ip), precision).max())
        return {"state": state, "points": points, "rows": rows, "truth": tr, "kref_acc": kref_acc, "kref_phi": kref_phi,
                "gate_acc": F.gate(kref_acc), "gate_phi": F.gate(kref_phi)}
    return cached(("field", precision, m, n, family), make)


@pytest.mark.parametrize("name,family,precision", FIELD_CASES, ids=["%s-%s-fp%d" % (n.replace(" ", "-"), f, p) for n, f, p in FIELD_CASES])
def test_the_field_of_a_context(nbx, oracle, name, family, precision):
    (m, n), shape = REGIMES[name][:2]
    case = field_case(oracle, precision, m, n, family, every=name != "field target")
    with nbx.Context(n, precision) as c:
        c.upload(case["state"])
        c.sync()
        t0 = time.perf_counter()
        r = c.field(*case["points"])
        seconds = time.perf_counter() - t0
        again = c.field(*case["points"])
        assert all(np.array_equal(bits(again[f]), bits(r[f])) for f in FR.KEYS)
    ka, kp = check_field({f: r[f][case["rows"]] for f in FR.KEYS}, case, precision)
    record(kernel="field", case="%s %s fp%d" % (name, family, precision), shape=shape, points_checked=len(case["rows"]), K_acc=ka, gate_acc=case["gate_acc"],
           K_phi=kp, gate_phi=case["gate_phi"], call_s=seconds)


@pytest.mark.parametrize("family", ["box", "heavy"])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_field_of_a_member(nbx, oracle, precision, family):
    (m, n), shape = REGIMES["field member fp%d" % precision][:2]
    case = field_case(oracle, precision, m, n, family, every=False)
    with nbx.Ensemble(n, 1, precision) as e:
        e.upload([case["state"]])
        r = e.field(*[p[None, :] for p in case["points"]])
    with nbx.Ragged((SMALL_MEMBERS[0], n), precision) as g:  # beside a member of one column, one tile
        g.upload([small_member(SMALL_MEMBERS[0], precision), case["state"]])
        rr = g.field(*[p[None, :] for p in case["points"]], first=1, count=1)
    assert all(np.array_equal(bits(rr[f]), bits(r[f])) for f in FR.KEYS)
    ka, kp = check_field({f: r[f][0][case["rows"]] for f in FR.KEYS}, case, precision)
    record(kernel="field", case="member %s fp%d" % (family, precision), shape=shape, points_checked=len(case["rows"]), K_acc=ka,
           gate_acc=case["gate_acc"], K_phi=kp, gate_phi=case["gate_phi"])


def own_sites_deviation(phi, k, precision):
    """(deviation in u of the sum of |terms|, gate): phi_i holds every body, the one at the point too (-G m / eps), so
    1/2 sum_i m phi_i is the lattice total less n G m / (2 eps).  Gate: a split's sum in T, the term floor, the finish's rounding."""
    hi, lo = L.potential(k, precision)
    gm = float(gm_as_uploaded(np.ones(1, dtype=NB.DTYPE[precision]))[0])
    self_terms = 0.5 * k ** 3 * gm / math.sqrt(EPS2)
    total = 0.5 * math.fsum(np.asarray(phi, dtype=np.float64).tolist())
    dev = abs((total + self_terms - hi) - lo) / (U[precision] * (abs(hi) + self_terms))
    return dev, 256.0 * shape_of(k)[3] + F.K_TERM + 1.0


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_field_at_the_lattices_own_sites_adds_up_to_the_closed_form(nbx, precision, perm):
    k = 33
    st = lattice(k, precision, perm)
    with nbx.Context(k ** 3, precision) as c:
        c.upload(st)
        phi = c.field(*[st[f] for f in NB.POS])["phi"]
    dev, gate = own_sites_deviation(phi, k, precision)
    record(kernel="field", case="lattice own sites %s" % case_name((k, precision, perm)), shape=shape_of(k), total_u=dev, gate_u=gate)
    assert dev <= gate, (dev, gate)


# ---- what the shapes reach ---------------------------------------------------------------------------------------------------------------
def test_every_kernel_family_meets_more_than_256_partial_rows():
    """The potential's, the timescale's and the pair counts' reduce walk splits x columns rows in strides of 256; neighbours and
    the field combine a body's or point's splits, at most 206 of them here.  From the shape functions, not from the device."""
    for k in CONTEXT_K + tuple(MEMBER_K.values()):
        columns, tiles, splits, per = P.diag_shape(k ** 3, k ** 3)
        assert (columns, tiles, splits, per) == FR.field_shape(k ** 3, k ** 3) == REGIMES["k%d" % k][1]
        assert columns * splits > 256, (k, columns, splits)  # potential, timescale, paircount: contexts and members of both precisions
    assert max(FR.field_shape(*REGIMES[name][0])[2] for name in REGIMES if name.startswith("field")) == 206
