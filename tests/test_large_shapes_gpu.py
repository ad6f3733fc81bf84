"""The pair-work analysis kernels -- the potential of nbx_diagnostics, nbx_timescale, nbx_field, nbx_neighbours, nbx_paircount,
nbx_binaries, the pair loop and update of nbx_tracers, and their ensemble and ragged forms -- at the launch shapes the other device modules never reach (they stop at n = 4099: nine
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

The velocity-reading kernels.  nbx_timescale and nbx_binaries stage a SECOND tile, the velocity records of the same j.  A lattice
at rest holds zero in every velocity record (but the planted body's), so a kernel that pairs a velocity with the wrong position --
record j + 1, the first split's tile in every split, a member's offset applied to one buffer alone, an index that wraps at 2^16 --
returns the same values there: tests/test_large_shapes_cpu.py shows that the comparison of tests/test_binaries_gpu.py on the 13^3
lattice at rest lets each of these through.  So the lattices also run in Hubble flow (lattice_ref.hubble: v = H x, H = 16 or 8,
every mass 1 / G): every velocity is exact, dv = H dx exactly and every pair value is a function of the squared lattice radius s.
timescale: the rates within 32 u / 128 u and min_r2 within 8 u of lattice_ref.hubble_timescale_expected, O(1) -- the approach rate
H^2 D^2 / (D^2 + eps^2) of the corner-to-corner pair stays below H^2, which a far mispairing exceeds.  binaries: e(s) grows with s,
so partner EQUALS the geometry's lowest-numbered face neighbour, energy is one bit pattern within binaries_ref.GATE u (A + B) of
e(1), and bound EQUALS the number of sites within s <= 3 (H = 16) or s <= 10 (H = 8), exact integers -- the nearest shell is 0.40 %
of A + B from e = 0 -- that change when a pair's velocity is another record's; bound=False returns the same partner and energy
bits and binaries_ref.identities holds.  At k = 33 and k = 81 (partner indices above 2^16, one split walking 2076 tiles), natural
and permuted; as an ensemble of two such lattices of DIFFERENT H and as ragged members among clouds of 5 and 8192 bodies, every
member also bit for bit a context of its state.  A cloud of 35 937 bodies (binaries_ref.cloud, its seed chosen on the CPU so that
no sampled row is ambiguous): binaries_ref.compare on 1000 rows -- seam_bodies', both sides of the probed column and split seams
among them -- against the row-sampled reference, and on EVERY body, in O(n), energy within the gate of the fp64 energy of the pair
(i, partner[i]) and energy[partner[i]] <= energy[i] + that window; the worst value goes to profiles/binaries_error.json.

The tracers.  tests/test_tracers_gpu.py stops at (n, m) = (4099, 513): the tracers' own partial rows [systems][tr_rows][m] have met
4 rows and 3 columns.  Here: (262 657, 300), one column and 206 rows; (32 769, 32 769), 65 x 15; (257, 524 289), 1025 columns, the
last of one tracer; two members with 65 537 tracers each.  Two steps, then one -- the second call starts on the other position
buffer -- then a kick, at dt = 0.01, bit for bit tracers_ref.round_trip / round_trip_kick on a twin, the bodies bit for bit plain
step's.  No tolerance is needed: nbx_field is held to field_ref.truth_at at exactly these shapes by this module.

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
module about a minute.  When the velocity-reading kernels and the tracers were added to it (nbx_binaries had met no reference above
n = 4097, no velocity tile anything but zeros at scale, the tracers no more than 4 partial rows): again nothing failed and no
kernel was changed.  timescale in Hubble flow: approach rate 1.1 u of 32 (fp32) and 2.0 u of 128 (fp64) at k = 81, 0.48 u and
1.0 u at k = 33, free-fall rate 0.64 u and 1.1 u, min_r2 0.12 u and exact; one call at k = 81 0.12 / 0.27 s.  binaries in Hubble
flow: partner and bound equal on every body of every case (bound up to 26 at H = 16, 146 at H = 8), energy 0.23 u (H = 16) and
0.26 u (H = 8) of 32 in fp32, exact in fp64; one call at k = 81 0.145 / 0.267 s, at k = 33 0.8 / 1.3 ms.  The cloud: every
sampled partner equal, every bound inside its bracket (895 of the 1000 brackets are one integer in fp32, all in fp64), energy
3.2 u of 32 (fp32) and 32.3 u of 128 (fp64) over all 35 937 bodies, a little above the 2.8 u and 30.0 u seen up to n = 4097 and
under the header's first-order 6.5 u and 55.5 u.  The members: the contexts' bits and the same deviations.  The tracers: every
bit equal; the two steps at (262 657, 300) take 0.044 / 0.079 s.  The additions take about six seconds.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import binaries_ref as BR
import field_ref as FR
import force_ref as F
import kick_ref as K
import lattice_ref as L
import neighbours_ref as NB
import paircount_ref as PC
import potential_ref as P
import tracers_ref as TR
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


# ---- the lattice in Hubble flow, and the cloud ------------------------------------------------------------------------------------------
HUBBLE_CASES = [(k, H, precision, perm) for k, H in ((33, 16.0), (33, 8.0), (81, 16.0)) for precision in (32, 64) for perm in (False, True)]
hubble_name = lambda c: "k%d-H%d-fp%d-%s" % (c[0], c[1], c[2], "permuted" if c[3] else "natural")
CLOUD_N = 35937
CLOUD_ROWS = 1000
TRACER_DT = 0.01  # tests/test_tracers_gpu.py's: no power of two, so a contracted a dt + w would show
# (n, m) of the tracer cases by the entry of REGIMES that is field_shape(m, n): the field's own extreme shapes
TRACER_SHAPES = {"field one column": (262657, 300), "field target": (32769, 32769), "field one split": (257, 524289)}
TRACER_MEMBER_M = 65537


def hubble(k, precision, perm, H):
    return cached(("hubble", k, precision, perm, H), lambda: L.hubble(k, precision, perm, H))


def hubble_binaries(k, H, precision, perm):
    return cached(("hubble binaries", k, H, precision, perm), lambda: L.hubble_binaries_expected(k, H, precision, perm))


def check_hubble_binaries(got, want, precision, rows=None):
    """partner and bound EQUAL lattice_ref.hubble_binaries_expected on every body (of `rows`, where `got` holds those bodies
    alone), energy one bit pattern within binaries_ref.GATE u (A + B) of e(1).  Returns the deviation of energy in u (A + B)."""
    pick = (lambda a: a) if rows is None else (lambda a: a[np.asarray(rows)])
    for f in ("partner", "bound"):
        g, w = np.asarray(got[f]), pick(want[f])
        assert g.shape == w.shape, (f, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (f, bad.size, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    e = np.asarray(got["energy"])
    assert (bits(e) == bits(e)[0]).all(), ("energy bits differ", np.flatnonzero(bits(e) != bits(e)[0])[:8].tolist())
    dev = abs(float(e[0]) - want["energy"]) / (U[precision] * want["mag"])
    assert dev <= BR.GATE[precision], dev
    return dev


def cloud(precision):
    return cached(("cloud", precision), lambda: BR.cloud(CLOUD_N, precision))


def cloud_rows():
    """The bodies of the cloud the row-sampled reference is asked for: seam_bodies' -- first, last, both sides of the probed column
    and split seams -- filled up to CLOUD_ROWS with seeded random ones.  binaries_ref.CLOUD_SEEDS[35937] was chosen for them."""
    return np.array(seam_bodies(CLOUD_N, FR.field_shape(CLOUD_N, CLOUD_N), count=CLOUD_ROWS), dtype=np.int64)


def check_cloud(got, state, precision, want, rows):
    """binaries_ref.compare on the sampled rows, and on ALL bodies in O(n): energy[i] within the gate of the fp64 energy of the
    pair (i, partner[i]), and energy[partner[i]] <= energy[i] + that pair's window (j's minimum is at most its pair with i).
    Returns the largest energy deviation in u (A + B)."""
    n = len(state["mass"])
    problems, worst = BR.compare(got, want, state, precision, rows=rows)
    assert not problems, problems
    p, e = np.asarray(got["partner"]), np.asarray(got["energy"], dtype=np.float64)
    i = np.arange(n)
    assert p.shape == (n,) and ((p >= 0) & (p < n) & (p != i)).all()
    e_own, mag = BR.pair_energy(state, i, p)
    dev = np.abs(e - e_own) / (U[precision] * mag)
    assert dev.max() <= BR.GATE[precision], (int(dev.argmax()), float(dev.max()))
    window = BR.GATE[precision] * U[precision] * mag
    late = np.flatnonzero(~(e[p] <= e + window))
    assert late.size == 0, (late.size, late[:8].tolist())
    return max(worst, float(dev.max()))


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


# ---- the velocity-reading kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONTEXT_CASES, ids=case_name)
def test_timescale_of_a_lattice_in_hubble_flow(nbx, case):
    k, precision, perm = case
    H = L.HUBBLE_H[0]
    with nbx.Context(k ** 3, precision) as c:
        c.upload(hubble(k, precision, perm, H))
        c.sync()
        t0 = time.perf_counter()
        got = c.timescale()
        seconds = time.perf_counter() - t0
        devs = check_timescale(got, L.hubble_timescale_expected(k, H, precision), precision)
        assert c.timescale() == got  # the same call twice: the same bits
        c.step(1, STEP_DT / 4, kenergy=False)
        moved = c.timescale()
        assert moved["steps_done"] == 1 and all(moved[f] != got[f] for f in ("approach_rate2", "freefall_rate2", "min_r2")) and c.timescale() == moved
    record(kernel="timescale, Hubble flow", case=case_name(case), shape=shape_of(k), H=H, worst_u=devs, rate_gate_u=RATE_GATE[precision],
           r2_gate_u=R2_GATE, call_s=seconds)


@pytest.mark.parametrize("case", HUBBLE_CASES, ids=hubble_name)
def test_binaries_of_a_lattice_in_hubble_flow(nbx, case):
    k, H, precision, perm = case
    want = hubble_binaries(k, H, precision, perm)
    with nbx.Context(k ** 3, precision) as c:
        c.upload(hubble(k, precision, perm, H))
        c.sync()
        t0 = time.perf_counter()
        got = c.binaries()
        seconds = time.perf_counter() - t0
        plain = c.binaries(bound=False)  # the kernels compiled without the count
    dev = check_hubble_binaries(got, want, precision)
    assert plain["bound"] is None and all(np.array_equal(bits(plain[f]), bits(got[f])) for f in ("partner", "energy"))
    assert not BR.identities(got), BR.identities(got)
    record(kernel="binaries, Hubble flow", case=hubble_name(case), shape=shape_of(k), H=H, energy_u=dev, gate_u=BR.GATE[precision],
           largest_bound=int(got["bound"].max()), call_s=seconds)


@pytest.mark.parametrize("precision", [32, 64])
def test_binaries_of_a_cloud_on_sampled_rows_and_on_every_body(nbx, precision):
    import test_binaries_gpu as BG  # the recorder of profiles/binaries_error.json
    st, rows = cloud(precision), cloud_rows()
    want = cached(("cloud reference", precision), lambda: BR.binaries(st, precision, rows=rows))
    assert BR.ambiguity(st, precision, rows=rows[:64]) == 0  # the seed's property, re-checked on a part (the CPU module checks all rows)
    with nbx.Context(CLOUD_N, precision) as c:
        c.upload(st)
        c.sync()
        t0 = time.perf_counter()
        got = c.binaries()
        seconds = time.perf_counter() - t0
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(c.binaries().values(), got.values()))
    worst = check_cloud(got, st, precision, want, rows)
    assert not BR.identities(got), BR.identities(got)
    sampled = got["bound"][rows]
    assert 0 < sampled.min() and sampled.max() < CLOUD_N - 1
    BG.note_worst(precision, worst, CLOUD_N, "cloud")
    record(kernel="binaries, cloud", case="fp%d" % precision, shape=shape_of(33), rows_checked=len(rows), energy_u=worst, gate_u=BR.GATE[precision],
           bound_exact_by_the_reference=int((want["bound_lo"] == want["bound_hi"]).sum()), call_s=seconds)


# ---- members -------------------------------------------------------------------------------------------------------------------------------
def velocity_context(nbx, state, precision):
    """(timescale, binaries) of a context of the state's size holding it."""
    with nbx.Context(len(state["mass"]), precision) as c:
        c.upload(state)
        return c.timescale(), c.binaries()


def same_binaries(a, b):
    return all(np.array_equal(bits(a[f]), bits(b[f])) for f in BR.KEYS)


def same_timescale(a, b):
    return all(a[f] == b[f] for f in ("approach_rate2", "freefall_rate2", "min_r2"))


@pytest.mark.parametrize("precision", [32, 64])
def test_velocity_reading_members_of_an_ensemble(nbx, precision):
    """Two lattices in Hubble flow of DIFFERENT H, so that a member that reads the other's velocities shows."""
    k = MEMBER_K[precision]
    n = k ** 3
    members = ((L.HUBBLE_H[0], False), (L.HUBBLE_H[1], True))
    states = [hubble(k, precision, perm, H) for H, perm in members]
    with nbx.Ensemble(n, 2, precision) as e:
        e.upload(states)
        ts, b = e.timescale(), e.binaries()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(e.binaries().values(), b.values()))
        plain = e.binaries(bound=False)
        assert plain["bound"] is None and all(np.array_equal(bits(plain[f]), bits(b[f])) for f in ("partner", "energy"))
        for m, (H, perm) in enumerate(members):
            got = {f: b[f][m] for f in BR.KEYS}
            tdev = check_timescale(ts[m], L.hubble_timescale_expected(k, H, precision), precision)
            dev = check_hubble_binaries(got, hubble_binaries(k, H, precision, perm), precision)
            assert not BR.identities(got)
            cts, cb = velocity_context(nbx, states[m], precision)
            assert same_timescale(ts[m], cts) and same_binaries(got, cb), m
            record(kernel="ensemble member, Hubble flow", case=hubble_name((k, H, precision, perm)), shape=shape_of(k), timescale_u=tdev, energy_u=dev,
                   gate_u=BR.GATE[precision])
        one = e.binaries(first=1, count=1)  # a launch that starts at the second member
        assert all(np.array_equal(bits(one[f][0]), bits(b[f][1])) for f in BR.KEYS)


def small_cloud(n, precision):
    return cached(("small cloud", n, precision), lambda: BR.cloud(n, precision, seed=100 + n % 97))


@pytest.mark.parametrize("precision", [32, 64])
def test_velocity_reading_members_of_a_ragged_ensemble_among_small_ones(nbx, precision):
    k = MEMBER_K[precision]
    n = k ** 3
    sizes = (SMALL_MEMBERS[0], n, SMALL_MEMBERS[1], n)
    members = {1: (L.HUBBLE_H[0], False), 3: (L.HUBBLE_H[1], True)}
    states = [small_cloud(sizes[0], precision), hubble(k, precision, *members[1][::-1]), small_cloud(sizes[2], precision),
              hubble(k, precision, *members[3][::-1])]
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        ts, b = r.timescale(), r.binaries()
        assert all(same_binaries(x, y) for x, y in zip(r.binaries(), b)) and all(same_timescale(x, y) for x, y in zip(r.timescale(), ts))
        for m in range(4):  # every member, the small ones that leave the grid early included, has the bits of a context of its size
            cts, cb = velocity_context(nbx, states[m], precision)
            assert same_timescale(ts[m], cts) and same_binaries(b[m], cb), m
        for m, (H, perm) in members.items():
            tdev = check_timescale(ts[m], L.hubble_timescale_expected(k, H, precision), precision)
            dev = check_hubble_binaries(b[m], hubble_binaries(k, H, precision, perm), precision)
            assert not BR.identities(b[m])
            record(kernel="ragged member, Hubble flow", case=hubble_name((k, H, precision, perm)), shape=shape_of(k), timescale_u=tdev, energy_u=dev,
                   gate_u=BR.GATE[precision])
        assert same_binaries(r.binaries(first=3, count=1)[0], b[3]) and same_binaries(r.binaries(first=0, count=1)[0], b[0])


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


# ---- the tracers at the field's extreme shapes ---------------------------------------------------------------------------------------------
def tracer_case(precision, n, m, seed=0):
    def make():
        state = K.make_state(9100 + 7 * seed + n % 1000, n, NB.DTYPE[precision])
        return state, TR.make_tracers(precision, state, m, seed=seed)
    return cached(("tracers", precision, n, m, seed), make)


def split_tracers(tr):
    return [tr[f] for f in TR.POS], [tr[f] for f in TR.VEL]


def stacked(dicts):
    return {f: np.ascontiguousarray(np.stack([d[f] for d in dicts])) for f in TR.KEYS}


def bodies_same(a, b):
    """Two downloads of one kind of object: a dict of arrays, or a list of them."""
    return all(TR.same(x, y) for x, y in zip(a, b)) if isinstance(a, list) else TR.same(a, b)


def run_tracers(o, twin, state, tr, precision):
    """Two steps, then one -- the second call starts on the other position buffer -- then one kick, on `o`, against the round
    trip on `twin`, an object of the same kind that holds the same bodies: nbx_field at the host's tracer positions, the update
    in numpy, one plain step.  Bit for bit, the bodies included.  Returns the seconds of the first tracers_step call."""
    h = 0.37 * TRACER_DT
    for obj in (o, twin):
        obj.upload(state)
    want, ke_want = TR.round_trip(twin, tr, precision, TRACER_DT, 3)
    o.tracers_upload(*split_tracers(tr))
    o.sync()
    t0 = time.perf_counter()
    o.tracers_step(2, TRACER_DT, kenergy=False)
    o.sync()
    seconds = time.perf_counter() - t0
    ke = o.tracers_step(1, TRACER_DT)
    got = o.tracers_download()
    assert TR.same(got, want) and not TR.same(want, tr)
    assert bodies_same(o.download(), twin.download()) and np.array_equal(ke, ke_want)  # the bodies are plain step's
    kicked = TR.round_trip_kick(twin, got, precision, h)
    o.tracers_kick(h)
    after = o.tracers_download()
    assert TR.same(after, kicked) and not TR.same(after, got)
    assert all(np.asarray(after[f]).tobytes() == np.asarray(got[f]).tobytes() for f in TR.POS)
    return seconds


@pytest.mark.parametrize("name", list(TRACER_SHAPES), ids=[n.replace(" ", "-") for n in TRACER_SHAPES])
@pytest.mark.parametrize("precision", [32, 64])
def test_tracers_of_a_context_at_the_fields_extreme_shapes(nbx, precision, name):
    """No tolerance: nbx_field is held to field_ref.truth_at at exactly these shapes (test_the_field_of_a_context), and the
    tracers are held to nbx_field's bits -- what is new here is the tracers' own partial-row buffer [tr_rows][tr_m], up to 206 rows
    and 1025 columns where tests/test_tracers_gpu.py reaches 4 and 3, and the update launch that adds the rows in place."""
    n, m = TRACER_SHAPES[name]
    assert REGIMES[name][0] == (m, n)
    state, tr = tracer_case(precision, n, m)
    with nbx.Context(n, precision) as c, nbx.Context(n, precision) as twin:
        seconds = run_tracers(c, twin, state, tr, precision)
        assert c.tracers_count() == m and c.stats()["steps_done"] == 3
    record(kernel="tracers", case="%s fp%d" % (name, precision), shape=REGIMES[name][1], n=n, m=m, two_steps_s=seconds)


@pytest.mark.parametrize("precision", [32, 64])
def test_tracers_of_two_members_at_65537_tracers_each(nbx, precision):
    """As above for an ensemble of two members of the largest lattice size a member holds, 2 x 65 537 tracers: the twin is an
    ensemble too, and nbx_ensemble_field is held to the truth at this shape by test_the_field_of_a_member."""
    name = "field member fp%d" % precision
    (m, n), shape = REGIMES[name][:2]
    assert m == TRACER_MEMBER_M and n == MEMBER_K[precision] ** 3 and 2 * m <= 2 ** 22
    cases = [tracer_case(precision, n, m, seed=1 + j) for j in range(2)]
    states, tr = [c[0] for c in cases], stacked([c[1] for c in cases])
    with nbx.Ensemble(n, 2, precision) as e, nbx.Ensemble(n, 2, precision) as twin:
        seconds = run_tracers(e, twin, states, tr, precision)
        got = e.tracers_download()
        assert all(got[f].shape == (2, m) for f in TR.KEYS) and not TR.same({f: got[f][0] for f in TR.KEYS}, {f: got[f][1] for f in TR.KEYS})
    record(kernel="tracers", case="two members fp%d" % precision, shape=shape, n=n, m=m, two_steps_s=seconds)


# ---- what the shapes reach ---------------------------------------------------------------------------------------------------------------
def test_every_kernel_family_meets_more_than_256_partial_rows():
    """The potential's, the timescale's and the pair counts' reduce walk splits x columns rows in strides of 256; neighbours and
    the field combine a body's or point's splits, at most 206 of them here.  From the shape functions, not from the device."""
    for k in CONTEXT_K + tuple(MEMBER_K.values()):
        columns, tiles, splits, per = P.diag_shape(k ** 3, k ** 3)
        assert (columns, tiles, splits, per) == FR.field_shape(k ** 3, k ** 3) == REGIMES["k%d" % k][1]
        assert columns * splits > 256, (k, columns, splits)  # potential, timescale, paircount: contexts and members of both precisions
    assert max(FR.field_shape(*REGIMES[name][0])[2] for name in REGIMES if name.startswith("field")) == 206
    # nbx_binaries' finish is of the second kind -- one thread per body walks that body's split rows in ascending order
    # (csrc/nbx_binaries_kernels.hpp: bound_finish_kernel), no stride of 256 --: 15 rows in the target regime, one at k = 81; the
    # tracers' update launch adds a tracer's tr_rows partial rows the same way, 206 of them at (n, m) = (262 657, 300)
    assert [FR.field_shape(k ** 3, k ** 3)[2] for k in CONTEXT_K] == [15, 1] and FR.field_shape(CLOUD_N, CLOUD_N)[2] == 15
    assert max(FR.field_shape(m, n)[2] for n, m in TRACER_SHAPES.values()) == 206
