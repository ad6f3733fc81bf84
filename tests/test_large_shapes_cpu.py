"""What tests/test_large_shapes_gpu.py relies on, checked without a device: the closed forms of tests/lattice_ref.py against brute
force (k = 5, 7) and against the O(n^2) references of the sibling modules (k = 13, permuted); the regime table against the
headers' shape rules, through tests/field_shape_driver.cpp, tests/diag_shape_driver.cpp and the planner's
tests/ragged_diag_plan_driver.cpp; and the sensitivity of the GPU module's comparisons: at k = 17 (4913 bodies) every fault the
restatements of neighbours_ref, paircount_ref, field_ref and potential_ref can plant, and a finish that adds only its first
rows, must be rejected by the very functions the GPU module applies to the device's values.

The lattice in Hubble flow (lattice_ref.hubble), which the GPU module runs nbx_timescale and nbx_binaries on: its closed forms
against binaries_ref.binaries and timescale_ref.timescale by brute force at k = 5 and 13; that no shell of pairs lies inside the
gate's window around e = 0; that binaries_ref.ambiguity flags only the exact ties of the face neighbours there; the row-sampled
reference (rows=) against the full one, and the property binaries_ref.CLOUD_SEEDS[35937] was chosen for; and four ways of pairing
the velocity tile with the wrong position record (binaries_ref.VELOCITY_FAULTS), planted in binaries_ref.restate and in
lattice_ref.restate_timescale: rejected by the Hubble comparisons at k = 17 (the wrap at 65 536 at k = 41, on a few rows), and NOT
seen by the comparison tests/test_binaries_gpu.py applies to the 13^3 lattice at rest -- the gap the Hubble shapes close.

One entry of potential_ref.FAULTS, "velm read at the global index", is no fault of an unsliced launch -- with i_begin = 0 the
local and the global index are one -- and the large shapes are unsliced: the test asserts that it changes no bit there
(tests/test_potential_probe_cpu.py plants it on a slice)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import binaries_ref as BR
import energy_ref as E
import field_ref as FR
import lattice_ref as L
import neighbours_ref as NB
import paircount_ref as PC
import potential_ref as P
import test_large_shapes_gpu as G
import timescale_ref as TS
from conftest import ROOT

CSRC = os.path.join(ROOT, "nbody-demo-2023_amd", "csrc")
K_FAULT = 17


# ---- the closed forms ------------------------------------------------------------------------------------------------------------------
def _lattice_d2(k):
    """The squared lattice distances of all ordered pairs of the natural lattice, an integer matrix."""
    s = np.arange(k ** 3)
    c = np.stack([s // (k * k), (s // k) % k, s % k], axis=1)
    return ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)


@pytest.mark.parametrize("k", [5, 7])
def test_closed_forms_against_brute_force(k):
    n = k ** 3
    d2 = _lattice_d2(k)
    off = ~np.eye(n, dtype=bool)
    squared = G.SQUARED + [0.5, 1.0, 2.0, 3 * (k - 1) ** 2 - 0.5, 3 * (k - 1) ** 2]
    assert L.pair_counts(k, squared) == [int(((d2 <= m) & off).sum()) // 2 for m in squared]
    assert L.pair_counts(k, [m + 0.5 for m in range(1, 7)]) == PC.lattice_counts(k, 6).tolist()
    assert L.pair_counts(k, [1.5]) == [PC.lattice_face_pairs(k)] and L.pair_counts(k, [math.inf]) == [n * (n - 1) // 2]
    w = L.shell_weights(k)
    assert w.tolist() == np.bincount(d2.ravel(), minlength=len(w)).tolist()
    for precision in (32, 64):
        gm = float(E.gm_as_uploaded(np.ones(1, dtype=NB.DTYPE[precision]))[0])
        inv = np.where(off, 1.0 / np.sqrt(d2.astype(np.longdouble) / 64 + np.longdouble(E.EPS2)), 0)
        brute = -0.5 * gm * float(inv.sum())
        hi, lo = L.potential(k, precision)
        assert abs(brute - hi - lo) <= 1e-15 * abs(hi) and abs(lo) <= 2.0 ** -53 * abs(hi)
        for perm in (False, True):
            st = L.state(k, precision, perm)
            assert (st["mass"] == 1.0).all()
            assert abs(E.potential([st[f] for f in NB.POS], st["mass"]) - hi) <= 1e-13 * abs(hi)
            truth = P.truth_total(st, precision)
            assert abs((truth[0] - hi) + (truth[1] - lo)) <= (1e-15 if precision == 32 else 1e-18) * abs(hi)  # truth_total sums fp32 states in fp64


@pytest.mark.parametrize("k,perm", [(5, False), (7, True), (13, True)])
def test_timescale_expected_is_the_restatements_search(k, perm):
    n = k ** 3
    for precision in (32, 64):
        rest = L.state(k, precision, perm, at_rest=True)
        back = TS.timescale(rest)
        assert {f: back[f] for f in TS.KEYS} == pytest.approx(L.timescale_background(precision), rel=1e-15)
        for body in sorted({0, n - 1, n // 2, 511 % n, 512 % n}):
            st = L.plant(rest, body)
            moved = [f for f in rest if not np.array_equal(st[f], rest[f])]
            assert sorted(moved) == ["mass", "pos_x", "vel_y"] and abs(float(st["pos_x"][body]) - float(rest["pos_x"][body])) == L.SHIFT
            assert float(st["pos_x"][body]) * 16 == round(float(st["pos_x"][body]) * 16)  # still exact
            want = TS.timescale(st)
            got = L.timescale_expected(k, body, precision, perm)
            for f in TS.KEYS:
                assert abs(got[f] - want[f]) <= 4 * 2.0 ** -53 * want[f], (k, precision, body, f)
            assert got["min_r2"] == 1.0 / 256 + E.EPS2 and got["approach_rate2"] == TS.PLANT_SPEED ** 2 / got["min_r2"]


def test_at_k_13_permuted_the_closed_forms_are_the_sibling_references():
    k, perm = NB.LATTICE_K, True
    for precision in (32, 64):
        st = L.state(k, precision, perm)
        index, faces = NB.lattice_expected(k, perm)
        for radius in (NB.LATTICE_RADIUS, NB.LATTICE_TIE_RADIUS):
            ref = NB.neighbours(st, radius, precision)
            assert np.array_equal(ref["index"], index) and np.array_equal(ref["within"], faces) and (ref["r2"] == L.FACE_R2).all()
        assert PC.counts(st, G.RADII, precision).tolist() == L.pair_counts(k, G.SQUARED)
        lo, hi = PC.bracket(st, G.RADII, precision)
        assert np.array_equal(lo, hi)  # mid-shell radii: no pair inside the 8 u window, the device is held to the exact count
        want = L.potential(k, precision)
        assert abs(E.potential([st[f] for f in NB.POS], st["mass"]) - want[0]) <= 1e-13 * abs(want[0])


def test_the_heavy_body_truth_is_the_direct_sum():
    k = 7
    bodies = [0, 171, k ** 3 - 1]
    for precision in (32, 64):
        for perm in (False, True):
            hi, lo = G.heavy_lattice_truth(k, precision, perm, bodies)
            for a, b in enumerate(bodies):
                want = P.truth_total(G.heavy_lattice_state(k, precision, perm, b), precision)
                assert abs((hi[a] - want[0]) + (lo[a] - want[1])) <= (1e-15 if precision == 32 else 1e-17) * abs(want[0]), (precision, perm, b)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_fields_restatement_at_the_lattices_own_sites_adds_up_to_the_closed_form(precision):
    for k in (7, 13):
        st = L.state(k, precision, True)
        phi = FR.restate(st, tuple(st[f] for f in NB.POS), precision)["phi"]
        dev, gate = G.own_sites_deviation(phi, k, precision)
        print("fp%d k = %d: %.2f u of %.0f" % (precision, k, dev, gate))
        assert dev <= gate and gate == 256.0 * FR.field_shape(k ** 3, k ** 3)[3] + 17.0
        assert G.own_sites_deviation(-phi, k, precision)[0] > gate  # the sign is seen


@pytest.mark.parametrize("precision", [32, 64])
def test_the_direct_field_truth_is_the_augmented_one(precision):
    for n, m, family in ((257, 513, "heavy"), (2049, 1025, "box"), (300, 2049, "origin")):
        state = FR.make_state(precision, n, family)
        points = FR.make_points(precision, state, m, family)
        a, b = FR.truth(state, points, precision), FR.truth_at(state, points, precision)
        tol = 1e-13 if precision == 32 else 2.0 ** -58  # two summation orders in fp64 / long double; in u_T: 2e-6 and 0.03
        scale = a["acc"][2]
        assert (np.abs((a["acc"][0] - b["acc"][0]) + (a["acc"][1] - b["acc"][1])).max(axis=1) <= tol * scale).all()
        assert (np.abs(a["acc"][2] - b["acc"][2]) <= 1e-12 * scale).all()
        assert (np.abs((a["phi"][0] - b["phi"][0]) + (a["phi"][1] - b["phi"][1])) <= tol * np.abs(a["phi"][0])).all()


# ---- the lattice in Hubble flow ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, NB.LATTICE_K])
@pytest.mark.parametrize("precision", [32, 64])
def test_hubble_closed_forms_against_brute_force(k, precision):
    """fp64 against fp64 with the same formula: 1e-13 relative, the module's figure for such comparisons; partner and bound equal."""
    for perm in (False, True):
        for H in L.HUBBLE_H:
            st = L.hubble(k, precision, perm, H)
            for p, w in zip(NB.POS, L.VEL):
                assert np.array_equal(st[w].astype(np.float64), H * st[p].astype(np.float64))
            assert abs(L.hubble_gm(precision) - 1.0) <= 2.0 ** -23 and (st["mass"] == st["mass"][0]).all()
            ref = BR.binaries(st, precision)
            want = L.hubble_binaries_expected(k, H, precision, perm)
            assert np.array_equal(ref["partner"], want["partner"]) and np.array_equal(ref["bound"], want["bound"]), (perm, H)
            assert np.array_equal(ref["bound_lo"], ref["bound_hi"])  # no pair inside the window: the device is held to the exact count
            assert (np.abs(ref["energy"] - want["energy"]) <= 1e-13 * abs(want["energy"])).all() and want["energy"] < 0
            assert (np.abs(ref["mag"] - want["mag"]) <= 1e-13 * want["mag"]).all()
            ts, tw = TS.timescale(st), L.hubble_timescale_expected(k, H, precision)
            for f in TS.KEYS:
                assert abs(ts[f] - tw[f]) <= 1e-13 * tw[f], (f, perm, H)
            assert tw["approach_rate2"] < H * H  # the supremum of every true pair
            assert L.restate_timescale(st) == {f: ts[f] for f in TS.KEYS}
            assert G.check_hubble_binaries(BR.restate(st, precision), want, precision) <= 1e-3


def test_no_shell_lies_inside_the_gate_window_around_zero_energy():
    """(s_max, the relative margin |e| / (A + B) of the nearest shell) for every H: 3, 10 and 25, margins of 0.40 %, 0.43 % and
    1.1 % -- four orders of magnitude outside 32 u (fp32); at H = 16 the bound sites are the 3 x 3 x 3 block about the body."""
    table = {16.0: (3, 0.0040), 8.0: (10, 0.0043), 4.0: (25, 0.0112)}
    assert set(L.HUBBLE_H) <= set(table)
    for H, (s_max, margin) in table.items():
        for precision in (32, 64):
            for k in G.CONTEXT_K + tuple(G.MEMBER_K.values()) + (5, NB.LATTICE_K, K_FAULT):
                got = L.hubble_shell(k, H, precision)
                assert got[0] == s_max and abs(got[1] - margin) <= 1e-4, (H, precision, k, got)
                assert got[1] > 1000 * BR.GATE[precision] * BR.U[precision]
    for k, perm in ((5, True), (33, False)):
        site = NB.lattice_order(k, perm)
        a = [np.where((c == 0) | (c == k - 1), 2, 3) for c in (site // (k * k), (site // k) % k, site % k)]
        assert np.array_equal(L.hubble_binaries_expected(k, 16.0, 32, perm)["bound"], a[0] * a[1] * a[2] - 1)


@pytest.mark.parametrize("precision", [32, 64])
def test_ambiguity_on_the_hubble_lattice_flags_only_exact_ties(precision):
    """Every body has three or more face neighbours at ONE energy, so binaries_ref.ambiguity flags every body -- which is why the
    partner is taken from the geometry there --, and nothing but those ties: the next shell's window ends far above e(1)'s."""
    k = 5
    g = BR.GATE[precision] * BR.U[precision]
    for H in L.HUBBLE_H:
        st = L.hubble(k, precision, True, H)
        assert BR.ambiguity(st, precision) == k ** 3 == BR.ambiguity(st, precision, rows=np.arange(k ** 3))
        e, mag = L.hubble_energy(np.array([1.0, 2.0]), H, precision)
        assert e[1] - g * mag[1] > e[0] + g * mag[0] + 1.0  # the edge neighbours' window ends more than 1 above the face neighbours'
        x = [st[f].astype(np.float64) for f in NB.POS]
        d2 = sum((c[:, None] - c[None, :]) ** 2 for c in x)
        faces = NB.lattice_expected(k, True)[1]
        assert np.array_equal((d2 == 1.0 / 64).sum(axis=1), faces) and faces.min() >= 3  # the ties: three to six partners at e(1)
        assert len(set(BR.binaries(st, precision)["energy"].tolist())) == 1


def test_the_row_sampled_reference_is_the_full_one_on_those_rows():
    n = 2049
    rows = np.array([0, 5, 511, 512, 1279, 1280, 2048, 7])
    for precision in (32, 64):
        st = BR.cloud(n, precision)
        full, part = BR.binaries(st, precision), BR.binaries(st, precision, rows=rows)
        assert all(np.array_equal(part[f], full[f][rows]) for f in full)
        assert BR.ambiguity(st, precision, rows=rows) == 0
        rs, rp = BR.restate(st, precision), BR.restate(st, precision, rows=rows)
        assert all(np.array_equal(rp[f], rs[f][rows]) for f in rs)
        assert not BR.compare(rs, part, st, precision, rows=rows)[0] and not BR.compare(rs, full, st, precision)[0]
        for fault in ("self not masked", "a split row dropped", "m_j alone instead of m_i + m_j", "velocity of record j + 1 read for record j"):
            assert BR.compare(BR.restate(st, precision, fault=fault), part, st, precision, rows=rows)[0], fault


@pytest.mark.parametrize("precision", [32, 64])
def test_the_cloud_of_35937_has_no_ambiguous_sampled_row(precision):
    """What binaries_ref.CLOUD_SEEDS[35937] was chosen for, from the reference alone: no sampled row ambiguous, none bound to
    nobody or to everybody, so the device is held to partner EQUAL on every sampled row."""
    n = G.CLOUD_N
    rows = G.cloud_rows()
    shape = FR.field_shape(n, n)
    assert shape == G.REGIMES["k33"][1] and len(rows) == G.CLOUD_ROWS == len(set(rows.tolist())) and BR.CLOUD_SEEDS[n] == 100 + n % 97
    columns, tiles, splits, per = shape
    seams = {0, n - 1, 511, 512, 255, 256, (columns - 1) * 512 - 1, (columns - 1) * 512, per * 256 - 1, per * 256,
             (splits - 1) * per * 256 - 1, (splits - 1) * per * 256, (splits // 2) * per * 256 - 1, (splits // 2) * per * 256}
    assert seams <= set(rows.tolist())  # both sides of every probed column and split seam
    st = BR.cloud(n, precision)
    assert BR.ambiguity(st, precision, rows=rows) == 0
    ref = BR.binaries(st, precision, rows=rows)
    assert 0 < ref["bound"].min() and ref["bound"].max() < n - 1
    assert ((ref["partner"] >= 0) & (ref["partner"] < n) & (ref["partner"] != rows)).all()


# ---- the regime table ------------------------------------------------------------------------------------------------------------------
def _build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
    return exe


def test_the_regime_table_is_the_headers(tmp_path):
    names = sorted(G.REGIMES)
    args = [str(v) for name in names for v in G.REGIMES[name][0]]
    field = subprocess.run([_build(tmp_path, "field_shape_driver")] + args, capture_output=True, text=True, check=True).stdout.splitlines()[:-1]
    diag = subprocess.run([_build(tmp_path, "diag_shape_driver")] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    for name, fl, dl in zip(names, field, diag):
        (m, n), shape, last_split, last_tile = G.REGIMES[name]
        assert tuple(int(v) for v in fl.split()) == (m, n) + shape == (m, n) + FR.field_shape(m, n), name
        assert tuple(int(v) for v in dl.split()) == (m, n) + shape == (m, n) + P.diag_shape(m, n), name  # one rule in two headers
        columns, tiles, splits, per = shape
        assert tiles - (splits - 1) * per == last_split and n - (tiles - 1) * 256 == last_tile, name
    shape = lambda name: G.REGIMES[name][1]
    # the target regime: splits aimed at 1024 workgroups, more than four tiles each
    for name in ("k33", "field target"):
        columns, tiles, splits, per = shape(name)
        assert -(-1024 // columns) < tiles // 4 and per == -(-tiles // -(-1024 // columns)) and per > 4, name
    # the min-tiles regime at its upper end: the members
    for name in ("k25", "k23"):
        columns, tiles, splits, per = shape(name)
        assert tiles // 4 < -(-1024 // columns) and per == -(-tiles // (tiles // 4)), name
    # one split under 1024 or more columns; one column under hundreds of splits
    assert shape("k81")[0] >= 1024 and shape("k81")[2] == 1 and shape("field one split")[0] >= 1024 and shape("field one split")[2] == 1
    assert shape("field one column")[0] == 1 and shape("field one column")[2] == 206
    assert 524289 - 1024 * 512 == 1  # the last column of "field one split" holds one point
    # the members' shapes again, through the planner of the batch objects
    exe = _build(tmp_path, "ragged_diag_plan_driver")
    for precision in (32, 64):
        k = G.MEMBER_K[precision]
        sizes = (G.SMALL_MEMBERS[0], k ** 3, G.SMALL_MEMBERS[1], k ** 3)
        plan = json.loads(subprocess.run([exe, "plan"], input="%d %d %s\n" % (precision, len(sizes), " ".join(map(str, sizes))), capture_output=True,
                                         text=True, check=True).stdout)
        assert "error" not in plan, plan
        assert [tuple(s[:4]) for s in plan["shape"]] == [P.diag_shape(n, n) for n in sizes] and tuple(plan["shape"][1][:4]) == shape("k%d" % k)
        assert plan["shape"][1][4] > 256 and plan["shape"][0][4] == 1  # rows: the lattice against the member of five bodies
    assert 25 ** 3 <= 16383 < 26 ** 3 and 23 ** 3 <= 12288 < 24 ** 3  # the largest lattices a member holds
    # the velocity-reading kernels and the tracers add no shape of their own: the Hubble lattices are k33, k81, k25 and k23, the
    # cloud is k33's size, and the tracers' (n, m) are the field's (m, n), rows of the table above
    assert G.CLOUD_N == G.REGIMES["k33"][0][0] and {c[0] for c in G.HUBBLE_CASES} == set(G.CONTEXT_K)
    for name, (n, m) in G.TRACER_SHAPES.items():
        assert G.REGIMES[name][0] == (m, n), name
    assert all(G.REGIMES["field member fp%d" % p][0] == (G.TRACER_MEMBER_M, G.MEMBER_K[p] ** 3) for p in (32, 64)) and 2 * G.TRACER_MEMBER_M <= 2 ** 22
    assert sorted(shape(name)[2] for name in G.TRACER_SHAPES) == [1, 15, 206] and shape("field one split")[0] == 1025  # tr_rows; columns
    G.test_every_kernel_family_meets_more_than_256_partial_rows()


def test_the_seams_are_among_the_probed_bodies():
    for k in G.CONTEXT_K:
        n, shape = k ** 3, G.shape_of(k)
        bodies = G.seam_bodies(n, shape)
        assert {0, n - 1, 511, 512, (shape[0] - 1) * 512 - 1, (shape[0] - 1) * 512} <= set(bodies) and len(bodies) >= 24
        sites = G.timescale_sites(n, shape)
        assert len(set(sites)) == 6 and all(0 <= s < n for s in sites) and sites[4] + 1 == sites[5] and sites[5] % 256 == 0
        if shape[2] > 1:
            assert shape[3] * 256 in bodies and sites[5] == shape[3] * 256
    rows = G.field_sample(32769, 65, every=False)
    assert {0, 32768, 511, 512, 64 * 512 - 1, 64 * 512} <= set(rows.tolist()) and 1000 <= len(rows) <= 1130
    assert len(G.field_sample(300, 1, every=True)) == 300


# ---- sensitivity: planted faults against the GPU module's comparisons --------------------------------------------------------------------
def rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("precision", [32, 64])
def test_every_neighbours_fault_is_rejected(precision):
    k = K_FAULT
    for perm in (False, True):
        st = L.state(k, precision, perm)
        both = lambda **kw: (NB.restate(st, NB.LATTICE_RADIUS, precision, **kw), NB.restate(st, NB.LATTICE_TIE_RADIUS, precision, **kw))
        assert G.check_neighbours(*both(), k, perm, precision) == 0.0
        for fault in NB.FAULTS if not perm else ("ties to the highest j", "finish takes the last split on ties", "padding record not masked"):
            assert rejected(G.check_neighbours, *both(fault=fault), k, perm, precision), (perm, fault)


def test_every_paircount_fault_is_rejected():
    """fp32 states: the lattice's coordinates are exact in both precisions and the restatement widens them, so the counts are the same."""
    k, precision = K_FAULT, 32
    st = L.state(k, precision, True)
    assert FR.field_shape(k ** 3, k ** 3) == (10, 20, 5, 4)
    assert G.check_counts(PC.restate(st, G.RADII, precision), k) == k ** 3 * (k ** 3 - 1) // 2
    G.check_counts(PC.restate(st, G.RADII[:19], precision), k, G.SQUARED[:19])
    G.check_counts(PC.restate(st, [NB.LATTICE_TIE_RADIUS], precision), k, [1.0])
    for fault in PC.FAULTS:
        if fault == "< instead of <=":  # mid-shell radii do not see it: the tie radius, whose h2 is the face neighbours' r2 bit for bit
            assert rejected(G.check_counts, PC.restate(st, [NB.LATTICE_TIE_RADIUS], precision, fault=fault), k, [1.0]), fault
        elif fault == "unused slot counted":  # twenty radii fill their last pass: the nineteen-radius call holds the unused slot
            assert rejected(G.check_counts, PC.restate(st, G.RADII[:19], precision, fault=fault), k, G.SQUARED[:19]), fault
        else:
            assert rejected(G.check_counts, PC.restate(st, G.RADII, precision, fault=fault), k), fault
    # the large shapes' own: a finish that stops after the first rows (32 of 50 here, 256 of 1065 at k = 33)
    assert rejected(G.check_counts, PC.restate(st, G.RADII, precision, finish_rows=32), k)
    assert not rejected(G.check_counts, PC.restate(st, G.RADII, precision, finish_rows=50), k)


WRAP_K = 41  # 68 921 bodies: the smallest lattice that has a record behind 65 536


def wrap_rows(n):
    return np.array([0, 1, 4095, 4096, BR.VELOCITY_WRAP - 1, BR.VELOCITY_WRAP, BR.VELOCITY_WRAP + 1, n - 1])


@pytest.mark.parametrize("precision", [32, 64])
def test_every_velocity_pairing_fault_is_rejected_in_hubble_flow_and_not_at_rest(precision):
    """The four ways of pairing the velocity tile with the wrong position record: the comparisons the GPU module applies to a
    lattice in Hubble flow reject each, in nbx_binaries' structure and in nbx_timescale's; the comparison of
    tests/test_binaries_gpu.py on the lattice at rest, all there was above n = 4097, lets every one of them through."""
    k = K_FAULT
    assert FR.field_shape(k ** 3, k ** 3) == P.diag_shape(k ** 3, k ** 3) == (10, 20, 5, 4)
    small = [f for f in BR.VELOCITY_FAULTS if f != "velocity index wraps at 65 536"]
    for perm, H, kernels in ((False, 16.0, "both"), (True, 8.0, "binaries"), (True, 16.0, "timescale")):  # the timescale cases all have H = 16
        st = L.hubble(k, precision, perm, H)
        other = L.hubble(k, precision, not perm, L.HUBBLE_H[1] if H == L.HUBBLE_H[0] else L.HUBBLE_H[0])  # the member before it
        want = L.hubble_binaries_expected(k, H, precision, perm)
        tw = L.hubble_timescale_expected(k, H, precision)
        if kernels != "timescale":
            G.check_hubble_binaries(BR.restate(st, precision), want, precision)
        if kernels != "binaries":
            G.check_timescale(L.restate_timescale(st), tw, precision)
        for fault in small:
            if kernels != "timescale":
                got = BR.restate(st, precision, fault=fault, member0=other)
                assert rejected(G.check_hubble_binaries, got, want, precision), (perm, H, fault)
            if kernels != "binaries":
                ts = L.restate_timescale(st, fault=fault, member0=other)
                assert rejected(G.check_timescale, ts, tw, precision), (perm, fault)
                assert ts["approach_rate2"] > H * H  # above the supremum of every true pair
    # the wrap shows behind 65 536 records alone: k = 41 on a few rows, each against all j
    n = WRAP_K ** 3
    rows = wrap_rows(n)
    fault = "velocity index wraps at 65 536"
    for perm in (False, True):
        st = L.hubble(WRAP_K, precision, perm, 16.0)
        want = L.hubble_binaries_expected(WRAP_K, 16.0, precision, perm)
        G.check_hubble_binaries(BR.restate(st, precision, rows=rows), want, precision, rows=rows)
        assert rejected(G.check_hubble_binaries, BR.restate(st, precision, rows=rows, fault=fault), want, precision, rows)
        tw = L.hubble_timescale_expected(WRAP_K, 16.0, precision)
        corners = np.flatnonzero(np.isin(NB.lattice_order(WRAP_K, perm), [0, n - 1]))  # the two bodies of the extreme pair
        G.check_timescale(L.restate_timescale(st, rows=corners), tw, precision)
        assert rejected(G.check_timescale, L.restate_timescale(st, rows=np.concatenate([corners, rows]), fault=fault), tw, precision)
    # at rest: the device test of the 13^3 lattice cannot see any of them -- the gap these shapes close
    for perm in (False, True):
        st = BR.lattice(precision, perm)
        want = BR.binaries(st, precision)
        want["partner"] = NB.lattice_expected(BR.LATTICE_K, perm)[0]
        clean = BR.restate(st, precision)
        for fault in small:
            got = BR.restate(st, precision, fault=fault, member0=st)
            assert not BR.differs(got, want, st, precision), (perm, fault)
            assert all(np.array_equal(got[f], clean[f]) for f in BR.KEYS)
    # and the members' own cloud comparison does see a member that reads the first member's velocities
    a, b = BR.cloud(513, precision), BR.cloud(1025, precision)
    assert BR.differs(BR.restate(b, precision, fault="velocity offset of the member not applied", member0=a), BR.binaries(b, precision), b, precision)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_potential_fault_is_rejected(precision):
    k = K_FAULT
    n = k ** 3
    base = L.state(k, precision, True)
    rs = P.Restatement(base, precision)
    assert P.diag_shape(n, n) == (10, 20, 5, 4)
    ones = base["mass"]
    # (a): the total
    dev = G.check_potential(rs.total(ones), k, precision)
    print("fp%d: the restated total deviates by %.2f u of %g" % (precision, dev, G.POTENTIAL_GATE))
    assert rejected(G.check_potential, rs.total(ones, fault=("last tile of the last split skipped", -1, -1)), k, precision)
    assert rejected(G.check_potential, rs.total(ones, finish_rows=32), k, precision)  # the large shapes' own: 32 of 50 rows
    assert rs.total(ones, finish_rows=50) == rs.total(ones)
    # (b): one heavy body
    bodies = [0, 511, 512, 1023, 1024, n - 1]
    hi, lo = G.heavy_lattice_truth(k, precision, True, bodies)
    for a, b in enumerate(bodies):
        mass = G.heavy_lattice_state(k, precision, True, b)["mass"]
        K = lambda **kw: float(P.k_metric(rs.total(mass, **kw), (hi[a], lo[a]), precision)[0])
        assert K() <= G.PROBE_GATE, (b, K())
        j = (b + 300) % n
        for fault in P.FAULTS:
            if fault == "velm read at the global index":
                assert rs.total(mass, fault=(fault, b, j)) == rs.total(mass)  # no fault where i_begin = 0
                continue
            assert K(fault=(fault, b, j)) > G.PROBE_GATE, (b, fault, K(fault=(fault, b, j)))
        assert K(finish_rows=32) > G.PROBE_GATE


@pytest.mark.parametrize("precision", [32, 64])
def test_every_field_fault_is_rejected(oracle, precision):
    n, m = K_FAULT ** 3, 1025
    case = G.field_case(oracle, precision, m, n, "box", every=True)
    assert FR.field_shape(m, n) == (3, 20, 5, 4)
    ka, kp = G.check_field(FR.restate(case["state"], case["points"], precision), case, precision)
    print("fp%d: the restatement's K %.2f of %.1f (acc), %.2f of %.1f (phi)" % (precision, ka, case["gate_acc"], kp, case["gate_phi"]))
    where = {"dropped record": (700, 1500), "doubled record": (3, n - 1), "split partial added twice": (-1, 1)}
    for fault in FR.FAULTS:
        p, j = where.get(fault, (-1, -1))
        assert rejected(G.check_field, FR.restate(case["state"], case["points"], precision, fault=(fault, p, j)), case, precision), fault
