"""What tests/test_large_steppers_gpu.py and the clamp, cold-start and degenerate cases of tests/test_advance_gpu.py rely on, and
why they see what the steppers' module tests could not; no GPU.

The shapes of the new cases against field_shape, through tests/field_shape_driver.cpp.  The floor histories the clamp cases
assert, from jerk_ref.direct in both precisions, every x at least 0.012 from a power of four.  advance_ref.FLOOR_FAULTS: each
leaves every history and clock of the fault cases of tests/test_advance_cpu.py as it was -- no floor binds there and nobody is
at rest -- and changes a clock of a named clamp, cold-start or degenerate case.  (That module's one run with a floor that binds
asserts floor_steps to within one, with no fault planted: it is no fault case.)

A model of the index arithmetic of one step (model()): which tiles a split walks, which row records the finish adds for body i
of member k, which candidates the clock of system k reads and which clock record its kernels take h from -- with planted faults.
OLD are the shapes the module tests stop at (n <= 4097, 3 x 2049, (5, 2049, 257, 1, 513), levels = 24), their candidates the start
candidates of jerk_ref's fp64 states by direct summation, so the model knows which body decides them; NEW are the cases of the
GPU module, the deciding body where that module plants it.  Per fault, the first shapes that catch it:

  a tile index kept in 8 bits                                        no old shape (17 tiles at most); k = 81: 2076 tiles reread tile 0
  the finish adds at most 8 splits                                   no old shape (4 splits at most); k = 33 (15), the members (13)
  the candidate loop stops at index 65 536                           no old shape; k = 81 with the body planted behind 2^16
  the candidate loop skips the last partial stride                   OLD n = 2 and 5 already: fewer than 256 candidates, none is read
  ... once a whole stride has been read                              no old shape: no old minimum sits in a tail; the plants at n - 1
  a member's candidates taken at k * n_largest in a ragged object    OLD (5, 2049, 257, 1, 513) already: member 1 would read at 2049
  the clock of member k > 255 read from record k & 255               no old shape (5 members at most); 1025 systems
  a member's rows at out_off * its own splits                        OLD (5, 2049, 257, 1, 513) already: member 2's rows, 1 split of 4

Three of the eight are no blind spot of the old shapes and are kept, named as such, rather than dropped: the module tests meet
them.  The other five pass every old shape and fail at the named new case; that is asserted fault by fault."""
import math
import os
import subprocess

import numpy as np
import pytest

import advance_ref as A
import field_ref as FR
import hermite_ref as H
import jerk_ref as R
import test_advance_cpu as TC
import test_advance_gpu as AG
import test_large_steppers_gpu as G
from conftest import PKG, ROOT
from energy_ref import EPS2, gm_as_uploaded

CSRC = os.path.join(PKG, "csrc")
TILE, COL = FR.TILE, FR.COL


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------
# (m, n) -> (columns, tiles, splits, tiles per split), tiles of the last split, records of the last tile
REGIMES = {
    "k33": ((35937, 35937), (71, 141, 15, 10), 1, 97),
    "k81": ((531441, 531441), (1038, 2076, 1, 2076), 2076, 241),
    "k25": ((15625, 15625), (31, 62, 13, 5), 2, 9),
    "k23": ((12167, 12167), (24, 48, 12, 4), 4, 135),
    "small member": ((8192, 8192), (16, 32, 8, 4), 4, 256),
    "five bodies": ((5, 5), (1, 1, 1, 1), 1, 5),
}


def test_the_regime_table_is_the_headers_and_the_gpu_modules(tmp_path):
    exe = str(tmp_path / "field_shape_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "field_shape_driver.cpp"), "-o", exe])
    names = sorted(REGIMES)
    lines = subprocess.run([exe] + [str(v) for name in names for v in REGIMES[name][0]], capture_output=True, text=True, check=True).stdout.splitlines()[:-1]
    for name, line in zip(names, lines):
        (m, n), shape, last_split, last_tile = REGIMES[name]
        assert tuple(int(v) for v in line.split()) == (m, n) + shape == (m, n) + FR.field_shape(m, n), name
        columns, tiles, splits, per = shape
        assert tiles - (splits - 1) * per == last_split and n - (tiles - 1) * TILE == last_tile, name
    for k, shape in G.SHAPES.items():
        assert REGIMES["k%d" % k][1] == shape and REGIMES["k%d" % k][0] == (k ** 3, k ** 3)
    assert G.MEMBER_K == {32: 25, 64: 23} and G.SMALL_MEMBERS == (5, 8192) and G.MANY == (1025, 5)
    assert REGIMES["k81"][1][1] > 256 and REGIMES["k33"][1][2] > 8 and REGIMES["k25"][1][2] > 8 and REGIMES["k23"][1][2] > 8
    # the gridDim.y of the ragged launch is the lattice's; the small members own 1 and 8 of its 13 or 12 rows of splits
    assert [REGIMES[name][1][2] for name in ("five bodies", "k25", "small member")] == [1, 13, 8]
    for k in (33, 81):
        n, sites = k ** 3, G.plant_sites(k)
        assert sites[0] == n - 1 and sites[1] == (REGIMES["k%d" % k][1][0] - 1) * COL and all(0 < p < n for p in sites)
        assert n % TILE != 0 and sites[0] >= (n // TILE) * TILE  # n - 1 lies in the last, partial stride of the candidate loop
    assert G.plant_sites(81)[2] > 1 << 16 and G.plant_sites(81)[3] % 256 == 255 and G.plant_sites(81)[3] > 1 << 16
    for f, w in zip(R.VEL, G.PLANT):  # the planted velocity is exact in fp32
        v = R.lattice(32, False, 33)[f]
        assert (np.abs(v) < 64).all() and np.array_equal(v * 2, np.rint(v * 2)) and w == 1024.0


# ---- the clamp cases on the CPU --------------------------------------------------------------------------------------------------------
def _floor(precision, n, family, levels, steps, fault=None, t_end=AG.FAR):
    return A.run(R.make_state(precision, n, family), precision, t_end, AG.K_CAP, levels, AG.ETA, steps, R.direct, fault=fault)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_floor_histories_of_the_clamp_cases(precision):
    some = False
    for n, family, levels, steps, exponents, floor_steps in AG.FLOOR_CASES:
        r = _floor(precision, n, family, levels, steps)
        assert [A.exponent(h) for _, h, _ in r["history"]] == exponents and r["clock"]["floor_steps"] == floor_steps, (n, family, levels, r["clock"])
        assert min(A.boundary_distance(x) for _, _, x in r["history"]) >= 0.012
        a, j = R.direct(R.make_state(precision, n, family))
        # the start: 0.0078 at the nearest (five bodies) -- the device's evaluation differs from this one by parts in 10^6 at most
        assert A.boundary_distance(AG.ETA ** 2 * A.minimum(A.start_candidates(a, j))) >= 1e-3
        some = some or 0 < floor_steps < steps
        part = _floor(precision, n, family, levels, 2)  # the seam the device cases cut at
        rest = A.run(part["state"], precision, AG.FAR, AG.K_CAP, levels, AG.ETA, steps - 2, R.direct, clock=part["clock"], carry=part["carry"])
        assert rest["clock"] == r["clock"] and H.same(rest["state"], r["state"])
    assert some
    # the members: t_end = dt_cap, levels = 3, 12 steps asked
    clocks = {(n, fam): _floor(precision, n, fam, AG.FLOOR_LEVELS, AG.FLOOR_MAX_STEPS, t_end=AG.DT_CAP)["clock"]
              for n, fam in AG.FLOOR_ENSEMBLE + AG.FLOOR_RAGGED}
    assert [(c["steps"], c["floor_steps"], c["floor_next"]) for c in clocks.values()] == [(7, 4, True), (8, 8, True), (8, 8, True), (1, 0, False)]
    assert all(c["t"] == AG.DT_CAP for c in clocks.values())


@pytest.mark.parametrize("precision", [32, 64])
def test_the_cold_start_and_the_degenerate_cases(precision):
    r = A.run(R.make_state(precision, 257, "rest"), precision, AG.FAR, AG.K_CAP, AG.LEVELS, AG.ETA, 6, R.direct)
    assert [A.exponent(h) for _, h, _ in r["history"]][:4] == [-4, -10, -16, -17] and r["clock"]["floor_steps"] == 0
    r = A.run(R.make_state(precision, 5, "rest"), precision, AG.FAR, AG.K_CAP, AG.LEVELS, AG.ETA, 6, R.direct)
    assert [A.exponent(h) for _, h, _ in r["history"]] == [-4, -4, -5, -5, -5, -5]
    for n in (5, 257):
        a, j = R.direct(R.make_state(precision, n, "rest"))
        assert not j.any() and np.isposinf(A.start_candidates(a, j)).all()
    T = R.DTYPE[precision]
    for name, infinite in (("massless", [1]), ("coincident", []), ("coincident massless", [0, 1])):
        st = AG.degenerate_states(precision)[name]
        a, j = R.direct(st)
        s = A.start_candidates(a.astype(T), j.astype(T))
        assert np.flatnonzero(np.isposinf(s)).tolist() == infinite and math.isfinite(A.minimum(s)) and not np.isnan(s).any(), (name, s)
        r = A.run(st, precision, AG.FAR, AG.K_CAP, AG.LEVELS, AG.ETA, 3, R.direct)
        assert all(math.isfinite(x) and x > 0 for _, _, x in r["history"]) and r["clock"]["floor_steps"] == 0


# ---- the floor faults ------------------------------------------------------------------------------------------------------------------
def _degenerate(name):
    return lambda p, f: A.run(AG.degenerate_states(p)[name], p, AG.FAR, AG.K_CAP, AG.LEVELS, AG.ETA, 3, R.direct, fault=f)


NEW_CLOCK_CASES = {
    "floor levels 2": lambda p, f: _floor(p, 5, "cloud", 2, 8, f),
    "floor levels 3": lambda p, f: _floor(p, 5, "cloud", 3, 16, f),
    "floor levels 0": lambda p, f: _floor(p, 5, "cloud", 0, 3, f),
    "floor 257 clustered": lambda p, f: _floor(p, 257, "clustered", 8, 6, f),
    "member done first": lambda p, f: _floor(p, 5, "cloud", AG.FLOOR_LEVELS, AG.FLOOR_MAX_STEPS, f, t_end=AG.DT_CAP),
    "cold 257": lambda p, f: A.run(R.make_state(p, 257, "rest"), p, AG.FAR, AG.K_CAP, AG.LEVELS, AG.ETA, 6, R.direct, fault=f),
    "massless": _degenerate("massless"),
    "coincident massless": _degenerate("coincident massless"),
}
FLOOR_FAULT_CAUGHT_BY = {
    "floor_steps counts a step when it is chosen": ["floor levels 2", "floor levels 3", "floor levels 0", "floor 257 clustered", "member done first"],
    "raised is evaluated after the clamp": ["floor levels 2", "floor levels 3", "floor levels 0", "floor 257 clustered", "member done first"],
    "a done system's floor_steps keeps counting": ["member done first"],
    "the start candidate is 0 where J is 0": ["cold 257", "massless", "coincident massless"],
}


def test_every_floor_fault_changes_no_case_of_the_advance_module_and_a_clock_of_a_new_case():
    assert set(A.FLOOR_FAULTS) == set(FLOOR_FAULT_CAUGHT_BY) and len(A.FLOOR_FAULTS) == 4 and not set(A.FLOOR_FAULTS) & set(A.FAULTS)
    old = [lambda f, seed=seed: TC._smooth(seed, 0.125, fault=f) for seed in R.HERMITE_SEEDS]
    old += [lambda f, n=n, fam=fam, p=p: TC._small(p, n, fam, fault=f) for p in (32, 64) for n, fam in ((5, "cloud"), (33, "clustered"), (257, "clustered"))]
    for run in old:
        good = run(None)
        for fault in A.FLOOR_FAULTS:
            bad = run(fault)
            assert bad["history"] == good["history"] and bad["clock"] == good["clock"] and H.same(bad["state"], good["state"]), fault
    for precision in (32, 64):
        good = {name: run(precision, None) for name, run in NEW_CLOCK_CASES.items()}
        for fault in A.FLOOR_FAULTS:
            caught = [name for name, run in NEW_CLOCK_CASES.items() if run(precision, fault)["clock"] != good[name]["clock"]]
            print("fp%d %-46s: %s" % (precision, fault, caught))
            assert caught == FLOOR_FAULT_CAUGHT_BY[fault], (precision, fault, caught)


# ---- the model of a step's index arithmetic --------------------------------------------------------------------------------------------
FAULTS = ("a tile index kept in 8 bits", "the finish adds at most 8 splits", "the candidate loop stops at index 65 536",
          "the candidate loop skips the last partial stride", "the candidate loop skips the last partial stride once a whole stride has been read",
          "a member's candidates taken at k * n_largest in a ragged object", "the clock of member k > 255 read from record k & 255",
          "a member's rows at out_off * its own splits")


def model(kind, sizes, cands, records, fault=None):
    """What one step gets wrong, as a list of words (empty: nothing).  kind: "context", "ensemble" or "ragged"; sizes: the bodies
    of every system; cands: one array of candidates per system; records: what every system's clock record holds (any values).
      tiles       split s of a system walks tiles [s per, min(tiles, (s + 1) per)): every tile of the system exactly once
      rows        the pair work writes (split s, body i) of system k at (out_off_k gridDim.y + s n_k + i), gridDim.y the largest
                  split count; the finish adds rows (out_off_k gridDim.y + i) + s n_k for s below the system's own split count
      candidates  the clock of system k takes the minimum over cand[off_k + i], i < n_k, in strides of 256: the k_crit of what
                  it reads must be the k_crit of the system's own minimum
      record      every kernel of system k reads clock record k"""
    assert fault is None or fault in FAULTS, fault
    wrong = []
    shapes = [FR.field_shape(n, n) for n in sizes]
    grid_y = max(s[2] for s in shapes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = np.concatenate([np.asarray(c, dtype=np.float64) for c in cands])
    for k, (n, (columns, tiles, splits, per)) in enumerate(zip(sizes, shapes)):
        walked = np.concatenate([np.arange(s * per, min(tiles, (s + 1) * per)) for s in range(splits)])
        if fault == "a tile index kept in 8 bits":
            walked = walked & 255
        if not np.array_equal(np.sort(walked), np.arange(tiles)):
            wrong.append("tiles of system %d" % k)
        base = off[k] * (splits if fault == "a member's rows at out_off * its own splits" else grid_y)
        added = min(splits, 8) if fault == "the finish adds at most 8 splits" else splits
        i = np.array([0, n // 2, n - 1], dtype=np.int64)
        written = {(s, int(b)): int(base + s * n + b) for s in range(splits) for b in i}
        read = {(s, int(b)): int(off[k] * grid_y + b + s * n) for s in range(added) for b in i}
        if read != written:
            wrong.append("rows of system %d" % k)
        start = k * max(sizes) if (fault == "a member's candidates taken at k * n_largest in a ragged object" and kind == "ragged") else int(off[k])
        stop = n
        if fault == "the candidate loop stops at index 65 536":
            stop = min(n, 1 << 16)
        elif fault == "the candidate loop skips the last partial stride" or (fault == FAULTS[4] and n >= TILE):
            stop = (n // TILE) * TILE
        if start + stop > len(flat):
            wrong.append("candidates of system %d: read behind the buffer" % k)
        elif A.k_crit(A.minimum(flat[start:start + stop]), 1.0) != A.k_crit(A.minimum(cands[k]), 1.0):
            wrong.append("candidates of system %d" % k)
        rec = k & 255 if fault == "the clock of member k > 255 read from record k & 255" else k
        if records[rec] != records[k]:
            wrong.append("record of system %d" % k)
    return wrong


def _start_candidates(st):
    """The start candidates of a state by direct summation in fp64, in chunks of rows."""
    x = np.stack([st[f].astype(np.float64) for f in R.POS])
    v = np.stack([st[f].astype(np.float64) for f in R.VEL])
    g = gm_as_uploaded(st["mass"]).astype(np.float64)
    n = x.shape[1]
    a, j = np.zeros((3, n)), np.zeros((3, n))
    for r in range(0, n, 128):
        d = x[:, None, :] - x[:, r:r + 128, None]
        u = v[:, None, :] - v[:, r:r + 128, None]
        r2 = (d * d).sum(axis=0) + EPS2
        w3 = g[None, :] / (r2 * np.sqrt(r2))
        c = -3.0 * (d * u).sum(axis=0) / r2
        a[:, r:r + 128], j[:, r:r + 128] = (d * w3).sum(axis=2), ((u + c * d) * w3).sum(axis=2)
    return A.start_candidates(a, j)


_old = {}


def old_shapes():
    """{name: (kind, sizes, cands, records)} of the shapes tests/test_hermite_gpu.py and tests/test_advance_gpu.py stop at."""
    if not _old:
        cand = lambda n, fam: _start_candidates(R.make_state(64, n, fam))
        for n, fam in AG.CASES:
            _old["context %d %s" % (n, fam)] = ("context", (n,), [cand(n, fam)], [0])
        _old["ensemble 3 x 2049"] = ("ensemble", (2049,) * 3, [cand(n, fam) for fam, n in AG.ENSEMBLE], [0, 1, 2])
        _old["ragged (5, 2049, 257, 1, 513)"] = ("ragged", AG.RAGGED, [cand(n, "cloud") for n in AG.RAGGED], list(range(5)))
    return _old


def _planted(n, p, low=2.0 ** -6):
    c = np.ones(n)
    c[p] = low  # three levels below the others
    return c


def new_shapes():
    """The cases of tests/test_large_steppers_gpu.py: the deciding body where that module plants it (its own conditions hold
    the device to that), else the last body of each system."""
    out = {}
    for k in (33, 81):
        n = k ** 3
        for p in G.plant_sites(k):
            out["k = %d planted at %d" % (k, p)] = ("context", (n,), [_planted(n, p)], [0])
    for precision, k in G.MEMBER_K.items():
        sizes = (G.SMALL_MEMBERS[0], k ** 3, G.SMALL_MEMBERS[1])
        cands = [_planted(m, m - 1, 4.0 ** -(3 + i)) for i, m in enumerate(sizes)]
        out["members fp%d ragged" % precision] = ("ragged", sizes, cands, [0, 1, 2])
        out["members fp%d ensemble" % precision] = ("ensemble", (k ** 3,), cands[1:2], [0])
    members, n = G.MANY
    out["many"] = ("ensemble", (n,) * members, [_planted(n, n - 1, 4.0 ** -(1 + m % 5)) for m in range(members)], [m % 5 for m in range(members)])
    return out


CAUGHT_BY_OLD = {  # fault -> the old shapes that catch it ([]: a blind spot of the module tests)
    FAULTS[0]: [], FAULTS[1]: [], FAULTS[2]: [],
    FAULTS[3]: ["context 2 cloud", "context 5 cloud", "ragged (5, 2049, 257, 1, 513)"],  # fewer than 256 candidates: nothing is read
    FAULTS[4]: [],
    FAULTS[5]: ["ragged (5, 2049, 257, 1, 513)"],  # member 1 at 2049 and not at 5
    FAULTS[6]: [],
    FAULTS[7]: ["ragged (5, 2049, 257, 1, 513)"],  # member 2: own split count 1, gridDim.y 4
}
NAMED_NEW_CASE = {
    FAULTS[0]: "k = 81 planted at 531440", FAULTS[1]: "k = 33 planted at 35936", FAULTS[2]: "k = 81 planted at 65537",
    FAULTS[3]: "k = 33 planted at 35936", FAULTS[4]: "k = 81 planted at 531440", FAULTS[5]: "members fp32 ragged", FAULTS[6]: "many",
    FAULTS[7]: "members fp64 ragged",
}


def test_the_model_without_a_fault_passes_every_shape():
    for name, shape in list(old_shapes().items()) + list(new_shapes().items()):
        assert model(*shape) == [], name


def test_no_old_minimum_sits_where_the_new_cases_put_theirs():
    """The body that decides an old case, on the fp64 start candidates: never in the last partial stride of 256, never behind
    4097 -- which is why a minimum that skipped a tail passed them."""
    for name, (kind, sizes, cands, _) in old_shapes().items():
        for n, c in zip(sizes, cands):
            if n >= TILE:
                assert int(np.argmin(c)) < (n // TILE) * TILE, (name, n, int(np.argmin(c)))


@pytest.mark.parametrize("fault", FAULTS)
def test_a_planted_fault_passes_the_old_shapes_and_fails_at_its_named_new_case(fault):
    old = [name for name, shape in old_shapes().items() if model(*shape, fault=fault)]
    new = {name: model(*shape, fault=fault) for name, shape in new_shapes().items()}
    print(fault, "\n old:", old, "\n new:", {k: v[:2] for k, v in new.items() if v})
    assert old == CAUGHT_BY_OLD[fault], (fault, old)  # [] for a blind spot; named above where the module tests meet it already
    assert new[NAMED_NEW_CASE[fault]], fault
    if fault == FAULTS[0]:
        assert [name for name, w in new.items() if w] == [n for n in new if n.startswith("k = 81")]  # 141 tiles at k = 33 fit 8 bits
    if fault == FAULTS[2]:
        assert not new["k = 33 planted at 35936"] and new["k = 81 planted at 65537"]
    if fault == FAULTS[6]:
        assert new["many"] == ["record of system %d" % k for k in range(256, 1025) if k % 5 != (k & 255) % 5]


@pytest.mark.parametrize("precision", [32, 64])
def test_the_members_of_the_many_systems_that_alias_modulo_256_take_different_steps(precision):
    """On the restatement (jerk_ref.direct): within (0, 256, 1024), (255, 1023) and (1, 257) no two members have the same clock
    after six steps, so a record read at k & 255 shows; every member with J = 0 at the start is a copy of "rest" in motion."""
    states = G.many_states(precision)
    assert len(states) == 1025 and all(len(s["mass"]) == 5 for s in states)
    clock = lambda m: A.run(states[m], precision, G.FAR, G.K_CAP, G.LEVELS, G.ETA, G.MANY_STEPS, R.direct)["clock"]
    for group in ((0, 256, 1024), (255, 1023), (1, 257)):
        got = [clock(m) for m in group]
        assert len({(c["t"], c["dt_next"]) for c in got}) == len(group), (group, got)
        assert all(c["steps"] == G.MANY_STEPS and c["floor_steps"] == 0 for c in got)
    for m in (2, 7, 1022):  # "rest", shifted: in motion and still without a jerk
        a, j = R.direct(states[m])
        assert m % 5 == 2 and not j.any() and (m == 2 or any(states[m][f].any() for f in R.VEL))
    assert not H.same(states[4], states[9]) and not H.same(states[2], states[7]) and H.same(states[0], states[5])  # shifted copies differ, the others are copies
