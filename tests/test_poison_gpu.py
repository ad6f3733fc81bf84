"""What a body that is not finite, or whose square overflows T, touches on the device (tests/poison_ref.py): the containment the
headers' "Unspecified results" sentences promise, held bit for bit.

Tier A   ensembles of 3 x 256, 3 x 257 and 3 x 2049 bodies and the ragged ensemble (256, 257, 5, 2049, 513), fp32 and fp64: one
         member holds one poisoned body -- every value of the catalogue in pos_x and vel_y, NaN and +inf in mass, in the member's
         first body and in its last; every interior member in turn, the first and the last member once -- and every clean
         member must give what it gives in a clean control object, over the full range, alone, and in the ranges that end just
         before and start just behind the poisoned member: all fourteen analysis families with their large and small arguments
         on ONE object, and step, kick, leapfrog, hermite_step (resumed), advance and tracers_step on an object each, with the
         kinetic energies, clocks, diagnostics, timescales, downloads and tracers they leave.  The poisoned member itself must
         show the poison in a float output of every family that reads the field (poison_ref.READS).
Tier B   the position poison in a context of 257 and of 2049 bodies and inside one member of each batch kind against the FAR
         control: neighbours, knn (k = 1, 8), nlist, paircount, fof and binaries keep every row their header does not free, the
         freed rows are well-formed and at most 5 % of the rows; field, tidal and tracers_step with point or tracer 0 and m - 1
         poisoned leave every other point and tracer alone.
         knn with k = 6 of n = 5 and neighbours of n = 2 bodies: a partner whose r2 is not below +inf is never inserted, so the
         rows of the OTHER bodies end early -- index -1, r2 +inf -- which is what the corrected sentences of nbx_knn.h and
         nbx_neighbours.h now say; pinned here exactly.

Every comparison is bit for bit (integers by np.array_equal, floats as bytes) or an exact integer condition.  Per-case wall time
and device calls go to poison.json in the GPU suite's report directory (OUT of tests/test_parity_gpu.py).

Measured on an MI355X, the module alone in a fresh process: 762 cases in 13.7 s of wall time, 1.7 s of it the first import and
library load; 10.8 s inside the cases.  An analysis case makes 69 (an ensemble) to 161 (the ragged ensemble) calls on its one
object and takes 23 ms at the median, 0.44 s at most (the first, which also creates the clean control); a steppers case -- six
objects, each stepped and asked -- 7 ms; a rows case of 14 calls 10 ms; about 42 000 device calls in all.  The full cross
product of poisons x fields x bodies x placements fits, so nothing was thinned.  Nothing failed: every comparison held bit for
bit in every case, every Tier B case freed body b's own row and no other, and nothing in csrc/ had to be changed; the two header
sentences named above were.  Pairs within radius +inf (recorded): a NaN position drops the n - 1 pairs of body b, an infinite
or overflowing one keeps them (inf <= inf).
"""
import json
import os
import time

import numpy as np
import pytest

import binaries_ref as B
import call_order_ref as R
import field_ref as FR
import poison_ref as P
import test_call_order_gpu as CO

pytestmark = pytest.mark.gpu

RECORDS = []
_controls = {}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for c in _controls.values():
        c.o.close()
    _controls.clear()
    from test_parity_gpu import OUT  # where the GPU suite leaves its reports
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "poison.json"), "w") as f:
        json.dump({"what": "wall time in seconds and device calls made per case of tests/test_poison_gpu.py", "cases": RECORDS,
                   "total_s": sum(r["seconds"] for r in RECORDS)}, f, indent=1)


def record(t0, test, case, precision, calls, **more):
    RECORDS.append(dict({"test": test, "case": case, "precision": precision, "calls": calls, "seconds": time.perf_counter() - t0}, **more))
    print(json.dumps(RECORDS[-1]))


class Control:
    """An object that holds `states` for the life of the module and is asked every (family, argument, range) once."""

    def __init__(self, nbx, kind, sizes, precision, states):
        self.kind, self.sizes, self.precision, self.asked = kind, sizes, precision, {}
        self.o = CO.make(nbx, kind, sizes, precision)
        CO.upload(self.o, kind, states)

    def ask(self, fam, tag, arg, first, count):
        key = (fam.name, tag, first, count)
        if key not in self.asked:
            self.asked[key] = fam.call(self.o, self.kind, self.sizes, arg, first, count)
        return self.asked[key]


def clean_control(nbx, kind, sizes, precision):
    key = ("clean", kind, sizes, precision)
    if key not in _controls:
        _controls[key] = Control(nbx, kind, sizes, precision, P.clean_states(sizes, precision))
    return _controls[key]


def names_of(fam):
    return ("large",) + (("small",) if "small" in fam.names() else ())


def case_id(case):
    kind, sizes, p, field, name, which = case
    shape = "ragged" if kind == "ragged" else "%dx%d" % (len(sizes), sizes[0])
    return "%s-member%d-%s=%s-%s" % (shape, p, field, name, which)


CASES_A = [(kind, sizes) + pl for kind, sizes in P.shapes() for pl in P.placements(len(sizes))]


def states_of(case, precision):
    kind, sizes, p, field, name, which = case
    clean = P.clean_states(sizes, precision)
    b = P.body_of(which, sizes[p])
    states = list(clean)
    states[p] = P.poisoned(clean[p], field, name, b, precision)
    return clean, states, b


# ---- Tier A: the analysis calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("case", CASES_A, ids=case_id)
def test_a_poisoned_member_leaves_every_analysis_call_of_the_other_members_alone(nbx, case, precision):
    t0 = time.perf_counter()
    kind, sizes, p, field, name, which = case
    S = len(sizes)
    clean, states, b = states_of(case, precision)
    control = clean_control(nbx, kind, sizes, precision)
    bad, hidden, calls = [], [], 0
    with CO.make(nbx, kind, sizes, precision) as o:
        CO.upload(o, kind, states)
        for fam in R.FAMILIES.values():
            args = fam.args(sizes, precision)
            for tag in names_of(fam):
                for first, count in P.ranges_a(S, p):
                    got = fam.call(o, kind, sizes, args[tag], first, count)
                    calls += 1
                    want = control.ask(fam, tag, args[tag], first, count)
                    bad += ["%s(%s) %s" % (fam.name, tag, t) for t in P.tier_a(fam, got, want, first, count, p)]
                    if (first, count) == (0, S) and tag == "large":
                        arg = args[tag][p] if fam.name in ("field", "tidal", "clumps") else args[tag]
                        if P.shows(fam, field, clean[p], b, arg, precision) and P.not_shown(fam, got[p], want[p]):
                            hidden.append(fam.name)
    record(t0, "analysis", case_id(case), precision, calls)
    assert not bad, (case_id(case), precision, bad[:12], len(bad))
    assert not hidden, (case_id(case), precision, "the poison does not show in the poisoned member's own", hidden)


# ---- Tier A: the steppers ------------------------------------------------------------------------------------------------------------
def by_member(kind, sizes, res):
    """A download (or tracers_download) as a list of one dict per member."""
    if isinstance(res, dict):
        return [{k: v[m] for k, v in res.items()} for m in range(len(sizes))]
    return list(res)


def tracer_set(sizes, precision):
    """(points, velocities), each three (members, TRACERS) arrays: box points of the members' clean states, two seeds."""
    clean = P.clean_states(sizes, precision)
    pts = [FR.make_points(precision, st, P.TRACERS, "box", seed=7 + m) for m, st in enumerate(clean)]
    vel = [FR.make_points(precision, st, P.TRACERS, "box", seed=70 + m) for m, st in enumerate(clean)]
    return [np.stack([q[c] for q in pts]) for c in range(3)], [np.stack([q[c] for q in vel]) for c in range(3)]


def _ke(ke):
    return {"kenergy_returned": np.asarray(ke)}


def run_step(o, kind, sizes, precision):
    return [_ke(k) for k in o.step(2, R.DT, kenergy=True)]


def run_kick(o, kind, sizes, precision):
    return [_ke(k) for k in o.kick(0.5 * R.DT, kenergy=True)]


def run_leapfrog(o, kind, sizes, precision):
    return [_ke(k) for k in o.leapfrog(2, R.DT)]


def run_hermite(o, kind, sizes, precision):
    o.hermite_step(R.DT, 2)
    o.hermite_step(R.DT, 1, resume=True)
    return [{} for _ in sizes]


def run_advance(o, kind, sizes, precision):
    o.advance(1.0, 2.0 ** -6, max_steps=3)
    return [{"clock_" + k: np.asarray(v) for k, v in c.items()} for c in o.clock()]


def run_tracers(o, kind, sizes, precision):
    o.tracers_upload(*tracer_set(sizes, precision))
    ke = o.tracers_step(2, R.DT)
    tr = by_member("ensemble", sizes, o.tracers_download())
    return [dict(_ke(k), **{"tracer_" + f: v for f, v in t.items()}) for k, t in zip(ke, tr)]


STEPPERS = {"step": run_step, "kick": run_kick, "leapfrog": run_leapfrog, "hermite_step": run_hermite, "advance": run_advance,
            "tracers_step": run_tracers}


def stepped(nbx, kind, sizes, precision, states, stepper):
    """What `stepper` returns and leaves, one dict per member: its own records, the download, diagnostics and timescale."""
    with CO.make(nbx, kind, sizes, precision) as o:
        CO.upload(o, kind, states)
        out = STEPPERS[stepper](o, kind, sizes, precision)
        down = by_member(kind, sizes, o.download())
        diag = R.FAMILIES["diagnostics"].call(o, kind, sizes, None, 0, len(sizes))
        ts = R.FAMILIES["timescale"].call(o, kind, sizes, None, 0, len(sizes))
    return [dict(a, **b, **{"diag_" + k: v for k, v in c.items()}, **{"ts_" + k: v for k, v in d.items()}) for a, b, c, d in zip(out, down, diag, ts)]


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("case", CASES_A, ids=case_id)
def test_a_poisoned_member_leaves_every_stepper_of_the_other_members_alone(nbx, case, precision):
    t0 = time.perf_counter()
    kind, sizes, p, field, name, which = case
    clean, states, b = states_of(case, precision)
    bad = []
    for stepper in STEPPERS:
        key = ("stepped", kind, sizes, precision, stepper)
        if key not in _cache:
            _cache[key] = stepped(nbx, kind, sizes, precision, clean, stepper)
        got = stepped(nbx, kind, sizes, precision, states, stepper)
        bad += ["%s: %s" % (stepper, t) for t in P.records_differ(got, _cache[key], p)]
        if stepper == "advance":  # the clean members' clocks have moved as the control's: three steps, none at the floor unless there
            assert all(int(g["clock_steps"]) == 3 for m, g in enumerate(got) if m != p), [g["clock_steps"] for g in got]
    record(t0, "steppers", case_id(case), precision, 6 * 4)
    assert not bad, (case_id(case), precision, bad[:12], len(bad))


# ---- Tier B --------------------------------------------------------------------------------------------------------------------------
TARGETS_B = [("context", (257,), 0), ("context", (2049,), 0), ("ensemble", (257,) * 3, 1), ("ensemble", (2049,) * 3, 1),
             ("ragged", P.RAGGED_SIZES, 1), ("ragged", P.RAGGED_SIZES, 3)]


def target_id(t):
    kind, sizes, p = t
    return "%s%d-member%d" % (kind, sizes[p], p)


def calls_b(o, kind, sizes, precision, p):
    """{(family, argument): member p's result} of the Tier B families, member p asked alone; paircount with +inf behind its radii."""
    first, count = (0, 1) if kind == "context" else (p, 1)
    out = {}
    for name, tags in P.TIER_B.items():
        fam = R.FAMILIES[name]
        for tag in tags:
            arg = fam.args(sizes, precision)[tag] if isinstance(tag, str) else tag
            if name == "paircount":
                arg = list(arg) + [np.inf]
            out[(name, tag)] = fam.call(o, kind, sizes, arg, first, count)[0]
    return out


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("which", P.BODIES)
@pytest.mark.parametrize("name", P.VALUES)
@pytest.mark.parametrize("target", TARGETS_B, ids=target_id)
def test_a_poisoned_position_leaves_the_rows_of_the_other_bodies_alone(nbx, target, name, which, precision):
    t0 = time.perf_counter()
    kind, sizes, p = target
    n = sizes[p]
    b = P.body_of(which, n)
    clean = P.clean_states(sizes, precision)
    key = ("far", kind, sizes, p, which, precision)
    if key not in _cache:
        states = list(clean)
        states[p] = P.far(clean[p], b)
        with CO.make(nbx, kind, sizes, precision) as o:
            CO.upload(o, kind, states)
            _cache[key] = calls_b(o, kind, sizes, precision, p)
    states = list(clean)
    states[p] = P.poisoned(clean[p], "pos_x", name, b, precision)
    with CO.make(nbx, kind, sizes, precision) as o:
        CO.upload(o, kind, states)
        got = calls_b(o, kind, sizes, precision, p)
    bad, notes = [], {}
    for (fam, tag), g in got.items():
        w = _cache[key][(fam, tag)]
        if fam == "paircount":
            notes["pairs within +inf"] = [int(g["counts"][-1]), int(w["counts"][-1])]
            g, w = {"counts": g["counts"][:-1]}, {"counts": w["counts"][:-1]}
        problems, freed, rec = P.tier_b(fam, g, w, b, n)
        bad += ["%s(%s): %s" % (fam, tag, t) for t in problems]
        if freed > P.FREED_CAP * n:
            bad.append("%s(%s): %d of %d rows freed" % (fam, tag, freed, n))
        notes.update({"%s %s" % (fam, k): v for k, v in rec.items()})
        notes["%s(%s) rows freed" % (fam, tag)] = freed
    record(t0, "rows", "%s-pos_x=%s-%s" % (target_id(target), name, which), precision, 2 * len(got), notes=notes)
    assert not bad, (target_id(target), name, which, precision, bad)


POINT_KINDS = [("context", (257,)), ("ensemble", (257,) * 3), ("ragged", P.RAGGED_SIZES)]


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("name", P.VALUES)
@pytest.mark.parametrize("shape", POINT_KINDS, ids=lambda s: "%s%d" % (s[0], len(s[1])))
def test_a_poisoned_point_or_tracer_leaves_every_other_point_and_tracer_alone(nbx, shape, name, precision):
    t0 = time.perf_counter()
    kind, sizes = shape
    S = len(sizes)
    clean = P.clean_states(sizes, precision)
    v = P.value(name, precision)
    bad = []
    with CO.make(nbx, kind, sizes, precision) as o:
        CO.upload(o, kind, clean)
        for fname in ("field", "tidal"):
            fam = R.FAMILIES[fname]
            for tag in P.POINTS:
                pts = fam.args(sizes, precision)[tag]
                m = R.POINTS[tag]
                for c in range(3):  # one coordinate at a time
                    hurt = [tuple(np.concatenate([[v], q[1:-1], [v]]).astype(q.dtype) if k == c else q for k, q in enumerate(mp)) for mp in pts]
                    got, want = fam.call(o, kind, sizes, hurt, 0, S), fam.call(o, kind, sizes, pts, 0, S)
                    for mem in range(S):
                        keys = P.others_differ(got[mem], want[mem], (0, m - 1), fam.keys)
                        bad += ["%s(%s) coordinate %d member %d: %s" % (fname, tag, c, mem, k) for k in keys]
                        if P.not_shown(fam, {k: got[mem][k][[0, m - 1]] for k in fam.keys}, {k: want[mem][k][[0, m - 1]] for k in fam.keys}):
                            bad.append("%s(%s) coordinate %d member %d: the poison does not show" % (fname, tag, c, mem))
    # tracers: tracer 0 and the last one poisoned in pos_x, in every member
    pts, vel = tracer_set(sizes, precision) if kind != "context" else [[a[0] for a in x] for x in tracer_set(sizes, precision)]
    hurt = [a.copy() for a in pts]
    hurt[0][..., 0] = hurt[0][..., -1] = v
    runs = []
    for points in (hurt, pts):
        with CO.make(nbx, kind, sizes, precision) as o:
            CO.upload(o, kind, clean)
            o.tracers_upload(points, vel)
            ke = o.tracers_step(2, R.DT)
            runs.append((np.asarray(ke), o.tracers_download(), by_member(kind, sizes, o.download()) if kind != "context" else [o.download()]))
    (ke_g, tr_g, down_g), (ke_w, tr_w, down_w) = runs
    bad += ["tracers_step: tracer %s" % k for k in P.others_differ(tr_g, tr_w, (0, P.TRACERS - 1), list(tr_w))]
    bad += ["tracers_step: body %s" % t for t in P.records_differ(down_g, down_w, -1)]
    if not R._same_value(ke_g, ke_w):
        bad.append("tracers_step: the bodies' kinetic energy")
    if R._same_value(tr_g["pos_x"], tr_w["pos_x"]):
        bad.append("tracers_step: the poison does not show")
    record(t0, "points", "%s%d-%s" % (kind, S, name), precision, 2 * 2 * 3 * 2 + 4)
    assert not bad, (kind, name, precision, bad[:12], len(bad))


# ---- k >= n - 1: the rows of the other bodies end early ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("name", ["big", "nan"])
def test_a_partner_whose_r2_is_not_below_infinity_is_missing_from_the_rows_of_the_other_bodies(nbx, name, precision):
    """n = 5, k = 6, body 0 poisoned: in the far control every other body's row is its four partners, body 0 the last of them,
    then {-1, +inf}; under the poison the rows hold the same three partners with the same r2 bits and then {-1, +inf} three
    times -- r2(i, 0) is +inf or NaN, and `c < +inf` passes neither.  neighbours of n = 2: body 1 has index -1, r2 +inf."""
    st = R.clean_state((5, 0), precision)
    rows = {}
    for tag, s in (("far", P.far(st, 0)), ("poison", P.poisoned(st, "pos_x", name, 0, precision))):
        with nbx.Context(5, precision) as c:
            c.upload(s)
            rows[tag] = c.knn(6)
    inf = B.DTYPE[precision](np.inf)
    for i in range(1, 5):
        f, g = {k: rows["far"][k][i] for k in rows["far"]}, {k: rows["poison"][k][i] for k in rows["poison"]}
        assert f["index"][3] == 0 and np.isfinite(f["r2"][:4]).all() and f["index"][4:].tolist() == [-1, -1] and (f["r2"][4:] == inf).all()
        assert sorted(g["index"][:3].tolist()) == [j for j in range(1, 5) if j != i]
        assert R._same_value(g["index"][:3], f["index"][:3]) and R._same_value(g["r2"][:3], f["r2"][:3])
        assert g["index"][3:].tolist() == [-1, -1, -1] and R._same_value(g["r2"][3:], np.full(3, inf))
    two = B.cloud(2, precision)
    with nbx.Context(2, precision) as c:
        c.upload(P.far(two, 0))
        f = c.neighbours(0.25)
        c.upload(P.poisoned(two, "pos_x", name, 0, precision))
        g = c.neighbours(0.25)
    assert f["index"][1] == 0 and np.isfinite(f["r2"][1]) and f["within"][1] == 0
    assert g["index"][1] == -1 and R._same_value(g["r2"][1:], np.full(1, inf)) and g["within"][1] == 0
