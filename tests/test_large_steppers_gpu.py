"""The fixed Hermite stepper and the adaptive one (include/nbx_hermite.h, include/nbx_advance.h) above n = 4097: the shapes of
tests/test_large_shapes_gpu.py, which the steppers' own modules (tests/test_hermite_gpu.py, tests/test_advance_gpu.py) stop short
of.  Their pair loops restate the jerk loop with the predictor fused into the loads, with partial rows and finish kernels of
their own, and nbx_advance adds a candidate buffer, a strided minimum per system and the quantiser: none of it had met more than
nine columns, four splits, 17 tiles, five members or 4097 candidates.

Everything is asked bit for bit, against the references the module tests use: hermite_ref.round_trip / hermite_ref.steps and
advance_ref.run, their evaluations the device's own jerk() on a twin object (hermite_ref.device_evaluate).  No O(n^2) reference,
no tolerance, no measured gate.  That is sound at these shapes because tests/test_jerk_gpu.py holds jerk() itself against
jerk_ref.truth at (71, 141, 15, 10) and at (1038, 2076, 1, 2076), and the steppers are held here to that call's bits on every body.

States: jerk_ref.lattice(precision, perm, k) -- Hubble flow plus rotation, every velocity exact -- cached with their results.
  k = 33   35 937 bodies, 71 columns x 15 splits, natural and permuted order: hermite_step(h, 1) and a resumed one against the
           round trip, h the restatement's first adaptive step; four calls of advance(max_steps=1) -- after each the clock is the
           restatement's, the state the restatement's and what hermite_step(dt_last, 1, resume) leaves on a third context -- and one
           call of four steps is those four calls
  k = 81   531 441 bodies, 1038 columns of one split that walks 2076 tiles, natural order: the same with two steps
  planted  one body of the natural lattice with PLANT added to its velocity, at n - 1, at the first body of the last column and, at
           k = 81, at 65 537 (behind 2^16) and at 518 399 (the last index below a multiple of 256): on the restatement's values
           that body is the argmin of the start candidates and the minimum without it has another k_crit, so a clock kernel that
           missed it would report another first step (dt_last after one step).  In these cases the body on the centre site
           is moved by 1/16 in x: at the centre of an odd lattice the acceleration is rounding noise while a planted velocity
           anywhere gives that body a jerk, so its candidate A / J would be the minimum whatever is planted (in fp64 far below
           any floor) -- measured here with the centre in place: argmin 17 968 of 35 937.  Moved, it has an acceleration.
  members  the lattice of k = 25 (fp32: 13 splits of 5 tiles) or k = 23 (fp64: 12 splits of 4 tiles), the largest a batch object
           holds, alone in an Ensemble and as the middle member of a Ragged of (5, k^3, 8192): every member ends where a lone
           context ends, with its clock, after hermite_step(h, 2) and after advance(max_steps=3); the small members' workgroups
           return early from a grid sized for the large one and their rows sit at out_off * gridDim.y
  many     an Ensemble of 1025 x 5 bodies, the families cycled: members 0, 255, 256, 257, 1023 and 1024 against lone contexts,
           steps == 6 and t the sum of the steps everywhere, clock(first, count) over sub-ranges against the full answer

dt_cap = 2^-4, levels = 40, eta = 0.125: on the restatement every chosen exponent lies strictly inside (k_cap - levels, k_cap), so
the clamp decides nothing here (tests/test_advance_gpu.py has the clamp), and eta^2 q stays 1e-9 away from every power of four.

Every case's shape, exponents, deciding indices and time go to large_steppers.json in the GPU suite's report directory (OUT of
tests/test_parity_gpu.py); nothing in that file is a gate.

Measured on an MI355X: the whole module 24 s, 19 s of it at k = 81 -- fp64: 7.0 s for the adaptive and the fixed case together
(two adaptive steps stay under the ten seconds they were given), 1.6 s per planted case; fp32: 3.2 s and 0.75 s -- and no other
test above 0.6 s.  The clamp and degenerate cases of tests/test_advance_gpu.py add under a second to that module's 3.8 s.
What the lattice showed on the way: from its second step on the body on the centre site, whose acceleration is rounding noise,
decides alone and takes the step down five or six levels a step (fp32, k = 33: 2^-7, 2^-13, 2^-18, 2^-24, next 2^-29), which is
why levels = 40 here and not the 24 of the module tests."""
import json
import os
import time

import numpy as np
import pytest

import advance_ref as A
import field_ref as FR
import hermite_ref as H
import jerk_ref as R

pytestmark = pytest.mark.gpu

K_CAP, LEVELS, ETA = -4, 40, 0.125
DT_CAP = 2.0 ** K_CAP
FAR = 1.0
CLOCK_KEYS = ("n", "t", "dt_last", "dt_next", "steps", "floor_steps", "done")
STEPS = {33: 4, 81: 2}  # adaptive steps of the context cases
SHAPES = {33: (71, 141, 15, 10), 81: (1038, 2076, 1, 2076), 25: (31, 62, 13, 5), 23: (24, 48, 12, 4)}
CONTEXT_CASES = ((33, False), (33, True), (81, False))
PLANT = (1024.0, 1024.0, 1024.0)  # added to one body's velocity: exact in both precisions (the lattice's are multiples of 1/2 below 64)
CENTRE_SHIFT = 1.0 / 16           # of the centre body's x in the planted cases (see the module docstring)
MEMBER_K = {32: 25, 64: 23}       # tests/test_large_shapes_gpu.py
SMALL_MEMBERS = (5, 8192)
MEMBER_H = 2.0 ** -8              # the lattice's own criterion asks for 2^-7
MANY = (1025, 5)
MANY_PROBED = (0, 255, 256, 257, 1023, 1024)
MANY_STEPS = 6
MANY_SHIFT = (0.125, -0.0625, 0.25)

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
    with open(os.path.join(OUT, "large_steppers.json"), "w") as f:
        json.dump({"dt_cap": DT_CAP, "levels": LEVELS, "eta": ETA, "cases": RECORDS}, f, indent=1)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def plant_sites(k):
    """The bodies that get PLANT, one at a time."""
    n = k ** 3
    sites = [n - 1, (FR.field_shape(n, n)[0] - 1) * FR.COL]
    if k == 81:
        sites += [(1 << 16) + 1, 518399]
    return sites


def state(precision, k, perm=False, plant=None):
    def make():
        st = R.lattice(precision, perm, k)
        if plant is not None:
            for f, w in zip(R.VEL, PLANT):
                v = st[f].astype(np.float64)
                v[plant] += w
                st[f] = np.ascontiguousarray(v.astype(st[f].dtype))
                assert np.array_equal(st[f].astype(np.float64), v)  # exact
            c = (k ** 3 - 1) // 2  # the natural lattice's centre site
            x = st["pos_x"].astype(np.float64)
            assert plant != c and x[c] == 0.0 and not st["pos_y"][c] and not st["pos_z"][c]
            x[c] += CENTRE_SHIFT
            st["pos_x"] = np.ascontiguousarray(x.astype(st["pos_x"].dtype))
        return st
    return cached(("state", precision, k, perm, plant), make)


def _adv(o, t_end=FAR, max_steps=1, resume=False):
    o.advance(t_end, DT_CAP, ETA, LEVELS, max_steps, resume)


def _check_boundary(x):
    """tests/test_advance_gpu.py's: eta^2 q of the restatement 1e-9 away from every power of four where the clamp does not decide."""
    if np.isfinite(x) and x > 0.0 and K_CAP - LEVELS <= A.k_crit(x, 1.0) <= K_CAP + 1:
        assert A.boundary_distance(x) >= 1e-9, x


def _decider(s):
    return int(np.nanargmin(s)) if not np.isnan(s).all() else -1


def driven(nbx, precision, k, perm=False, plant=None, steps=None, full=True):
    """`steps` calls of advance(max_steps=1), resumed after the first, on one context; beside it the restatement fed by jerk() of a
    second context and, if full, a third context driven by hermite_step with the restatement's steps, and one call of all the
    steps on the second.  Computed once per case; every reference-side figure in it comes from the restatement."""
    steps = STEPS[k] if steps is None else steps

    def make():
        st = state(precision, k, perm, plant)
        n = k ** 3
        seen, rows, ref, times = [], [], None, []
        with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b, nbx.Context(n, precision) as c:
            plain = H.device_evaluate(b)

            def ev(s):
                seen.append(plain(s))
                return seen[-1]

            a.upload(st)
            if full:
                c.upload(st)
            for call in range(steps):
                t0 = time.perf_counter()
                _adv(a, resume=call > 0)
                clock = a.clock()
                times.append(time.perf_counter() - t0)
                ref = A.run(st if ref is None else ref["state"], precision, FAR, K_CAP, LEVELS, ETA, 1, ev, clock=ref and ref["clock"],
                            carry=ref and ref["carry"])
                (_, h, x), = ref["history"]
                _check_boundary(x)
                got = a.download()
                row = {"clock": clock, "ref": A.public(ref["clock"], FAR, n), "h": h, "round_trip": H.same(got, ref["state"])}
                if full:
                    c.hermite_step(h, 1, resume=call > 0)
                    row["fixed"] = H.same(got, c.download())
                rows.append(row)
            out = {"rows": rows, "state": got, "clock": rows[-1]["clock"], "steps": [r["h"] for r in rows], "times": times}
            if full:
                t0 = time.perf_counter()
                b.upload(st)
                _adv(b, max_steps=steps)
                out["one_call"] = (H.same(b.download(), got), b.clock())
                out["one_call_time"] = time.perf_counter() - t0
        start = A.start_candidates(*seen[0])
        _check_boundary(ETA * ETA * A.minimum(start))
        T = R.DTYPE[precision]
        after = [A.candidates(seen[i][0].astype(T), seen[i][1].astype(T), seen[i + 1][0].astype(T), seen[i + 1][1].astype(T), rows[i]["h"])
                 for i in range(steps)]
        out.update(start=start, deciders=[_decider(start)] + [_decider(s) for s in after],
                   exponents=[A.exponent(h) for h in out["steps"]] + [A.exponent(ref["clock"]["dt_next"])])
        record(case="context", precision=precision, k=k, perm=perm, plant=plant, shape=FR.field_shape(n, n), exponents=out["exponents"],
               deciders=out["deciders"], seconds_per_call=[round(t, 4) for t in times], one_call_seconds=round(out.get("one_call_time", 0.0), 4))
        # the clamp decides nothing: on the restatement every chosen exponent lies strictly inside (k_cap - levels, k_cap)
        assert all(K_CAP - LEVELS < e < K_CAP for e in out["exponents"]), out["exponents"]
        return out
    return cached(("driven", precision, k, perm, plant, steps, full), make)


@pytest.mark.parametrize("k", sorted(SHAPES))
def test_the_shapes_are_the_regimes_they_are_named_for(k):
    assert FR.field_shape(k ** 3, k ** 3) == SHAPES[k]


@pytest.mark.parametrize("k,perm", CONTEXT_CASES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_fixed_step_of_the_lattice_is_the_round_trip_and_a_resumed_one_continues_it(nbx, precision, k, perm):
    n = k ** 3
    assert FR.field_shape(n, n) == SHAPES[k]
    h = driven(nbx, precision, k, perm)["steps"][0]  # the restatement's first adaptive step: a sensible one
    st = state(precision, k, perm)
    t0 = time.perf_counter()
    with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b:
        a.upload(st)
        a.hermite_step(h, 1)
        got = a.download()
        end, kept = H.round_trip(b, st, h, 1)
        assert H.same(got, end) and not H.same(got, st), (precision, k, perm)
        a.hermite_step(h, 1, resume=True)
        end2, _ = H.round_trip(b, end, h, 1, carry=kept)
        assert H.same(a.download(), end2) and not H.same(end, end2), (precision, k, perm)
    record(case="fixed", precision=precision, k=k, perm=perm, shape=FR.field_shape(n, n), exponents=[A.exponent(h)] * 2,
           seconds=round(time.perf_counter() - t0, 3))


@pytest.mark.parametrize("k,perm", CONTEXT_CASES)
@pytest.mark.parametrize("precision", [32, 64])
def test_step_by_step_the_lattices_clock_is_the_restatements_and_its_state_the_fixed_steppers(nbx, precision, k, perm):
    n = k ** 3
    assert FR.field_shape(n, n) == SHAPES[k]
    t0 = time.perf_counter()
    d = driven(nbx, precision, k, perm)
    for call, row in enumerate(d["rows"]):
        assert {key: row["clock"][key] for key in CLOCK_KEYS} == row["ref"], (precision, k, perm, call, row["clock"], row["ref"])
        assert row["clock"]["steps"] == call + 1 and row["clock"]["dt_last"] == row["h"] and not row["clock"]["done"]
        assert row["round_trip"], (precision, k, perm, call)  # the restatement's state
        assert row["fixed"], (precision, k, perm, call)       # hermite_step(dt_last, 1, resume) on a third context
    same, clock = d["one_call"]
    assert same and clock == d["clock"], (precision, k, perm, clock, d["clock"])  # one call of all the steps
    print("fp%d k = %d perm %d: steps 2^%s, decided by %s, %.2f s (calls %s, one call %.2f s)" % (
        precision, k, perm, d["exponents"], d["deciders"], time.perf_counter() - t0, ["%.2f" % t for t in d["times"]], d["one_call_time"]))


def _plants():
    return [(k, p) for k in (33, 81) for p in plant_sites(k)]


@pytest.mark.parametrize("k,p", _plants())
@pytest.mark.parametrize("precision", [32, 64])
def test_a_planted_body_at_a_high_index_decides_the_first_step(nbx, precision, k, p):
    n = k ** 3
    columns = FR.field_shape(n, n)[0]
    assert 0 < p < n and (p == n - 1 or p == (columns - 1) * FR.COL or p > 1 << 16) and (k == 33 or 518399 % 256 == 255)
    d = driven(nbx, precision, k, False, plant=p, steps=1, full=False)
    # on the restatement's values: p is the argmin, and the minimum without it has another k_crit
    start = d["start"]
    assert int(np.argmin(start)) == p and not np.isnan(start).any(), (int(np.argmin(start)), p)
    with_p, without = A.k_crit(A.minimum(start), ETA * ETA), A.k_crit(A.minimum(np.delete(start, p)), ETA * ETA)
    assert with_p != without and K_CAP - LEVELS < with_p < without, (with_p, without)
    plain = A.k_crit(A.minimum(driven(nbx, precision, k)["start"]), ETA * ETA)  # the lattice without a planted body
    row, = d["rows"]
    assert {key: row["clock"][key] for key in CLOCK_KEYS} == row["ref"], (precision, k, p, row["clock"], row["ref"])
    assert row["clock"]["dt_last"] == 2.0 ** with_p and row["round_trip"], (precision, k, p, row["clock"])
    print("fp%d k = %d plant %d: k_crit %d, without it %d, the plain lattice %d; after the step decided by %d" % (
        precision, k, p, with_p, without, plain, d["deciders"][1]))


def _member(down, k):
    return {f: down[f][k] for f in H.POS + H.VEL}


def lone(nbx, precision, name, st):
    """(state after hermite_step(MEMBER_H, 2), state and clock after advance(max_steps=3)) of a default context holding st."""
    def make():
        with nbx.Context(len(st["mass"]), precision) as c:
            c.upload(st)
            c.hermite_step(MEMBER_H, 2)
            fixed = c.download()
            c.upload(st)
            _adv(c, max_steps=3)
            return fixed, c.download(), c.clock()
    return cached(("lone", precision, name), make)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_largest_member_alone_and_between_small_ones_ends_where_a_lone_context_ends(nbx, precision):
    k = MEMBER_K[precision]
    n = k ** 3
    assert FR.field_shape(n, n) == SHAPES[k] and [FR.field_shape(m, m)[2] for m in SMALL_MEMBERS] == [1, 8]
    sizes = (SMALL_MEMBERS[0], n, SMALL_MEMBERS[1])
    states = [R.make_state(precision, sizes[0], "cloud"), state(precision, k), R.make_state(precision, sizes[2], "cloud")]
    want = [lone(nbx, precision, ("member", m), s) for m, s in zip(sizes, states)]
    t0 = time.perf_counter()
    with nbx.Ensemble(n, 1, precision) as e:
        e.upload([states[1]])
        e.hermite_step(MEMBER_H, 2)
        assert H.same(_member(e.download(), 0), want[1][0]), precision
        e.upload([states[1]])
        _adv(e, max_steps=3)
        assert H.same(_member(e.download(), 0), want[1][1]) and e.clock() == [want[1][2]], (precision, e.clock(), want[1][2])
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        r.hermite_step(MEMBER_H, 2)
        for m, (down, w) in enumerate(zip(r.download(), want)):
            assert H.same(down, w[0]), (precision, m)
        r.upload(states)
        _adv(r, max_steps=3)
        clocks = r.clock()
        for m, (down, w) in enumerate(zip(r.download(), want)):
            assert H.same(down, w[1]) and clocks[m] == w[2], (precision, m, clocks[m], w[2])
    assert all(c["steps"] == 3 and c["floor_steps"] == 0 and not c["done"] for c in clocks), clocks
    record(case="members", precision=precision, sizes=sizes, shape=FR.field_shape(n, n), exponents=[A.exponent(c["dt_last"]) for c in clocks],
           seconds=round(time.perf_counter() - t0, 3))


def many_states(precision):
    """1025 systems of five bodies, the families cycled; the members of "grid" and "rest" shifted by a velocity of their own
    (jerk_ref.shifted: exact), so that copies of one family end at different states -- the shifted members at rest still have
    J = 0.  Members that alias modulo 256 (0, 256, 1024; 255, 1023; 1, 257) are of different families."""
    def make():
        out = []
        for m in range(MANY[0]):
            fam = R.FAMILIES[m % len(R.FAMILIES)]
            st = R.make_state(precision, MANY[1], fam)
            if fam in ("grid", "rest"):
                st = R.shifted(st, tuple(w * (m // len(R.FAMILIES)) for w in MANY_SHIFT))
            out.append(st)
        return out
    return cached(("many", precision), make)


@pytest.mark.parametrize("precision", [32, 64])
def test_an_ensemble_of_1025_systems_of_five_bodies_keeps_1025_clocks_apart(nbx, precision):
    members, n = MANY
    states = many_states(precision)
    t0 = time.perf_counter()
    with nbx.Ensemble(n, members, precision) as e, nbx.Ensemble(n, members, precision) as s:
        e.upload(states)
        _adv(e, max_steps=MANY_STEPS)
        down, clocks = e.download(), e.clock()
        assert len(clocks) == members
        for first, count in ((0, 1), (members - 1, 1), (255, 3)):
            assert e.clock(first, count) == clocks[first:first + count], (first, count)
        s.upload(states)  # the same six steps one call at a time: the sum of every member's steps
        total = np.zeros(members)
        for call in range(MANY_STEPS):
            _adv(s, resume=call > 0)
            total += np.array([c["dt_last"] for c in s.clock()])  # exact: powers of two within 40 levels of one another
        assert s.clock() == clocks and all(H.same(_member(down, m), _member(s.download(), m)) for m in MANY_PROBED)
    for m, c in enumerate(clocks):
        assert c["steps"] == MANY_STEPS and c["t"] == total[m] and c["n"] == n and not c["done"], (m, c, total[m])
    for m in MANY_PROBED:
        with nbx.Context(n, precision) as c:
            c.upload(states[m])
            _adv(c, max_steps=MANY_STEPS)
            assert H.same(_member(down, m), c.download()) and clocks[m] == c.clock(), (precision, m, clocks[m], c.clock())
    for group in ((0, 256, 1024), (255, 1023), (1, 257)):  # records k & 255 would hold another family's clock
        assert len({(clocks[m]["t"], clocks[m]["dt_next"]) for m in group}) == len(group), [clocks[m] for m in group]
    record(case="many", precision=precision, shape=[members, n], exponents=sorted({A.exponent(c["dt_last"]) for c in clocks}),
           seconds=round(time.perf_counter() - t0, 3))
