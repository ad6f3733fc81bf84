"""Adaptive power-of-two time steps chosen on the device (include/nbx_advance.h) against the numpy restatement of its criterion and
quantiser (tests/advance_ref.py) fed by the device's own evaluations, and against the fixed Hermite stepper driven with the same
sequence of steps; as a context, as members of an ensemble and as members of one ragged ensemble, in fp32 and fp64.

Everything is asked bit for bit: after every call the clock is the restatement's, the state is what the round trip of public calls
(jerk, host predictor, upload, jerk, host corrector: hermite_ref) leaves with the restatement's steps, and what
hermite_step(dt_last, 1, resume) leaves on a second context; one call of six steps is six calls of one; a member ends where a lone
context holding its state ends, with the same clock.

dt_cap = 2^-4, levels = 24, eta = 0.125, jerk_ref.make_state.  Shapes, the smallest at which each part can go wrong: n = 1 (no
criterion: the cap), 2, 5 (the step shrinks 2^-6 -> 2^-8), 257 (one column, two tiles with 255 padding records; cloud and
clustered), 513 (a second column of one body), 2049 (five columns, two splits; cloud, whose step doubles, and clustered), 4097 (nine
columns, four splits, the last one short), an ensemble of 3 x 2049 and a ragged ensemble of (5, 2049, 257, 1, 513).

The chosen step depends on the last bit of a candidate only where eta^2 q sits on a power of four; the tests check, on the
restatement's values alone, that every case stays 1e-9 (relative) away from one wherever the choice is not decided by the clamp.

The clamp and the degenerate candidates, in the second half of this module, all with dt_cap = 2^-4 and eta = 0.125, bit for bit
against advance_ref.run fed by the device's evaluations: floors that bind (levels = 0, 2, 3, 8; floor_steps counted once the step
is taken, across a resumed call, per member, kept by a member that is done while others go on), systems at rest (every start
candidate +inf, dt_cap first, then a drop of several levels at once), +inf candidates beside finite ones (a massless body's
partner; a coincident pair), and a member whose candidates are all NaN or +inf.  tests/test_large_steppers_cpu.py shows on the CPU
which planted faults these cases see that the ones above do not.  The shapes above n = 4097 -- 15 splits, 2076 tiles, 1025
clocks, a minimum decided by the last candidate of 531 441 -- live in tests/test_large_steppers_gpu.py."""
import math
import os
import sys

import numpy as np
import pytest

import advance_ref as A
import hermite_ref as H
import jerk_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

K_CAP, LEVELS, ETA = -4, 24, 0.125
DT_CAP = 2.0 ** K_CAP
FAR = 1.0  # a t_end six steps do not reach, whatever their size
CALLS = 6
CASES = ((1, "cloud"), (2, "cloud"), (5, "cloud"), (257, "cloud"), (257, "clustered"), (513, "cloud"), (2049, "cloud"), (2049, "clustered"),
         (4097, "cloud"))
ENSEMBLE = (("cloud", 2049), ("clustered", 2049), ("grid", 2049))
RAGGED = (5, 2049, 257, 1, 513)
CLOCK_KEYS = ("n", "t", "dt_last", "dt_next", "steps", "floor_steps", "done")
_driven, _lone = {}, {}


def _adv(o, t_end=FAR, max_steps=1, resume=False, eta=ETA, dt_cap=DT_CAP, levels=LEVELS):
    o.advance(t_end, dt_cap, eta, levels, max_steps, resume)


def _check_boundary(x):
    """eta^2 q of the restatement: where k_crit lies inside [k_floor, k_cap + 1] it is 1e-9 away from every power of four."""
    if math.isfinite(x) and x > 0.0 and K_CAP - LEVELS <= A.k_crit(x, 1.0) <= K_CAP + 1:
        assert A.boundary_distance(x) >= 1e-9, x


def driven(nbx, precision, n, family):
    """CALLS calls of advance(max_steps=1), resumed after the first, on one context; beside it the restatement, its evaluations
    the device's own (upload, jerk on a second context), and a third context driven by hermite_step with the restatement's steps.
    Per call: the device's clock, the restatement's, and whether the three states are the same bits.  Computed once per case."""
    key = (precision, n, family)
    if key in _driven:
        return _driven[key]
    st = R.make_state(precision, n, family)
    rows = []
    with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b, nbx.Context(n, precision) as c:
        a.upload(st)
        c.upload(st)
        ref = None
        for call in range(CALLS):
            _adv(a, resume=call > 0)
            if ref is None:
                ref = A.run(st, precision, FAR, K_CAP, LEVELS, ETA, 1, H.device_evaluate(b))
                _check_boundary(ETA * ETA * A.minimum(A.start_candidates(*H.device_evaluate(b)(st))))
            else:
                ref = A.run(ref["state"], precision, FAR, K_CAP, LEVELS, ETA, 1, H.device_evaluate(b), clock=ref["clock"], carry=ref["carry"])
            (_, h, x), = ref["history"]
            _check_boundary(x)
            c.hermite_step(h, 1, resume=call > 0)
            got = a.download()
            rows.append({"clock": a.clock(), "ref": A.public(ref["clock"], FAR, n), "h": h, "round_trip": H.same(got, ref["state"]),
                         "fixed": H.same(got, c.download()), "moved": not H.same(got, st)})
        _driven[key] = {"rows": rows, "state": got, "clock": rows[-1]["clock"], "steps": [r["h"] for r in rows]}
    return _driven[key]


def lone(nbx, precision, n, family, t_end=FAR, max_steps=CALLS):
    """(state, clock) of a default context of n bodies holding the family's state after advance(t_end, max_steps): what a member is
    held to."""
    key = (precision, n, family, t_end, max_steps)
    if key not in _lone:
        with nbx.Context(n, precision) as c:
            c.upload(R.make_state(precision, n, family))
            _adv(c, t_end, max_steps)
            _lone[key] = (c.download(), c.clock())
    return _lone[key]


@pytest.mark.parametrize("n,family", CASES)
@pytest.mark.parametrize("precision", [32, 64])
def test_step_by_step_the_clock_is_the_restatements_and_the_state_is_the_fixed_steppers(nbx, precision, n, family):
    d = driven(nbx, precision, n, family)
    for call, row in enumerate(d["rows"]):
        assert {k: row["clock"][k] for k in CLOCK_KEYS} == row["ref"], (precision, n, family, call, row["clock"], row["ref"])
        assert row["clock"]["steps"] == call + 1 and row["clock"]["dt_last"] == row["h"] and not row["clock"]["done"]
        assert row["round_trip"], (precision, n, family, call)  # the round trip of public calls with the restatement's steps
        assert row["fixed"], (precision, n, family, call)       # hermite_step(dt_last, 1, resume) on a second context
        assert row["moved"] or n == 1, (precision, n, family, call)
    print("fp%d n = %d %s: steps 2^%s, next 2^%d" % (precision, n, family, [A.exponent(h) for h in d["steps"]], A.exponent(d["clock"]["dt_next"])))


@pytest.mark.parametrize("precision", [32, 64])
def test_the_reference_histories_hold_shrinking_and_doubling_steps(nbx, precision):
    """On the restatement's values: n = 5 shrinks from 2^-6 to 2^-8, 2049 bodies of the cloud double (2^-12 -> 2^-11) and come back."""
    steps = {case: [A.exponent(h) for h in driven(nbx, precision, *case)["steps"]] for case in ((5, "cloud"), (2049, "cloud"))}
    assert steps[(5, "cloud")][0] == -6 and steps[(5, "cloud")][-1] == -8, steps
    assert any(b == a + 1 for a, b in zip(steps[(2049, "cloud")], steps[(2049, "cloud")][1:])), steps
    assert any(b < a for s in steps.values() for a, b in zip(s, s[1:])), steps


@pytest.mark.parametrize("n,family", CASES)
@pytest.mark.parametrize("precision", [32, 64])
def test_one_call_of_six_steps_is_six_calls_of_one(nbx, precision, n, family):
    d = driven(nbx, precision, n, family)
    state, clock = lone(nbx, precision, n, family)
    assert H.same(state, d["state"]) and clock == d["clock"], (precision, n, family, clock, d["clock"])


@pytest.mark.parametrize("precision", [32, 64])
def test_every_member_of_an_ensemble_and_of_a_ragged_ensemble_ends_where_a_lone_context_ends_with_its_clock(nbx, precision):
    n = ENSEMBLE[0][1]
    with nbx.Ensemble(n, len(ENSEMBLE), precision) as e:
        e.upload([R.make_state(precision, m, fam) for fam, m in ENSEMBLE])
        _adv(e, max_steps=CALLS)
        down, clocks = e.download(), e.clock()
        for k, (fam, m) in enumerate(ENSEMBLE):
            state, clock = lone(nbx, precision, m, fam)
            assert H.same({f: down[f][k] for f in H.POS + H.VEL}, state) and clocks[k] == clock, (precision, k, fam, clocks[k], clock)
        assert e.clock(1, 1) == clocks[1:2]
    # the members' steps differ from one another -- on the restatement: the last steps taken, and the next ones (2^-12, 2^-14, 2^-12)
    refs = [driven(nbx, precision, m, fam)["rows"][-1]["ref"] for fam, m in ENSEMBLE]
    assert len({r["dt_last"] for r in refs}) == len(ENSEMBLE), refs
    assert [r["dt_next"] for r in refs] == [2.0 ** -12, 2.0 ** -14, 2.0 ** -12], refs
    with nbx.Ragged(RAGGED, precision) as r:
        r.upload([R.make_state(precision, m, "cloud") for m in RAGGED])
        _adv(r, max_steps=2)
        _adv(r, max_steps=CALLS - 2, resume=True)
        clocks = r.clock()
        for k, (m, down) in enumerate(zip(RAGGED, r.download())):
            state, clock = lone(nbx, precision, m, "cloud")
            assert H.same(down, state) and clocks[k] == clock, (precision, k, m, clocks[k], clock)
        assert len({c["dt_last"] for c in clocks}) >= 3


def _snapshot(o):
    return o.download(), o.clock()


def _same_snapshot(a, b):
    (sa, ca), (sb, cb) = a, b
    states = all(H.same(x, y) for x, y in zip(sa, sb)) if isinstance(sa, list) else H.same(sa, sb)
    return states and ca == cb


@pytest.mark.parametrize("precision", [32, 64])
def test_a_system_lands_on_t_end_exactly_stops_there_and_carries_on_towards_a_larger_one(nbx, precision):
    n, st = 5, R.make_state(precision, 5, "cloud")
    with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b:
        a.upload(st)
        _adv(a, DT_CAP, 0)  # no step yet: the clock is set, dt_next can be asked for
        ref = A.run(st, precision, DT_CAP, K_CAP, LEVELS, ETA, 0, H.device_evaluate(b))
        assert {k: a.clock()[k] for k in CLOCK_KEYS} == A.public(ref["clock"], DT_CAP, n) and a.clock()["steps"] == 0 and a.clock()["dt_last"] == 0.0
        assert H.same(a.download(), st)
        _adv(a, DT_CAP, 32)
        ref = A.run(st, precision, DT_CAP, K_CAP, LEVELS, ETA, 32, H.device_evaluate(b))
        for _, _, x in ref["history"]:
            _check_boundary(x)
        end = _snapshot(a)
        clock = end[1]
        assert clock["done"] and clock["t"] == DT_CAP and clock["steps"] == ref["clock"]["steps"] == len(ref["history"]) < 32
        assert {k: clock[k] for k in CLOCK_KEYS} == A.public(ref["clock"], DT_CAP, n) and H.same(end[0], ref["state"])
        print("fp%d n = 5: %d steps to dt_cap (the prototype: 11)" % (precision, clock["steps"]))
        _adv(a, DT_CAP, 8, resume=True)  # done: 24 launches that change no bit
        assert _same_snapshot(_snapshot(a), end)
        _adv(a, 2 * DT_CAP, 4, resume=True)  # a larger t_end: it moves on
        more = A.run(ref["state"], precision, 2 * DT_CAP, K_CAP, LEVELS, ETA, 4, H.device_evaluate(b), clock=ref["clock"], carry=ref["carry"])
        got = _snapshot(a)
        assert {k: got[1][k] for k in CLOCK_KEYS} == A.public(more["clock"], 2 * DT_CAP, n) and H.same(got[0], more["state"])
        assert got[1]["steps"] == clock["steps"] + 4 and got[1]["t"] > DT_CAP and not got[1]["done"]
    # an ensemble whose members finish at different steps: the early finisher stays put while the other still steps
    with nbx.Ensemble(5, 2, precision) as e:
        e.upload([R.make_state(precision, 5, "cloud"), R.make_state(precision, 5, "clustered")])
        _adv(e, DT_CAP, 20)
        down, clocks = e.download(), e.clock()
        assert clocks[0]["done"] and clocks[0]["steps"] == clock["steps"] and not clocks[1]["done"] and clocks[1]["steps"] == 20
        for k, fam in enumerate(("cloud", "clustered")):
            state, want = lone(nbx, precision, 5, fam, DT_CAP, 20)
            assert H.same({f: down[f][k] for f in H.POS + H.VEL}, state) and clocks[k] == want, (precision, k, clocks[k], want)
        assert H.same({f: down[f][0] for f in H.POS + H.VEL}, end[0]) and clocks[0] == end[1]


def _refused(nbx, call, text):
    with pytest.raises(nbx.NbxError) as err:
        call()
    assert err.value.code == nbx.NBX_ERR_STATE and text in str(err.value), str(err.value)


@pytest.mark.parametrize("precision", [32, 64])
def test_resume_is_refused_where_the_promise_is_seen_to_be_broken(nbx, precision):
    s5, s3 = R.make_state(precision, 5, "cloud"), R.make_state(precision, 3, "cloud")
    with nbx.Context(5, precision) as c, nbx.Ensemble(5, 2, precision) as e, nbx.Ragged([5, 3], precision) as r:
        for o, up in ((c, lambda: c.upload(s5)), (e, lambda: e.upload([s5, s5])), (r, lambda: r.upload([s5, s3]))):
            up()
            _refused(nbx, lambda: _adv(o, resume=True), "resume without a previous advance call")
            _refused(nbx, lambda: o.clock(), "no advance call has been made")
            _adv(o, max_steps=0, resume=False)  # the evaluation alone is a call to carry on from
            _adv(o, resume=True)
            up()
            _refused(nbx, lambda: _adv(o, resume=True), "resume after an upload")
            _adv(o)
            o.step(1, kenergy=False)
            _refused(nbx, lambda: _adv(o, resume=True), "resume after a step")
            _adv(o)
            o.kick(0.01)
            _refused(nbx, lambda: _adv(o, resume=True), "resume after a step or a kick")
            _adv(o)
            o.hermite_step(2.0 ** -10, 1)
            _refused(nbx, lambda: _adv(o, resume=True), "resume after a fixed Hermite step")
            _adv(o)
            _refused(nbx, lambda: o.hermite_step(2.0 ** -10, 1, resume=True), "resume without a previous Hermite call")  # the fixed stepper's text
            _refused(nbx, lambda: _adv(o, resume=True, dt_cap=DT_CAP / 2), "resume with another dt_cap or levels")
            _refused(nbx, lambda: _adv(o, resume=True, levels=LEVELS - 1), "resume with another dt_cap or levels")
            _adv(o, resume=True, eta=ETA / 2)  # eta may change
            _adv(o, max_steps=0, resume=True)  # nothing launched
            with pytest.raises(nbx.NbxError) as err:
                _adv(o, t_end=FAR + DT_CAP / 2, resume=True)
            assert err.value.code == nbx.NBX_ERR_ARG and "whole multiple of dt_cap" in str(err.value)
    with nbx.Context(5, 32) as c:
        c.upload(R.make_state(32, 5, "cloud"))
        with pytest.raises(nbx.NbxError) as err:
            _adv(c, t_end=2.0 ** -130, dt_cap=2.0 ** -130)  # no normal fp32 value
        assert err.value.code == nbx.NBX_ERR_ARG and "normal value of the object's precision" in str(err.value)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_same_call_gives_the_same_bits_and_analysis_calls_between_resumed_calls_change_nothing(nbx, precision):
    n = 513
    st = R.make_state(precision, n, "cloud")
    want = lone(nbx, precision, n, "cloud")
    with nbx.Context(n, precision) as a:
        for _ in range(2):  # the same call twice from the same upload
            a.upload(st)
            _adv(a, max_steps=CALLS)
            assert _same_snapshot(_snapshot(a), want), precision
        a.upload(st)
        before = a.stats()
        _adv(a, max_steps=3)
        mid = _snapshot(a)
        j = a.jerk()
        a.field(st["pos_x"][:9], st["pos_y"][:9], st["pos_z"][:9])
        a.diagnostics()
        a.neighbours()
        a.timescale()
        assert H.same(a.jerk(), j, R.KEYS) and _same_snapshot(_snapshot(a), mid)
        _adv(a, max_steps=CALLS - 3, resume=True)
        assert _same_snapshot(_snapshot(a), want), precision
        assert a.stats()["steps_done"] == before["steps_done"] and a.step(0) == 0.0  # not counted; the partials belong to no state
    with nbx.Ragged([n, 5], precision) as r:
        r.upload([st, R.make_state(precision, 5, "cloud")])
        _adv(r, max_steps=3)
        r.jerk()
        r.field(*[np.tile(st[f][:9], (2, 1)) for f in H.POS])
        r.diagnostics()
        _adv(r, max_steps=CALLS - 3, resume=True)
        assert H.same(r.download()[0], want[0]) and r.clock()[0] == want[1], precision


# ---- the clamp, the cold start, candidates that are not finite ---------------------------------------------------------------------
# (n, family, levels, steps, the exponents of the steps, floor_steps after them): jerk_ref.direct gives these histories in both
# precisions with every x at least 0.012 from a power of four (tests/test_large_steppers_cpu.py); here they are asserted on the
# restatement fed by the device's own evaluations, and the device's clock against that.
FLOOR_CASES = ((5, "cloud", 2, 8, [-6] * 8, 7), (5, "cloud", 3, 16, [-6] + [-7] * 15, 13), (5, "cloud", 0, 3, [-4] * 3, 3),
               (257, "clustered", 8, 6, [-12] * 6, 6))
FLOOR_LEVELS = 3  # of the member cases
FLOOR_ENSEMBLE = ((5, "cloud"), (5, "clustered"))
FLOOR_RAGGED = ((5, "cloud"), (257, "clustered"), (1, "cloud"))
FLOOR_MAX_STEPS = 12  # more than the 8 steps of 2^-7 that reach dt_cap: the launches of the last ones find members that are done
COLD_SIZES = (5, 257, 2049)
COLD_RAGGED = ((5, "rest"), (257, "cloud"), (257, "rest"))
_solo = {}


def degenerate_states(precision):
    """{name: state}.  massless: two bodies, body 0 without mass -- body 1 feels nothing, a = j = 0, its candidate +inf at the
    start and after every step (a zero denominator), body 0 decides.  coincident: three bodies, 0 and 1 at one position with one
    velocity -- the softening keeps every value finite.  coincident massless: the same with body 2 without mass -- the pair feels
    nothing (d = 0, u = 0 between its two), so two candidates are +inf and body 2 decides."""
    two = R.make_state(precision, 2, "cloud")
    two["mass"][0] = 0
    three = R.make_state(precision, 3, "cloud")
    for f in H.POS + H.VEL:
        three[f][1] = three[f][0]
    light = {k: v.copy() for k, v in three.items()}
    light["mass"][2] = 0
    return {"massless": two, "coincident": three, "coincident massless": light}


def _check_every_x(history):
    for _, _, x in history:
        assert not (math.isfinite(x) and x > 0.0) or A.boundary_distance(x) >= 1e-9, x


def solo(nbx, precision, name, state, levels, max_steps, t_end=FAR, first=None):
    """A context holding `state` after advance(t_end, levels, max_steps) -- as one call, or as a call of `first` steps and a resumed
    one of the rest -- beside the restatement fed by the device's own evaluations on a second context.  Asserts that clock and
    state are the restatement's after every call; returns {"state", "clock", "ref", "start"}, start the restatement's start
    candidates.  Computed once."""
    key = (precision, name, levels, max_steps, t_end, first)
    if key in _solo:
        return _solo[key]
    n = len(state["mass"])
    with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b:
        ev = H.device_evaluate(b)
        start = A.start_candidates(*ev(state))
        a.upload(state)
        parts = [max_steps] if first is None else [first, max_steps - first]
        ref, history = None, []
        for call, steps in enumerate(parts):
            _adv(a, t_end, steps, resume=call > 0, levels=levels)
            ref = A.run(state if ref is None else ref["state"], precision, t_end, K_CAP, levels, ETA, steps, ev,
                        clock=ref and ref["clock"], carry=ref and ref["carry"])
            history += ref["history"]
            got, clock = a.download(), a.clock()
            assert {k: clock[k] for k in CLOCK_KEYS} == A.public(ref["clock"], t_end, n), (precision, name, levels, call, clock, ref["clock"])
            assert H.same(got, ref["state"]), (precision, name, levels, call)
    _check_every_x(history)
    _solo[key] = {"state": got, "clock": clock, "ref": dict(ref, history=history), "start": start}
    return _solo[key]


@pytest.mark.parametrize("n,family,levels,steps,exponents,floor_steps", FLOOR_CASES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_floor_that_binds_is_counted_once_the_step_is_taken_in_one_call_and_across_a_resumed_one(nbx, precision, n, family, levels, steps,
                                                                                                  exponents, floor_steps):
    st = R.make_state(precision, n, family)
    whole = solo(nbx, precision, (n, family), st, levels, steps)
    seam = solo(nbx, precision, (n, family), st, levels, steps, first=2)  # the floor_next the first call leaves is taken in the second
    for d in (whole, seam):
        assert [A.exponent(h) for _, h, _ in d["ref"]["history"]] == exponents and d["ref"]["clock"]["floor_steps"] == floor_steps, d["ref"]
        assert d["clock"]["floor_steps"] == floor_steps and d["clock"]["steps"] == steps and not d["clock"]["done"]
        assert d["clock"]["dt_next"] == 2.0 ** (K_CAP - levels)  # every case ends at its floor
    assert H.same(whole["state"], seam["state"]) and whole["clock"] == seam["clock"]
    print("fp%d n = %d %s levels %d: steps 2^%s, floor_steps %d" % (precision, n, family, levels, exponents, floor_steps))


@pytest.mark.parametrize("precision", [32, 64])
def test_one_floor_case_counts_some_of_its_steps_and_not_all(nbx, precision):
    counts = [(solo(nbx, precision, (n, fam), R.make_state(precision, n, fam), levels, steps)["ref"]["clock"]["floor_steps"], steps)
              for n, fam, levels, steps, _, _ in FLOOR_CASES]
    assert any(0 < f < s for f, s in counts) and any(f == s for f, s in counts), counts


@pytest.mark.parametrize("precision", [32, 64])
def test_every_member_carries_its_own_floor_steps_and_keeps_them_once_it_is_done(nbx, precision):
    """levels = 3, t_end = dt_cap, 12 steps asked: every member reaches t_end at the floor (2^-7) or, alone of its kind, at dt_cap
    (n = 1); the launches of the steps that follow find it done and must leave its count alone while the others go on."""
    def want(n, fam):
        return solo(nbx, precision, (n, fam), R.make_state(precision, n, fam), FLOOR_LEVELS, FLOOR_MAX_STEPS, t_end=DT_CAP)

    with nbx.Ensemble(5, len(FLOOR_ENSEMBLE), precision) as e:
        e.upload([R.make_state(precision, n, fam) for n, fam in FLOOR_ENSEMBLE])
        _adv(e, DT_CAP, FLOOR_MAX_STEPS, levels=FLOOR_LEVELS)
        down, clocks = e.download(), e.clock()
        for k, (n, fam) in enumerate(FLOOR_ENSEMBLE):
            w = want(n, fam)
            assert H.same({f: down[f][k] for f in H.POS + H.VEL}, w["state"]) and clocks[k] == w["clock"], (precision, k, clocks[k], w["clock"])
    with nbx.Ragged([n for n, _ in FLOOR_RAGGED], precision) as r:
        r.upload([R.make_state(precision, n, fam) for n, fam in FLOOR_RAGGED])
        _adv(r, DT_CAP, 2, levels=FLOOR_LEVELS)
        _adv(r, DT_CAP, FLOOR_MAX_STEPS - 2, resume=True, levels=FLOOR_LEVELS)
        ragged = r.clock()
        for k, ((n, fam), down) in enumerate(zip(FLOOR_RAGGED, r.download())):
            w = want(n, fam)
            assert H.same(down, w["state"]) and ragged[k] == w["clock"], (precision, k, ragged[k], w["clock"])
    # on the restatement: all done, at different steps, with different counts; the first to finish has a count to keep
    refs = [want(n, fam)["ref"]["clock"] for n, fam in FLOOR_ENSEMBLE + FLOOR_RAGGED[1:]]
    assert all(c["t"] == DT_CAP and c["steps"] < FLOOR_MAX_STEPS for c in refs), refs
    assert refs[0]["steps"] < refs[1]["steps"] and 0 < refs[0]["floor_steps"] < refs[1]["floor_steps"] and refs[0]["floor_next"], refs
    assert (refs[-1]["steps"], refs[-1]["floor_steps"], refs[-1]["dt_last"]) == (1, 0, DT_CAP), refs[-1]  # n = 1
    assert clocks[0]["floor_steps"] == refs[0]["floor_steps"] and ragged[2]["floor_steps"] == 0 and all(c["done"] for c in clocks + ragged)
    print("fp%d: steps %s, floor_steps %s" % (precision, [c["steps"] for c in refs], [c["floor_steps"] for c in refs]))


@pytest.mark.parametrize("n", COLD_SIZES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_system_at_rest_starts_at_dt_cap_and_shrinks_by_many_levels_at_once(nbx, precision, n):
    """Six calls of one step from rest.  J is exactly 0 at the start, every start candidate +inf, so the first step is dt_cap
    whatever it costs; the criterion then sees the jerk and drops the step by several levels in one go (jerk_ref.direct,
    n = 257: 2^-4, 2^-10, 2^-16, 2^-17)."""
    st = R.make_state(precision, n, "rest")
    d = driven_from(nbx, precision, ("rest", n), st)
    exps = [A.exponent(h) for h in d["steps"]]
    assert np.isposinf(d["start"]).all() and len(d["start"]) == n and exps[0] == K_CAP, (exps, d["start"])
    assert n == 5 or any(b < a - 1 for a, b in zip(exps, exps[1:])), exps  # five bodies are slow enough for one level at a time
    assert min(exps) > K_CAP - LEVELS  # the floor does not hide it
    for call, row in enumerate(d["rows"]):
        assert {k: row["clock"][k] for k in CLOCK_KEYS} == row["ref"], (precision, n, call, row["clock"], row["ref"])
        assert row["round_trip"] and row["fixed"] and row["moved"], (precision, n, call)
    print("fp%d n = %d at rest: steps 2^%s, next 2^%d" % (precision, n, exps, A.exponent(d["clock"]["dt_next"])))


def driven_from(nbx, precision, name, st):
    """driven() for a state that is no family of a CASES entry, with the start candidates of the restatement."""
    key = (precision,) + name
    if key not in _driven:
        n = len(st["mass"])
        rows, ref = [], None
        with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b, nbx.Context(n, precision) as c:
            ev = H.device_evaluate(b)
            start = A.start_candidates(*ev(st))
            _check_boundary(ETA * ETA * A.minimum(start))
            a.upload(st)
            c.upload(st)
            for call in range(CALLS):
                _adv(a, resume=call > 0)
                ref = A.run(st if ref is None else ref["state"], precision, FAR, K_CAP, LEVELS, ETA, 1, ev, clock=ref and ref["clock"],
                            carry=ref and ref["carry"])
                (_, h, x), = ref["history"]
                _check_boundary(x)
                c.hermite_step(h, 1, resume=call > 0)
                got = a.download()
                rows.append({"clock": a.clock(), "ref": A.public(ref["clock"], FAR, n), "h": h, "round_trip": H.same(got, ref["state"]),
                             "fixed": H.same(got, c.download()), "moved": not H.same(got, st)})
        _driven[key] = {"rows": rows, "state": got, "clock": rows[-1]["clock"], "steps": [r["h"] for r in rows], "start": start}
    return _driven[key]


@pytest.mark.parametrize("precision", [32, 64])
def test_members_at_rest_beside_a_moving_one_end_where_lone_contexts_end(nbx, precision):
    states = [R.make_state(precision, n, fam) for n, fam in COLD_RAGGED]
    with nbx.Ragged([n for n, _ in COLD_RAGGED], precision) as r:
        r.upload(states)
        _adv(r, max_steps=CALLS)
        clocks = r.clock()
        for k, ((n, fam), down) in enumerate(zip(COLD_RAGGED, r.download())):
            w = solo(nbx, precision, (n, fam), states[k], LEVELS, CALLS)
            assert H.same(down, w["state"]) and clocks[k] == w["clock"], (precision, k, clocks[k], w["clock"])
            assert np.isposinf(w["start"]).all() == (fam == "rest")
    assert clocks[0]["t"] != clocks[2]["t"] and clocks[1]["t"] != clocks[2]["t"]


@pytest.mark.parametrize("name", ["massless", "coincident", "coincident massless"])
@pytest.mark.parametrize("precision", [32, 64])
def test_candidates_that_are_infinite_beside_finite_ones_leave_the_finite_ones_to_decide(nbx, precision, name):
    """On the restatement: the massless cases hold +inf candidates next to a finite minimum, at the start and after every step
    (a body that feels nothing has a zero denominator); the coincident pair with masses has none -- no pair of it is at rest
    relative to a third body -- and every one of its values is finite, which is what the softening is for."""
    st = degenerate_states(precision)[name]
    n = len(st["mass"])
    d = solo(nbx, precision, name, st, LEVELS, 3)
    start = d["start"]
    infinite = {"massless": [1], "coincident": [], "coincident massless": [0, 1]}[name]
    assert np.flatnonzero(np.isposinf(start)).tolist() == infinite and not np.isnan(start).any(), start
    assert math.isfinite(A.minimum(start)) and int(np.argmin(start)) not in infinite
    assert all(math.isfinite(x) and x > 0.0 for _, _, x in d["ref"]["history"]), d["ref"]["history"]  # a finite minimum after every step
    assert d["clock"]["steps"] == 3 and d["clock"]["floor_steps"] == 0 and 2.0 ** (K_CAP - LEVELS) < d["clock"]["dt_next"] <= DT_CAP
    assert all(np.isfinite(d["state"][f]).all() for f in H.POS + H.VEL)
    for i in infinite:  # the bodies that feel nothing keep their velocities: a1 = j1 = 0, so the denominator of the criterion is 0
        assert all(d["state"][v][i] == st[v][i] for v in H.VEL), (name, i)
    print("fp%d %s: start candidates %s, steps 2^%s" % (precision, name, start, [A.exponent(h) for _, h, _ in d["ref"]["history"]]))


@pytest.mark.parametrize("precision", [32, 64])
def test_a_member_whose_candidates_are_all_nan_or_infinite_steps_at_dt_cap_and_does_not_reach_the_member_before_it(nbx, precision):
    """The construction of tests/test_jerk_gpu.py: (inf, nan, -inf) in one velocity of the second member.  Every jerk of that
    member is a NaN, so every start candidate is +inf and every later one a NaN or +inf: q = +inf, never a NaN selected, three
    steps of dt_cap and no floor step.  Its state is unspecified and not compared; member 0 is a lone context's, bit for bit."""
    n = 513
    st = R.make_state(precision, n, "cloud")
    bad = {k: v.copy() for k, v in st.items()}
    bad["vel_x"][0], bad["vel_y"][0], bad["vel_z"][0] = np.inf, np.nan, -np.inf
    state, clock = lone(nbx, precision, n, "cloud", FAR, 3)
    want = {"t": 3 * DT_CAP, "dt_last": DT_CAP, "dt_next": DT_CAP, "steps": 3, "floor_steps": 0}
    with nbx.Ensemble(n, 2, precision) as e:
        e.upload([st, bad])
        _adv(e, max_steps=3)
        down, clocks = e.download(), e.clock()
        assert H.same({f: down[f][0] for f in H.POS + H.VEL}, state) and clocks[0] == clock, (precision, clocks[0], clock)
        assert {k: clocks[1][k] for k in want} == want, clocks[1]
    with nbx.Ragged([n, n], precision) as r:
        r.upload([st, bad])
        _adv(r, max_steps=3)
        clocks = r.clock()
        assert H.same(r.download()[0], state) and clocks[0] == clock, (precision, clocks[0], clock)
        assert {k: clocks[1][k] for k in want} == want, clocks[1]
    assert clock["dt_last"] < DT_CAP  # member 0's own steps are not the cap's: it did not take member 1's clock


def test_an_adaptive_step_costs_at_most_twice_the_fixed_step_where_the_step_is_launch_bound(nbx):
    """An ensemble of 64 x 256, fp32: per step, advance(max_steps=8, resume) with every step at dt_cap against
    hermite_step(dt_cap, 8, resume) on a second ensemble holding the same upload, in this process, arms alternated, the best of
    five rounds (tools/advance_cost.py).  Three launches against two: 1.5, and the rest of the 2.0 for the candidate write and
    timer noise."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import advance_cost
    r = advance_cost.measure(nbx, "ensemble", rounds=5)
    print("ensemble 64 x 256 fp32: advance %.1f us, hermite %.1f us per step, ratio %.4f; a finished object %.1f us per step" % (
        r["advance_us_per_step"], r["hermite_us_per_step"], r["ratio"], r["finished_us_per_step"]))
    advance_cost.write(advance_cost.OUT, {"ensemble": r})
    assert (r["systems"], r["n_min"], r["n_max"]) == (64, 256, 256)
    assert r["same_bits_from_both_arms"] and r["every_step_is_dt_cap"] and r["finished_object_is_done_and_stays"], r
    assert r["ratio"] <= 2.0, r
