"""The resident fourth-order Hermite stepper on the device (include/nbx_hermite.h) against the round trip of public calls it
replaces and the numpy restatement of its formulas (tests/hermite_ref.py), as a context, as members of an ensemble and as members
of one ragged ensemble, in fp32 and fp64.

Everything is asked bit for bit but the order of the scheme: a resident step leaves what jerk(), the host predictor, an upload,
jerk(), the host corrector and an upload leave; a resumed call continues the carried round trip; a member ends where a lone context
holding its state ends.

Shapes, the smallest at which each part can go wrong: n = 1, 2, 5; 257 (one column, two tiles with 255 padding records), 513 (a
second column of one body), 2049 (five columns, two splits), 4097 (nine columns, four splits, the last one short), an ensemble of
3 x 2049 and a ragged ensemble of (5, 2049, 257, 1, 513).  dt = 0.015 is no fp32 value (h is dt rounded to T) and is large enough
for every rounding of the scheme to show in the bits of a few hundred bodies (tests/test_hermite_cpu.py says why).

The larger shapes -- 71 columns x 15 splits, 1038 columns of one split walking 2076 tiles, the largest member a batch object holds
between small ones -- live in tests/test_large_steppers_gpu.py, held to the same round trip bit for bit."""
import os
import sys

import numpy as np
import pytest

import hermite_ref as H
import jerk_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

DT = 0.015
SIZES = (1, 2, 5, 257, 513, 2049, 4097)
FAMILIES = ("cloud", "grid")
ENSEMBLE = (("cloud", 2049), ("grid", 2049), ("clustered", 2049))
RAGGED = (5, 2049, 257, 1, 513)
_lone = {}


def lone_context(nbx, precision, n, family, steps=2):
    """Where a default context of n bodies holding the family's state is after hermite_step(DT, steps): what a member is held to."""
    key = (precision, n, family, steps)
    if key not in _lone:
        with nbx.Context(n, precision) as c:
            c.upload(R.make_state(precision, n, family))
            c.hermite_step(DT, steps)
            _lone[key] = c.download()
    return _lone[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", [32, 64])
def test_one_resident_step_is_the_round_trip_and_a_resumed_one_continues_it(nbx, precision, n):
    for family in FAMILIES:
        st = R.make_state(precision, n, family)
        with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b:
            a.upload(st)
            a.hermite_step(DT, 1)
            got = a.download()
            end, kept = H.round_trip(b, st, DT, 1)
            assert all(got[f].dtype == R.DTYPE[precision] and got[f].shape == (n,) for f in H.POS + H.VEL)
            assert H.same(got, end), (precision, n, family)
            assert H.same(b.download(), end)  # the round trip's last upload, read back
            if n > 1:
                assert not H.same(got, st), (precision, n, family)  # the bodies moved
            # the kept a, j are jerk()'s at the predicted state: a second, resumed step is the round trip carried on
            a.hermite_step(DT, 1, resume=True)
            end2, _ = H.round_trip(b, end, DT, 1, carry=kept)
            assert H.same(a.download(), end2), (precision, n, family)
            assert H.same(lone_context(nbx, precision, n, family), end2)  # and two steps in one call are the same two steps


@pytest.mark.parametrize("precision", [32, 64])
def test_every_member_of_an_ensemble_and_of_a_ragged_ensemble_ends_where_a_lone_context_ends(nbx, precision):
    n = ENSEMBLE[0][1]
    states = [R.make_state(precision, m, fam) for fam, m in ENSEMBLE]
    with nbx.Ensemble(n, len(ENSEMBLE), precision) as e:
        e.upload(states)
        e.hermite_step(DT, 1)
        e.hermite_step(DT, 1, resume=True)
        down = e.download()
        for k, (fam, m) in enumerate(ENSEMBLE):
            assert H.same({f: down[f][k] for f in H.POS + H.VEL}, lone_context(nbx, precision, m, fam)), (precision, k, fam)
    states = [R.make_state(precision, m, "cloud") for m in RAGGED]
    with nbx.Ragged(RAGGED, precision) as r:
        r.upload(states)
        r.hermite_step(DT, 2)
        for k, (m, down) in enumerate(zip(RAGGED, r.download())):
            assert H.same(down, lone_context(nbx, precision, m, "cloud")), (precision, k, m)
        # the round trip on the batch object itself: the members end to end are one state of the formulas
        with nbx.Ragged(RAGGED, precision) as t:
            end, _ = H.round_trip(t, H.joined(states), DT, 2)
        assert all(H.same(down, want) for down, want in zip(r.download(), H.parted(end, RAGGED, H.POS + H.VEL)))


def _refused(nbx, call, text):
    with pytest.raises(nbx.NbxError) as err:
        call()
    assert err.value.code == nbx.NBX_ERR_STATE and text in str(err.value), str(err.value)


@pytest.mark.parametrize("precision", [32, 64])
def test_several_steps_in_one_call_and_resume(nbx, precision):
    n = 2049
    st = R.make_state(precision, n, "cloud")
    with nbx.Context(n, precision) as a, nbx.Context(n, precision) as b, nbx.Context(n, precision) as c:
        a.upload(st)
        a.hermite_step(DT, 3)
        three = a.download()
        end3, kept = H.round_trip(b, st, DT, 3)
        assert H.same(three, end3), precision  # three carried round-trip steps
        a.hermite_step(DT, 2, resume=True)
        b.upload(st)
        b.hermite_step(DT, 5)
        five = b.download()
        assert H.same(a.download(), five), precision  # 3 + 2 resumed is 5
        assert H.same(H.round_trip(c, end3, DT, 2, carry=kept)[0], five), precision
        # without resume the second call evaluates afresh at the corrected state: a different quantity, a different end
        c.upload(st)
        c.hermite_step(DT, 3)
        c.hermite_step(DT, 2)
        assert not H.same(c.download(), five), precision
        # resume is refused where the promise is seen to be broken: after an upload, a step, a kick
        c.upload(three | {"mass": st["mass"]})
        _refused(nbx, lambda: c.hermite_step(DT, 1, resume=True), "resume after an upload")
        c.hermite_step(DT, 1)
        c.step(1, kenergy=False)
        _refused(nbx, lambda: c.hermite_step(DT, 1, resume=True), "resume after a step")
        c.hermite_step(DT, 1)
        c.kick(0.01)
        _refused(nbx, lambda: c.hermite_step(DT, 1, resume=True), "resume after a step or a kick")
        c.hermite_step(DT, 1)
        c.hermite_step(DT, 1, resume=True)  # and honoured again after a call that started afresh


@pytest.mark.parametrize("precision", [32, 64])
def test_resume_is_refused_on_a_fresh_object_of_every_kind_and_after_an_upload_a_step_or_a_kick(nbx, precision):
    s5, s3 = R.make_state(precision, 5, "cloud"), R.make_state(precision, 3, "cloud")
    with nbx.Context(5, precision) as c, nbx.Ensemble(5, 2, precision) as e, nbx.Ragged([5, 3], precision) as r:
        for o, up in ((c, lambda: c.upload(s5)), (e, lambda: e.upload([s5, s5])), (r, lambda: r.upload([s5, s3]))):
            up()
            _refused(nbx, lambda: o.hermite_step(DT, 1, resume=True), "resume without a previous Hermite call")
            o.hermite_step(DT, 0)  # nothing launched, nothing kept
            _refused(nbx, lambda: o.hermite_step(DT, 1, resume=True), "resume without a previous Hermite call")
            o.hermite_step(DT, 1)
            o.hermite_step(DT, 1, resume=True)
            up()
            _refused(nbx, lambda: o.hermite_step(DT, 1, resume=True), "resume after an upload")
            o.hermite_step(DT, 1)
            o.step(1, kenergy=False)
            _refused(nbx, lambda: o.hermite_step(DT, 1, resume=True), "resume after a step")
            o.hermite_step(DT, 1)
            o.kick(0.01)
            _refused(nbx, lambda: o.hermite_step(DT, 1, resume=True), "resume after a step or a kick")


def test_an_fp64_ensemble_is_of_fourth_order_and_follows_the_numpy_restatement(nbx):
    """An fp64 ensemble of jerk_ref's two systems, T = 0.25 in 16 and in 32 steps against 256 steps (dt / 16), all resident: the
    error ratio of a fourth-order scheme is 16 and of a second-order one 4; 8, their geometric mean, separates them.  The end state
    is jerk_ref.hermite's at the same dt to within that restatement's own distance from its dt / 16 run."""
    states = [R.hermite_state(seed) for seed in R.HERMITE_SEEDS]
    n, n1 = len(states[0]["mass"]), R.HERMITE_STEPS
    ends = {}
    with nbx.Ensemble(n, 2, 64) as e:
        for steps in (n1, 2 * n1, 16 * n1):
            e.upload(states)
            e.hermite_step(R.HERMITE_T / steps, steps)
            down = e.download()
            ends[steps] = [{f: down[f][m] for f in R.POS + R.VEL} for m in range(2)]
    for m, seed in enumerate(R.HERMITE_SEEDS):
        e1, e2 = (R.state_error(ends[s][m], ends[16 * n1][m]) for s in (n1, 2 * n1))
        ref1 = R.hermite(states[m], R.HERMITE_T / n1, n1)
        own = R.state_error(ref1, R.hermite(states[m], R.HERMITE_T / (16 * n1), 16 * n1))
        away = R.state_error(ends[n1][m], ref1)
        print("seed %d: resident errors %.3g %.3g ratio %.1f; from the numpy restatement %.3g, whose own error is %.3g" % (seed, e1, e2, e1 / e2, away, own))
        assert e1 / e2 >= 8.0, (seed, e1, e2)
        assert away <= own, (seed, away, own)


TIMED = {"Context": ("force_launches_timed", "force_ms_total"), "Ensemble": ("launches_timed", "step_ms_total"),
         "Ragged": ("launches_timed", "step_ms_total")}


@pytest.mark.parametrize("precision", [32, 64])
def test_steps_done_the_timed_fields_the_tracers_and_the_energy_partials_are_as_the_header_says(nbx, precision):
    n = 257
    s, s5 = R.make_state(precision, n, "cloud"), R.make_state(precision, 5, "cloud")
    T = R.DTYPE[precision]
    with nbx.Context(n, precision) as c, nbx.Ensemble(n, 2, precision) as e, nbx.Ragged([n, 5], precision) as r:
        for o, states, shape in ((c, s, (7,)), (e, [s, s], (2, 7)), (r, [s, s5], (2, 7))):
            o.upload(states)
            rng = np.random.default_rng(5)
            pts, vel = [rng.uniform(-1, 1, shape).astype(T) for _ in range(3)], [rng.uniform(-1, 1, shape).astype(T) for _ in range(3)]
            o.tracers_upload(pts, vel)
            o.profile(True)
            ke = o.step(2)
            assert np.all(np.asarray(o.step(0)) == np.asarray(ke)) and np.all(np.asarray(ke) > 0)  # the partials of the last step
            before, tracers = o.stats(), o.tracers_download()
            assert before["steps_done"] == 2 and before[TIMED[type(o).__name__][0]] > 0
            o.hermite_step(DT, 3)
            o.hermite_step(DT, 1, resume=True)
            after = o.stats()
            for k in ("steps_done",) + TIMED[type(o).__name__]:
                assert after[k] == before[k], (type(o).__name__, k)  # not counted, no launch timed
            assert H.same(o.tracers_download(), tracers)  # tracers do not move
            assert np.all(np.asarray(o.step(0)) == 0.0)  # as after an upload: the partials belong to no state
            o.profile(False)
            d = o.diagnostics()
            assert (d if isinstance(d, dict) else d[0])["steps_done"] == 2


def _with_mass(down, states):
    if isinstance(down, list):
        return [dict(d, mass=s["mass"]) for d, s in zip(down, states)]
    return dict(down, mass=states["mass"] if isinstance(states, dict) else np.stack([s["mass"] for s in states]))


@pytest.mark.parametrize("precision", [32, 64])
def test_a_following_step_is_the_step_after_an_upload_of_the_downloaded_state_graph_replay_on_and_off(nbx, precision):
    n = 513
    st = R.make_state(precision, n, "cloud")
    for graph in (1, 2):
        for nsteps in (3, 4):  # a context replays windows of four steps and more
            with nbx.Context(n, precision, use_graph=graph) as a, nbx.Context(n, precision, use_graph=graph) as b:
                a.upload(st)
                a.step(nsteps, 0.001)  # the graph, where there is one, is cached before the Hermite call
                a.upload(st)
                a.hermite_step(DT, 2)
                down = a.download()
                b.upload(_with_mass(down, st))
                assert a.diagnostics() == dict(b.diagnostics(), steps_done=nsteps)  # diagnostics() sees the new state
                replays = a.stats()["graph_replays"]
                assert a.step(nsteps, 0.001) == b.step(nsteps, 0.001), (precision, graph, nsteps)
                assert H.same(a.download(), b.download()), (precision, graph, nsteps)
                assert a.stats()["graph_replays"] - replays == (1 if graph == 1 and nsteps >= 4 else 0)
    s5 = R.make_state(precision, 5, "cloud")
    for make, states in ((lambda: nbx.Ensemble(n, 2, precision), [st, st]), (lambda: nbx.Ragged([n, 5], precision), [st, s5])):
        with make() as a, make() as b:
            a.upload(states)
            a.hermite_step(DT, 2)
            b.upload(_with_mass(a.download(), states))
            assert np.array_equal(a.step(3, 0.001), b.step(3, 0.001))
            da, db = a.download(), b.download()
            assert all(H.same(x, y) for x, y in zip(da, db)) if isinstance(da, list) else H.same(da, db)


@pytest.mark.parametrize("precision", [32, 64])
def test_analysis_calls_between_resumed_calls_change_nothing(nbx, precision):
    n = 513
    st = R.make_state(precision, n, "cloud")
    with nbx.Context(n, precision) as a:
        a.upload(st)
        a.hermite_step(DT, 3)
        mid = a.download()
        j = a.jerk()
        a.field(st["pos_x"][:9], st["pos_y"][:9], st["pos_z"][:9])
        a.diagnostics()
        a.neighbours()
        assert H.same(a.jerk(), j, R.KEYS) and H.same(a.download(), mid)
        a.hermite_step(DT, 2, resume=True)
        assert H.same(a.download(), lone_context(nbx, precision, n, "cloud", steps=5)), precision
    with nbx.Ragged([n, 5], precision) as r:
        r.upload([st, R.make_state(precision, 5, "cloud")])
        r.hermite_step(DT, 3)
        r.jerk()
        r.field(*[np.tile(st[f][:9], (2, 1)) for f in H.POS])
        r.diagnostics()
        r.hermite_step(DT, 2, resume=True)
        assert H.same(r.download()[0], lone_context(nbx, precision, n, "cloud", steps=5)), precision


def test_errors_come_in_the_headers_order_with_their_texts(nbx):
    def fails(call, code, text):
        with pytest.raises(nbx.NbxError) as err:
            call()
        assert err.value.code == code and str(err.value).endswith(text), str(err.value)

    s5, s3 = R.make_state(32, 5, "cloud"), R.make_state(32, 3, "cloud")
    with nbx.Context(5, 32) as c, nbx.Ensemble(5, 3, 32) as e, nbx.Ragged([5, 3], 32) as r:
        for o, name in ((c, "nbx_hermite_step"), (e, "nbx_ensemble_hermite_step"), (r, "nbx_ragged_hermite_step")):
            # 2, 3: the arguments, before the state -- nothing is uploaded yet
            for dt in (float("nan"), float("inf"), 1e300):  # 1e300 is no finite fp32 value
                fails(lambda: o.hermite_step(dt, -1, resume=True), nbx.NBX_ERR_ARG, name + ": dt is not finite")
            fails(lambda: o.hermite_step(DT, -1, resume=True), nbx.NBX_ERR_ARG, name + ": nsteps < 0")
        # 5: not uploaded, before resume and before nsteps == 0
        fails(lambda: c.hermite_step(DT, 0, resume=True), nbx.NBX_ERR_STATE, "nbx_hermite_step: nbx_upload has not been called")
        e.upload([s5], first=0)
        e.upload([s5], first=2)
        fails(lambda: e.hermite_step(DT, 0, resume=True), nbx.NBX_ERR_STATE, "nbx_ensemble_hermite_step: member 1 has not been uploaded")
        r.upload([s5], first=0)
        fails(lambda: r.hermite_step(DT, 0, resume=True), nbx.NBX_ERR_STATE, "nbx_ragged_hermite_step: member 1 has not been uploaded")
        # 6: a local step awaits commit, before resume
        c.upload(s5)
        c.step_local()
        fails(lambda: c.hermite_step(DT, 1, resume=True), nbx.NBX_ERR_STATE, "nbx_hermite_step: a local step awaits nbx_commit")
        c.commit()
        # 8: resume, before nsteps == 0; 9: nsteps == 0 is NBX_OK and changes nothing
        e.upload([s5], first=1)
        r.upload([s3], first=1)
        for o, name in ((c, "nbx_hermite_step"), (e, "nbx_ensemble_hermite_step"), (r, "nbx_ragged_hermite_step")):
            fails(lambda: o.hermite_step(DT, 0, resume=True), nbx.NBX_ERR_STATE, name + ": resume without a previous Hermite call on this object")
            before = o.download()
            o.hermite_step(DT, 0)
            after = o.download()
            assert all(H.same(x, y) for x, y in zip(before, after)) if isinstance(before, list) else H.same(before, after)
    # 7: a sliced context, after the commit check
    with nbx.Context(2049, 32, i_begin=0, i_count=512, n_alloc=2304) as c:
        c.upload(R.make_state(32, 2049, "cloud"))
        c.step_local()
        fails(lambda: c.hermite_step(DT, 1), nbx.NBX_ERR_STATE, "nbx_hermite_step: a local step awaits nbx_commit")
        c.commit()
        fails(lambda: c.hermite_step(DT, 1), nbx.NBX_ERR_STATE,
              "nbx_hermite_step: the context owns a slice of the bodies (the velocities of the others are not resident)")
    # 4: more than 2^22 bodies, before the state
    with nbx.Context((1 << 22) + 1, 32) as c:
        fails(lambda: c.hermite_step(DT, 1), nbx.NBX_ERR_ARG, "nbx_hermite_step: n exceeds 4194304")
    # an fp64 object takes the dt an fp32 object cannot hold (nothing to launch: the check alone)
    with nbx.Context(5, 64) as c:
        c.upload(R.make_state(64, 5, "cloud"))
        c.hermite_step(1e300, 0)


def test_a_resident_step_costs_no_more_than_the_round_trip_it_replaces(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32: per step, hermite_step(dt, 8,
    resume) against the carried round trip of public calls it replaces (jerk, host update, upload), in this process, arms
    alternated (tools/hermite_cost.py).  ratio <= 1.0, the condition every call of this kind carries; both arms return the same
    bits."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hermite_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = hermite_cost.measure(nbx, kind)
        print("%s fp32: resident %.1f us, round trip %.1f us per step, ratio %.4f; plain step %.1f us" % (
            kind, r["resident_us_per_step"], r["round_trip_us_per_step"], r["ratio"], r["plain_step_us_per_step"]))
        cells[kind] = r
    hermite_cost.write(hermite_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_bits_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
