"""Resident tracers on the device (include/nbx_tracers.h) against the round trip they replace (tests/tracers_ref.py: round_trip --
nbx_field at the host's tracer positions, the update in numpy in the object's dtype, nbx_step(dt, 1)), bit for bit, as a context,
as members of an ensemble and as members of one ragged ensemble, in fp32 and fp64.

Shapes, with what field_shape(m, n) makes of them (checked below against field_ref.field_shape, the header's rule restated):
    (n, m) = (63, 1)        1 tile,   1 column,                        1 split
             (300, 700)     2 tiles,  2 columns (m > n),               1 split
             (2049, 1025)   9 tiles,  3 columns, the last of 1 tracer, 2 splits of 5 + 4 tiles
             (4099, 513)    17 tiles, 2 columns,                       4 splits of 5 + 5 + 5 + 2 tiles
The time step of the bit tests is 0.01, no power of two: a dt rounds, so a contracted a dt + w would show.

The only tolerance is the field's own (test 4): one step from rest at dt = 2^-6 leaves w = a dt exactly, and that a is held per
tracer to field_ref's gate K <= 2 max(K_ref, 16) against field_ref.truth.  Everything else is equality of bits."""
import ctypes
import os
import sys

import numpy as np
import pytest

import field_ref as R
import kick_ref as K
import tracers_ref as TR
from conftest import ROOT

pytestmark = pytest.mark.gpu

SHAPES = ((63, 1), (300, 700), (2049, 1025), (4099, 513))
DT = 0.01
POS, VEL = TR.POS, TR.VEL


def _split(tr):
    return [tr[k] for k in POS], [tr[k] for k in VEL]


def _stack(trs):
    return {k: np.ascontiguousarray(np.stack([t[k] for t in trs])) for k in TR.KEYS}


def _row(tr, j):
    return {k: tr[k][j] for k in TR.KEYS}


def _case(precision, n, m, seed=0):
    state = K.make_state(9000 + 7 * seed + n, n, R.DTYPE[precision])
    return state, TR.make_tracers(precision, state, m, seed=seed)


def test_the_shapes_are_what_the_table_says():
    assert [R.field_shape(m, n) for n, m in SHAPES] == [(1, 1, 1, 1), (2, 2, 1, 2), (3, 9, 2, 5), (2, 17, 4, 5)]
    assert 1025 % 512 == 1 and 17 == 5 + 5 + 5 + 2 and 9 == 5 + 4
    assert [R.field_shape(513, n)[2] for n in (5, 2049, 700, 4099)] == [1, 2, 1, 4]  # the ragged members of test 3


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against the round trip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("precision", [32, 64])
def test_five_steps_are_the_round_trips_bits_also_as_three_and_two(nbx, precision, n, m):
    state, tr = _case(precision, n, m)
    with nbx.Context(n, precision) as c, nbx.Context(n, precision) as twin:
        twin.upload(state)
        want, ke_want = TR.round_trip(twin, tr, precision, DT, 5)
        bodies = twin.download()
        for parts in ((5,), (3, 2)):  # (3, 2): the second call starts on the other position buffer
            c.upload(state)
            c.tracers_upload(*_split(tr))
            assert c.tracers_count() == m
            for k in parts[:-1]:
                c.tracers_step(k, DT, kenergy=False)
            ke = c.tracers_step(parts[-1], DT)
            got = c.tracers_download()
            assert all(got[k].dtype == R.DTYPE[precision] and got[k].shape == (m,) for k in TR.KEYS)
            assert TR.same(got, want), parts
            assert TR.same(c.download(), bodies) and ke == ke_want, parts
        assert not TR.same(want, tr)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the bodies against a twin that replays a graph, and under other launch plans
# ---------------------------------------------------------------------------------------------------------------------------
PLANS = (("default", 32, {}), ("default", 64, {}), ("sgprw-2-splits", 32, dict(kernel_variant="KERNEL_SGPRW", j_split=2)),
         ("lds-2-splits", 32, dict(kernel_variant="KERNEL_LDS", j_split=2)), ("fp64-sgprw-2-splits", 64, dict(kernel_variant="KERNEL_SGPRW", j_split=2)))


@pytest.mark.parametrize("name,precision,opts", PLANS, ids=[p[0] + "-fp%d" % p[1] for p in PLANS])
def test_the_bodies_are_those_of_plain_steps_that_replay_a_graph(nbx, name, precision, opts):
    n, m = 2048, 513
    opts = {k: getattr(nbx, v) if isinstance(v, str) else v for k, v in opts.items()}
    state, tr = _case(precision, n, m)
    with nbx.Context(n, precision, **opts) as c, nbx.Context(n, precision, **opts) as twin:
        for o in (c, twin):
            o.upload(state)
        c.tracers_upload(*_split(tr))
        ke = c.tracers_step(8, DT)
        ke_twin = twin.step(8, DT)
        assert TR.same(c.download(), twin.download()) and ke == ke_twin
        st, st_twin = c.stats(), twin.stats()
        assert st["steps_done"] == st_twin["steps_done"] == 8
        if name == "default":
            assert st_twin["graph_replays"] > 0 and st["graph_replays"] == 0  # the comparison means what it says
        assert c.step(0, DT) == twin.step(0, DT) == ke  # the partials the last step left
        assert not TR.same(c.tracers_download(), tr)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. members
# ---------------------------------------------------------------------------------------------------------------------------
def _context_after(nbx, precision, state, tr, nsteps, h, NB, loop):
    """(tracers, bodies, kinetic energy) of a context holding one member's state and tracers after nsteps steps and a kick of h:
    the context whose bodies step as a member's do (include/nbx_ensemble.h: the one-launch kernel of the batch object's plan)."""
    with nbx.Context(len(state["mass"]), precision, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
        c.upload(state)
        c.tracers_upload(*_split(tr))
        ke = c.tracers_step(nsteps, DT)
        c.tracers_kick(h)
        return c.tracers_download(), c.download(), ke


@pytest.mark.parametrize("kind", ["ensemble", "ragged"])
@pytest.mark.parametrize("precision", [32, 64])
def test_every_member_is_a_context_holding_its_state_and_tracers(nbx, precision, kind):
    m, h = 513, -0.003
    sizes = (2049, 2049, 2049) if kind == "ensemble" else (5, 2049, 700, 4099)
    S = len(sizes)
    cases = [_case(precision, n, m, seed=1 + k) for k, n in enumerate(sizes)]
    states, trs = [c[0] for c in cases], [c[1] for c in cases]
    with (nbx.Ensemble(sizes[0], S, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)) as o:
        st = o.stats()
        want = [_context_after(nbx, precision, s, t, 3, h, st["bodies_per_lane"], st["inner_loop"]) for s, t in cases]
        o.upload(states)
        assert o.tracers_count() == 0
        o.tracers_upload(*_split(_stack(trs[1:])), first=1)  # the first upload fixes m; member 0 has none yet
        assert o.tracers_count() == m
        for call in (lambda: o.tracers_step(1, DT), lambda: o.tracers_kick(h), lambda: o.tracers_download()):
            with pytest.raises(nbx.NbxError) as err:
                call()
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has no tracers" in str(err.value)
        part = o.tracers_download(first=1, count=S - 1)  # the uploaded members can be read back
        assert all(TR.same(_row(part, j), trs[1 + j]) for j in range(S - 1))
        with pytest.raises(nbx.NbxError) as err:  # another m on a part of the members
            o.tracers_upload(*_split(_stack([TR.make_tracers(precision, states[0], 7)])), first=0)
        assert err.value.code == nbx.NBX_ERR_ARG and "m differs" in str(err.value)
        o.tracers_upload(*_split(_stack(trs[:1])), first=0)
        ke = o.tracers_step(3, DT)
        o.tracers_kick(h)
        got, bodies = o.tracers_download(), o.download()
        assert all(got[k].shape == (S, m) for k in TR.KEYS)
        for j in range(S):
            assert TR.same(_row(got, j), want[j][0]), j
            assert TR.same(bodies[j] if kind == "ragged" else _row(bodies, j), want[j][1]) and ke[j] == want[j][2], j
        for first, count in ((S - 1, 1), (1, 2), (0, 0)):
            part = o.tracers_download(first=first, count=count)
            assert all(part[k].shape == (count, m) and np.array_equal(part[k], got[k][first:first + count]) for k in TR.KEYS)
        assert not TR.same(_row(got, 0), _row(got, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. one step against the truth
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["box", "own"])  # off the bodies, and on them
@pytest.mark.parametrize("n,m", [(2049, 1025), (4099, 513)])
@pytest.mark.parametrize("precision", [32, 64])
def test_one_step_from_rest_applies_an_acceleration_inside_the_fields_gate(nbx, oracle, precision, n, m, family):
    c = R.case(oracle, precision, n, m, family)
    T = R.DTYPE[precision]
    dt = 2.0 ** -6  # w' = fl(a dt) = a dt exactly, p' = p + fl(w' dt)
    rest = [np.zeros(m, dtype=T) for _ in range(3)]
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        ctx.tracers_upload(c["points"], rest)
        ctx.tracers_step(1, dt, kenergy=False)
        got = ctx.tracers_download()
    acc = [(got[k] / T(dt)).astype(T) for k in VEL]
    assert all(np.array_equal((a * T(dt)).astype(T), got[k]) for a, k in zip(acc, VEL))  # the division was exact
    k_max = float(R.k_acc(acc, c["truth"], precision).max())
    print("fp%d (n, m) = (%d, %d) %s: K %.2f of %.1f (K_ref %.2f)" % (precision, n, m, family, k_max, c["gate_acc"], c["kref_acc"]))
    assert k_max <= c["gate_acc"], (precision, n, m, family, k_max, c["gate_acc"])
    for p, w, q in zip(POS, VEL, c["points"]):
        assert np.array_equal(got[p], (q + (got[w] * T(dt)).astype(T)).astype(T))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the kick
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(2049, 1025), (300, 700)])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_kick_is_velocity_only_with_the_fields_acceleration_and_leapfrog_is_the_hand_made_sequence(nbx, precision, n, m):
    state, tr = _case(precision, n, m, seed=5)
    h = 0.37 * DT
    L = nbx.load()
    with nbx.Context(n, precision) as c, nbx.Context(n, precision) as twin:
        for o in (c, twin):
            o.upload(state)
            o.tracers_upload(*_split(tr))
        want = TR.round_trip_kick(c, tr, precision, h)  # nbx_field's a at the tracers, the update in numpy
        c.tracers_kick(h)
        got = c.tracers_download()
        assert TR.same(got, want)
        assert all(got[k].tobytes() == tr[k].tobytes() for k in POS) and not any(np.array_equal(got[k], tr[k]) for k in VEL)
        assert TR.same(c.download(), twin.download()) and c.stats()["steps_done"] == 0  # the bodies are untouched
        # leapfrog of the joint system, from the same start, against the C calls made by hand
        c.tracers_upload(*_split(tr))
        ke = c.tracers_leapfrog(4, DT)
        out = ctypes.c_double(0.0)
        assert L.nbx_kick(twin._h, -0.5 * DT, None) == 0 and L.nbx_tracers_kick(twin._h, -0.5 * DT) == 0
        assert L.nbx_tracers_step(twin._h, DT, 4, None) == 0
        assert L.nbx_tracers_kick(twin._h, 0.5 * DT) == 0 and L.nbx_kick(twin._h, 0.5 * DT, ctypes.byref(out)) == 0
        assert TR.same(c.tracers_download(), twin.tracers_download()) and TR.same(c.download(), twin.download()) and ke == out.value
        plain = nbx.Context(n, precision)
        with plain:  # and the bodies' half of it is plain leapfrog
            plain.upload(state)
            assert plain.leapfrog(4, DT) == ke and TR.same(plain.download(), c.download())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. independence
# ---------------------------------------------------------------------------------------------------------------------------
def test_plain_calls_leave_the_tracers_alone_and_the_tracer_calls_leave_the_rest_alone(nbx):
    n, m, precision = 2049, 700, 32
    state, tr = _case(precision, n, m, seed=6)
    other = K.make_state(77, n, np.float32)
    pts = R.make_points(precision, state, 1500, "box", seed=9)
    with nbx.Context(n, precision) as c, nbx.Context(n, precision) as twin:
        for o in (c, twin):
            o.upload(state)
            o.profile(True)
        c.tracers_upload(*_split(tr))
        f0 = c.field(*pts)
        c.step(3, DT)
        c.kick(0.5 * DT)
        c.field(*pts)
        c.diagnostics()
        c.timescale()
        c.upload(other)
        assert TR.same(c.tracers_download(), tr) and c.tracers_count() == m  # plain calls do not touch them
        c.upload(state)
        assert all(c.field(*pts)[k].tobytes() == f0[k].tobytes() for k in R.KEYS)
        # the tracer calls own nothing else: the field's results, the partials, the profile, the counters
        ke = c.tracers_step(3, DT)
        c.tracers_kick(0.5 * DT)
        twin.step(3, DT)  # the plain calls of above that count: three steps, the new state
        twin.upload(state)
        ke_twin = twin.step(3, DT)
        f3, f3_twin = c.field(*pts), twin.field(*pts)
        assert all(f3[k].tobytes() == f3_twin[k].tobytes() for k in R.KEYS) and not all(f3[k].tobytes() == f0[k].tobytes() for k in R.KEYS)
        assert ke == ke_twin and c.step(0, DT) == twin.step(0, DT) == ke
        timing = ("force_ms_total",)
        sa, sb = c.stats(), twin.stats()
        assert sa["force_launches_timed"] == sb["force_launches_timed"] > 0  # the tracer launches are not in the force profile
        assert {k: v for k, v in sa.items() if k not in timing} == {k: v for k, v in sb.items() if k not in timing}


@pytest.mark.parametrize("precision", [32, 64])
def test_a_larger_set_then_a_smaller_one_then_none(nbx, precision):
    n = 2049
    state, _ = _case(precision, n, 1, seed=7)

    def fresh(tr):
        with nbx.Context(n, precision) as c:
            c.upload(state)
            c.tracers_upload(*_split(tr))
            c.tracers_step(2, DT, kenergy=False)
            return c.tracers_download()

    sets = [TR.make_tracers(precision, state, m, seed=m) for m in (513, 1500, 3)]  # the buffers grow, then serve a smaller set
    with nbx.Context(n, precision) as c, nbx.Context(n, precision) as twin:
        twin.upload(state)
        for tr in sets:
            c.upload(state)
            c.tracers_upload(*_split(tr))
            assert c.tracers_count() == len(tr["pos_x"])
            c.tracers_step(2, DT, kenergy=False)
            assert TR.same(c.tracers_download(), fresh(tr)), len(tr["pos_x"])
        T = R.DTYPE[precision]
        none = [np.zeros(0, dtype=T)] * 3
        c.upload(state)
        c.tracers_upload(none, none)
        assert c.tracers_count() == 0
        for call in (lambda: c.tracers_step(1, DT), lambda: c.tracers_kick(DT), lambda: c.tracers_download()):
            with pytest.raises(nbx.NbxError) as err:
                call()
            assert err.value.code == nbx.NBX_ERR_STATE and "no tracers have been uploaded" in str(err.value)
        assert c.step(2, DT) == twin.step(2, DT) and TR.same(c.download(), twin.download())  # plain steps still work


def test_state_errors_on_real_objects(nbx):
    state, tr = _case(32, 300, 7, seed=8)
    with nbx.Context(300, 32) as c:
        c.tracers_upload(*_split(tr))  # tracers may arrive before the bodies
        for call, where in ((lambda: c.tracers_step(1, DT), "nbx_tracers_step"), (lambda: c.tracers_kick(DT), "nbx_tracers_kick")):
            with pytest.raises(nbx.NbxError) as err:
                call()
            assert err.value.code == nbx.NBX_ERR_STATE and where + ": nbx_upload has not been called" in str(err.value)
        c.upload(state)
        c.step_local(DT)
        with pytest.raises(nbx.NbxError) as err:
            c.tracers_step(1, DT)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_tracers_step: a local step awaits nbx_commit" in str(err.value)
        c.commit()
        c.tracers_step(1, DT)
    with nbx.Context(300, 32, i_begin=0, i_count=256) as c:  # a slice: refused as by nbx_step
        c.upload(state)
        c.tracers_upload(*_split(tr))
        for call, where in ((lambda: c.tracers_step(1, DT), "nbx_tracers_step"), (lambda: c.tracers_kick(DT), "nbx_tracers_kick")):
            with pytest.raises(nbx.NbxError) as err:
                call()
            assert err.value.code == nbx.NBX_ERR_STATE and where + ": context owns a slice" in str(err.value)
    states = [K.make_state(60 + k, 300, np.float32) for k in range(3)]
    with nbx.Ensemble(300, 3, 32) as e:
        e.upload(states[:2])
        e.tracers_upload(*_split(_stack([tr] * 3)))
        with pytest.raises(nbx.NbxError) as err:
            e.tracers_step(1, DT)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_ensemble_tracers_step: member 2 has not been uploaded" in str(err.value)
        L = nbx.load()
        big = (1 << 22) // 3 + 1
        p = tr["pos_x"].ctypes.data_as(ctypes.c_void_p)
        assert L.nbx_ensemble_tracers_upload(e._h, 0, 3, big, p, p, p, p, p, p) == nbx.NBX_ERR_ARG  # refused before the arrays are read
        assert L.nbx_last_error().decode() == "nbx_ensemble_tracers_upload: members * m exceeds 4194304"
        assert e.tracers_count() == 7


# ---------------------------------------------------------------------------------------------------------------------------
# 7. cost
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_step_costs_no_more_than_the_round_trip_it_replaces(nbx):
    """fp32, in this process, rounds alternated, medians (tools/tracers_cost.py; the warm-up and repetition counts are those of
    tests/test_field_gpu.py's cost test): per step, one tracers_step call of K steps against K round trips -- nbx_field, the update
    in numpy, nbx_step(dt, 1) -- on objects created and uploaded beforehand, for one context of n = m = 4096 and for 16 x 2048 with
    m = 2048.  The new path does the same pair work and omits two copies and a synchronisation per step, so no margin is claimed:
    ratio <= 1.0.  The baseline is code of the parent commit."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tracers_cost
    for kind in ("context", "ensemble"):
        r = tracers_cost.measure(nbx, kind, rounds=5, window=0.05)
        print("%s fp32 m = %d: tracers_step %.1f us, round trip %.1f us, plain step %.1f us per step; ratio %.3f"
              % (kind, r["m"], r["tracers_step_us"], r["round_trip_us"], r["plain_step_us"], r["ratio"]))
        assert (r["n_min"], r["n_max"], r["m"], r["members"]) == ((4096, 4096, 4096, 1) if kind == "context" else (2048, 2048, 2048, 16))
        assert r["same_bits_from_both_arms"], kind
        assert r["ratio"] <= 1.0, (kind, r["ratio"])
