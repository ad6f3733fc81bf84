"""Pair approach and free-fall rates on the device (include/nbx_timescale.h) against the fp64 numpy restatement
tests/timescale_ref.py, as a context, as members of an ensemble and as members of one ragged ensemble.

Error budget, to first order, u the unit round-off of the object's precision (2^-24 or 2^-53): r2 and w carry 5u each; fp32:
rsq within 1 ulp gives 4.5u on inv and 10u on inv2, hence 16u on approach and 17.5u on freefall; fp64: rsq() is documented in
nbx_pair.hpp at 3/2 e^2 with e <= 2^-25, i.e. 12u, hence about 42u on approach and 57u on freefall.  A max or min over pairs
moves by no more than its terms do.  Gates, each about twice its bound: fp32 rates within 32u relative, fp64 rates within 128u,
min_r2 within 8u in both.  The largest deviations seen go to profiles/timescale_error.json.

States: kick_ref.make_state, plain; the same spread out (timescale_ref.spread_state) with one planted pair that is closest,
fastest-approaching and heaviest by a factor of ten (test_timescale_cpu.py checks the factor with the restatement; here it is
checked again for every state used); and, for the padding mask, all bodies 50 away from the origin in every coordinate with
velocities of order 1, where a zero padding record would give a small but wrong approach rate ("offset") -- small enough to
hide behind the maximum, so there is also "bulk": the bodies about the origin, all moving at 50 in x, where the padding record,
at rest at the origin, would be the fastest-approaching partner by far (the restatement says so below)."""
import ctypes
import json
import math
import os
import sys
import zlib

import numpy as np
import pytest

import kick_ref as K
import timescale_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = {32: 2.0 ** -24, 64: 2.0 ** -53}
RATE_GATE = {32: 32.0, 64: 128.0}  # in u
R2_GATE = 8.0
ERROR_FILE = os.path.join(ROOT, "profiles", "timescale_error.json")
SHAPES = (1, 2, 255, 256, 257, 513, 2049, 4097)
RAGGED_SIZES = (1, 2, 255, 257, 513, 2049, 300)
DTYPE = {32: np.float32, 64: np.float64}


def state_names(n):
    """The states a size is tested with: plain, the padding-mask state at the tile edge, and the planted pairs that fit."""
    names = ["plain"]
    if n in (255, 257):
        names += ["offset", "bulk"]
    if n >= 2:
        names.append("pair:0:%d" % (n - 1))
    if n > 2:
        names.append("pair:%d:0" % (n - 1))
    if n >= 257:
        names.append("pair:255:256")
    if n >= 255:
        names.append("pair:100:101")  # two neighbours inside one tile
    if n == 2049:
        names.append("pair:1279:1280")  # either side of the boundary between its two j splits (5 and 4 tiles)
    return names


_states, _refs, _ctx = {}, {}, {}


def state(precision, n, name):
    key = (precision, n, name)
    if key not in _states:
        if name == "plain":
            s = K.make_state(1000 + n, n, DTYPE[precision])
        elif name == "offset":
            s = K.make_state(2000 + n, n, np.float64)
            for k in K.FIELDS[:3]:
                s[k] = s[k] + 50.0
            for k in K.FIELDS[3:6]:
                s[k] = s[k] / 0.3 + 0.5
            s = {k: np.ascontiguousarray(v.astype(DTYPE[precision])) for k, v in s.items()}
        elif name == "bulk":
            s = K.make_state(2500 + n, n, np.float64)
            s["vel_x"] = s["vel_x"] + 50.0
            s = {k: np.ascontiguousarray(v.astype(DTYPE[precision])) for k, v in s.items()}
        else:
            i, j = (int(x) for x in name.split(":")[1:])
            s = R.plant_pair(R.spread_state(3000 + n, n, DTYPE[precision]), i, j)
        _states[key] = s
    return _states[key]


def ref(precision, n, name):
    """The restatement's values, computed once per state; a planted pair is checked to be extreme by the factor of ten."""
    key = (precision, n, name)
    if key not in _refs:
        s = state(precision, n, name)
        if name.startswith("pair"):
            i, j = (int(x) for x in name.split(":")[1:])
            t, back = R.timescale_and_background(s, i, j)
            pair = R.pair_values(s, i, j)
            assert {k: t[k] for k in R.KEYS} == pair, key
            if n > 2:
                assert pair["approach_rate2"] >= 10 * back["approach_rate2"] and pair["freefall_rate2"] >= 10 * back["freefall_rate2"], key
                assert 10 * pair["min_r2"] <= back["min_r2"], key
        else:
            t = R.timescale(s)
        _refs[key] = t
    return _refs[key]


def context_values(nbx, precision, n, name):
    """What a default context of n bodies holding the state returns, asked once per state: the bits the members are held to."""
    key = (precision, n, name)
    if key not in _ctx:
        with nbx.Context(n, precision) as c:
            c.upload(state(precision, n, name))
            t = c.timescale()
            assert c.timescale() == t  # two calls in a row: the same bits
        _ctx[key] = t
    return _ctx[key]


_worst = {}


def _record(extra=None):
    out = {}
    if os.path.exists(ERROR_FILE):
        with open(ERROR_FILE) as f:
            out = json.load(f)
    out["what"] = ("largest relative deviation of nbx_timescale / nbx_ensemble_timescale / nbx_ragged_timescale from the fp64 restatement "
                   "tests/timescale_ref.py seen by tests/test_timescale_gpu.py, in units of u = 2^-24 (fp32) or 2^-53 (fp64); gates: rates "
                   "32 u (fp32) and 128 u (fp64), min_r2 8 u")
    for (precision, field), v in _worst.items():
        out.setdefault("fp%d" % precision, {})[field] = v
    if extra:
        out.update(extra)
    os.makedirs(os.path.dirname(ERROR_FILE), exist_ok=True)
    with open(ERROR_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def check(got, precision, n, name, steps_done=0):
    want = ref(precision, n, name)
    assert got["n"] == n and got["steps_done"] == steps_done
    if n == 1:  # no pair
        assert (got["approach_rate2"], got["freefall_rate2"], got["min_r2"]) == (0.0, 0.0, math.inf)
        return
    for field in R.KEYS:
        dev = abs(got[field] - want[field]) / want[field] / U[precision]
        print("fp%d n = %d %s %s: %.17g against %.17g, %.2f u" % (precision, n, name, field, got[field], want[field], dev))
        key = (precision, field)
        if dev > _worst.get(key, {"u": -1.0})["u"]:
            _worst[key] = {"u": dev, "n": n, "state": name}
        assert dev <= (R2_GATE if field == "min_r2" else RATE_GATE[precision]), (precision, n, name, field, got[field], want[field], dev)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_restatement(nbx, precision, n):
    for name in state_names(n):
        check(context_values(nbx, precision, n, name), precision, n, name)
    _record()


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_restatement_and_have_the_bits_of_a_context(nbx, precision, n):
    names = state_names(n)
    S = len(names)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload([state(precision, n, name) for name in names])
        full = e.timescale()
        assert e.timescale() == full
        assert len(full) == S
        for m, name in enumerate(names):
            check(full[m], precision, n, name)
            assert full[m] == context_values(nbx, precision, n, name), (precision, n, name)
        # a member's entry is the same whatever first and count it was asked with
        for first, count in ((0, 1), (S - 1, 1), (S // 2, S - S // 2), (S, 0), (0, 0)):
            assert e.timescale(first, count) == full[first:first + count], (first, count)
        assert e.timescale(first=S // 2) == full[S // 2:]
        assert e.timescale() == full
    _record()


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_restatement_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    """One ragged ensemble of RAGGED_SIZES, queried whole and as sub-ranges that start in the middle; three populations of states
    so that every size meets a planted pair in every place it has."""
    S = len(RAGGED_SIZES)
    for pick in (0, 1, 2, 3, 4, -1):  # -1: the last state of every size -- the split boundary at 2049, the neighbours elsewhere
        names = [state_names(n)[min(pick, len(state_names(n)) - 1)] for n in RAGGED_SIZES]
        with nbx.Ragged(RAGGED_SIZES, precision) as r:
            r.upload([state(precision, n, name) for n, name in zip(RAGGED_SIZES, names)])
            full = r.timescale()
            assert r.timescale() == full and len(full) == S
            for m, (n, name) in enumerate(zip(RAGGED_SIZES, names)):
                check(full[m], precision, n, name)
                assert full[m] == context_values(nbx, precision, n, name), (precision, n, name)
            for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (1, 3), (S, 0), (3, 0)):
                assert r.timescale(first, count) == full[first:first + count], (first, count)
            assert r.timescale(first=5) == full[5:]
            assert r.timescale() == full  # a partial call leaves nothing behind that a full one sees
    # the same systems in another order: other neighbours, other offsets, other rows -- the same bits
    names = [state_names(n)[-1] for n in RAGGED_SIZES]
    with nbx.Ragged(RAGGED_SIZES[::-1], precision) as r:
        r.upload([state(precision, n, name) for n, name in zip(RAGGED_SIZES, names)][::-1])
        assert r.timescale() == full[::-1]
    _record()


def test_every_planted_place_is_met():
    assert set(state_names(2049)) == {"plain", "pair:0:2048", "pair:2048:0", "pair:255:256", "pair:100:101", "pair:1279:1280"}
    assert set(state_names(4097)) == {"plain", "pair:0:4096", "pair:4096:0", "pair:255:256", "pair:100:101"}  # 4 splits, 9 columns
    assert set(state_names(257)) == {"plain", "offset", "bulk", "pair:0:256", "pair:256:0", "pair:255:256", "pair:100:101"}
    assert state_names(1) == ["plain"] and state_names(2) == ["plain", "pair:0:1"]
    assert max(len(state_names(n)) for n in RAGGED_SIZES) == 7  # the picks of the ragged test reach every state


@pytest.mark.parametrize("precision", [32, 64])
def test_the_padding_record_would_be_seen_without_the_mask(precision):
    """The restatement with a zero record appended -- what the position buffer holds behind n: in the bulk state it would be the
    fastest-approaching partner by a factor, so that state tells a masked kernel from an unmasked one; in the offset state its
    rate is there but below the maximum."""
    for n in (255, 257):
        s = state(precision, n, "bulk")
        padded = {k: np.concatenate([v, np.zeros(1, dtype=v.dtype)]) for k, v in s.items()}
        assert R.timescale(padded)["approach_rate2"] > 10 * ref(precision, n, "bulk")["approach_rate2"]
        s = state(precision, n, "offset")
        pad = R.pair_values({k: np.concatenate([v, np.zeros(1, dtype=v.dtype)]) for k, v in s.items()}, 0, n)
        assert 0 < pad["approach_rate2"] < ref(precision, n, "offset")["approach_rate2"]


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 2, 4, 8)] +
    [dict(kernel_variant="KERNEL_SGPRW", bodies_per_lane=b) for b in (1, 2, 3, 4)] +
    [dict(kernel_variant="KERNEL_JLANE", bodies_per_lane=b) for b in (2, 4, 5, 6, 7, 8, 16)] +
    [dict(j_split=s) for s in (1, 2, 4, 8, 32)] + [dict(kernel_variant="KERNEL_LDS", j_split=4), dict(kernel_variant="KERNEL_SGPRW", j_split=16)])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_bits_do_not_depend_on_the_contexts_options(nbx, precision):
    """n = 16384: kernel variant, summation order, bodies per lane 1 ... 8 and explicit j splits, where nbx_create takes them."""
    n = 16384
    s = K.make_state(77, n, DTYPE[precision])
    with nbx.Context(n, precision) as c:
        c.upload(s)
        want = c.timescale()
    assert want["n"] == n and want["approach_rate2"] > 0 and want["freefall_rate2"] > 0 and 0 < want["min_r2"] < 1
    made = []
    for o in CONTEXT_OPTIONS:
        opts = {k: getattr(nbx, v) if isinstance(v, str) else v for k, v in o.items()}
        try:
            c = nbx.Context(n, precision, **opts)
        except nbx.NbxError as e:
            assert e.code == nbx.NBX_ERR_ARG, (o, str(e))  # not a shape this precision has
            continue
        with c:
            c.upload(s)
            st = c.stats()
            assert c.timescale() == want, (o, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    print("fp%d: %d of %d option sets made a context; distinct shapes: %d" % (precision, len(made), len(CONTEXT_OPTIONS), len(set(made))))
    assert {m[0] for m in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR, nbx.KERNEL_SGPRW}
    assert {m[1] for m in made} == {nbx.ORDER_TREE, nbx.ORDER_REFERENCE}
    assert {m[2] for m in made} >= ({1, 2, 4, 8} if precision == 32 else {1, 2, 4}) and len(set(made)) >= 12


def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


def _flat(down):
    if isinstance(down, dict):
        return [down[f] for f in K.FIELDS[:6]]
    return [d[f] for d in down for f in K.FIELDS[:6]]


UNTOUCHED = ("steps_done", "force_launches_timed", "force_ms_total", "launches_timed", "step_ms_total", "graph_replays")


def _make(nbx, kind, precision=32):
    sizes = (300, 2049, 513)
    if kind == "context":
        return nbx.Context(2049, precision), state(precision, 2049, "plain")
    if kind == "ensemble":
        return nbx.Ensemble(2049, 3, precision), [state(precision, 2049, name) for name in ("plain", "pair:0:2048", "pair:1279:1280")]
    return nbx.Ragged(sizes, precision), [K.make_state(40 + k, n, DTYPE[precision]) for k, n in enumerate(sizes)]


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_the_call_is_on_the_stream_and_leaves_the_trajectory_and_every_counter_alone(nbx, kind):
    dt = 1.0 / 256
    o, states = _make(nbx, kind)
    with o:
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        t3 = o.timescale()
        t3b = o.timescale(1, 2) if kind != "context" else o.timescale()
        after = o.stats()
        assert {k: before[k] for k in UNTOUCHED if k in before} == {k: after[k] for k in UNTOUCHED if k in after}
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        ke_a = o.step(3, dt)
        a = _flat(o.download())
    for t in (t3 if kind != "context" else [t3]):
        assert t["steps_done"] == 3
    assert t3b == (t3[1:3] if kind != "context" else t3)
    o, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.step(3, dt)  # synchronises
        o.sync()
        assert o.timescale() == t3
    o, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        t0 = o.timescale()
        ke_b = o.step(6, dt)
        b = _flat(o.download())
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)
    assert t0 != t3


def test_state_errors(nbx):
    L = nbx.load()
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.timescale()
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_timescale: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        assert c.timescale()["n"] == 300
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.timescale()
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_commit" in str(err.value)
    n, blk = 1000, 512
    with nbx.Context(n, 32, i_begin=0, i_count=blk, n_alloc=2 * blk) as c:  # a sliced context: the others' velocities are not resident
        c.upload(states[2])
        with pytest.raises(nbx.NbxError) as err:
            c.timescale()
        assert err.value.code == nbx.NBX_ERR_STATE and "slice" in str(err.value) and "nbx_timescale" in str(err.value)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.timescale()
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_commit" in str(err.value)  # the commit comes first
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_timescale"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_timescale")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.timescale()
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.timescale(first, count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value), (first, count)
            part = o.timescale(0, 3)  # the uploaded members can be asked before the others arrive
            assert [t["n"] for t in part] == [len(s["mass"]) for s in st[:3]]
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.timescale(first, count)
                assert err.value.code == nbx.NBX_ERR_ARG, (first, count, str(err.value))
            o.upload(st[3:], first=3)
            assert o.timescale(0, 3) == part
            f = getattr(L, name)
            t = (nbx.Timescale * 3)()
            t[0].min_r2 = -7.0
            assert f(o._h, 1, 0, t) == nbx.NBX_OK and t[0].min_r2 == -7.0 and t[0].struct_size == 0  # count == 0: nothing written
            t[1].struct_size = ctypes.sizeof(nbx.Timescale) - 8
            assert f(o._h, 0, 3, t) == nbx.NBX_ERR_ARG
            assert b"out[1].struct_size" in L.nbx_last_error() and t[0].min_r2 == -7.0 and t[2].n == 0
            t[1].struct_size = 0  # "this version"; set on return
            assert f(o._h, 0, 3, t) == nbx.NBX_OK
            assert [t[k].struct_size for k in range(3)] == [ctypes.sizeof(nbx.Timescale)] * 3 and [t[k].asdict() for k in range(3)] == part


def test_adaptive_steps_beat_equal_steps_on_the_planted_encounters(nbx):
    """The three systems of test_timescale_cpu.py as one fp64 ensemble: adaptive() reaches T in no more steps than the run with
    equal steps it is compared with, and ends with a smaller energy error by Ensemble.diagnostics() -- the inequality the
    restatement shows with more than 4x room (610 steps, 4.1e-4 against 2.1e-3 ... 2.2e-3)."""
    s0 = [R.encounter_state(seed) for seed in R.ENCOUNTER_SEEDS]
    with nbx.Ensemble(K.N, 3, 64) as e:
        e.upload(s0)
        e0 = [d["etotal"] for d in e.diagnostics()]
        t, steps, dts = e.adaptive(R.ENCOUNTER_T, R.ENCOUNTER_ETA, R.ENCOUNTER_DT_MAX)
        d = e.diagnostics()
        ea = [abs(x["etotal"] - a) / abs(a) for x, a in zip(d, e0)]
    assert t == R.ENCOUNTER_T and steps == len(dts) and all(x["steps_done"] == steps for x in d)
    fixed_steps = steps
    with nbx.Ensemble(K.N, 3, 64) as e:
        e.upload(s0)
        e.step(fixed_steps, R.ENCOUNTER_T / fixed_steps, kenergy=False)
        ef = [abs(x["etotal"] - a) / abs(a) for x, a in zip(e.diagnostics(), e0)]
    print("adaptive: %d steps of %.3e ... %.3e, errors %s; fixed: %d steps of %.3e, errors %s"
          % (steps, min(dts), max(dts), ["%.3e" % x for x in ea], fixed_steps, R.ENCOUNTER_T / fixed_steps, ["%.3e" % x for x in ef]))
    _record({"adaptive_on_the_device": {"steps": steps, "dt_min": min(dts), "dt_max": max(dts), "adaptive_energy_error": ea,
                                        "fixed_steps": fixed_steps, "fixed_energy_error": ef}})
    assert steps <= fixed_steps
    assert all(a < f for a, f in zip(ea, ef)), (ea, ef)


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32: one batch call against 16
    nbx_timescale calls on contexts created and uploaded beforehand, in this process, rounds alternated
    (tools/timescale_cost.py).  The pair work of the two arms is the same and one call issues 2 launches and 1 synchronisation
    where the contexts issue 32 and 16, so the gate has no further margin: ratio <= 1.0, the condition the sibling features use.
    The time against one diagnostics call on the same object is recorded, not gated."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import timescale_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = timescale_cost.measure(nbx, kind)
        print("%s fp32: batch %.1f us, 16 contexts %.1f us, ratio %.3f; diagnostics %.1f us, timescale / diagnostics %.2f"
              % (kind, r["batch_us"], r["contexts_us"], r["ratio"], r["diagnostics_us"], r["against_diagnostics"]))
        cells[kind] = r
    timescale_cost.write(timescale_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
