"""Nearest neighbour and radius count of every body on the device (include/nbx_neighbours.h) against the fp64 numpy reference
tests/neighbours_ref.py, as a context, as members of an ensemble and as members of one ragged ensemble.

What is asked: index and within EQUAL the reference -- the states have no ambiguous body at all, which test_neighbours_cpu.py
asserts with the reference alone (no second-nearest partner within a relative 16 u of the nearest, no r2 within 8 u of h2) -- and
r2 within 8 u of the reference's, u the unit round-off of the object's precision: the gate tests/test_timescale_gpu.py puts on
min_r2, the same arithmetic (5 u to first order).

Shapes, the smallest at which each part can go wrong: n = 257 (one split, two tiles, the last holding one body and 255 padding
records), n = 2049 (five columns, two splits of 5 and 4 tiles), n = 4097 (nine columns, four splits, the last one short),
lattice(13) = 2197 bodies (two splits meeting at j = 1280, so equal candidates arrive from both), n = 1 and n = 2."""
import ctypes
import math
import os
import sys
import zlib

import numpy as np
import pytest

import kick_ref as K
import neighbours_ref as R
from conftest import ROOT
from energy_ref import EPS2

pytestmark = pytest.mark.gpu

FAMILIES = {"box": R.box, "shifted": R.shifted, "reversed": R.reversed_box, "member": R.member}
_states, _refs, _ctx = {}, {}, {}


def state(precision, family, n):
    key = (precision, family, n)
    if key not in _states:
        if family.startswith("lattice"):
            _states[key] = R.lattice(R.LATTICE_K, precision, perm=family == "lattice permuted")
        else:
            _states[key] = FAMILIES[family](n, precision)
    return _states[key]


def ref(precision, family, n, radius=R.RADIUS):
    """The reference's values, computed once per state and radius and left unchanged."""
    key = (precision, family, n, radius)
    if key not in _refs:
        r = R.neighbours(state(precision, family, n), radius, precision)
        r["pairs"] = R.mutual_pairs(r["index"])
        for a in r.values():
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def context_values(nbx, precision, family, n, radius=R.RADIUS):
    """What a default context of n bodies holding the state returns, asked once per state: the bits the members are held to."""
    key = (precision, family, n, radius)
    if key not in _ctx:
        with nbx.Context(n, precision) as c:
            c.upload(state(precision, family, n))
            got = c.neighbours(radius)
            assert same(c.neighbours(radius), got)  # two calls in a row: the same bits
            got["min_r2"] = c.timescale()["min_r2"] if n > 1 else math.inf
        _ctx[key] = got
    return _ctx[key]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) if a[k] is not None else b[k] is None for k in R.KEYS)


def check(nbx, got, precision, family, n, radius=R.RADIUS):
    want = ref(precision, family, n, radius)
    assert got["index"].dtype == np.int32 and got["within"].dtype == np.int32 and got["r2"].dtype == R.DTYPE[precision]
    assert got["index"].shape == got["r2"].shape == got["within"].shape == (n,)
    if n == 1:  # no partner
        assert got["index"].tolist() == [-1] and got["r2"].tolist() == [math.inf] and got["within"].tolist() == [0]
        return
    dev = np.abs(got["r2"].astype(np.float64) - want["r2"]) / want["r2"] / R.U[precision]
    print("fp%d %s(%d) radius %g: %d indices and %d counts differ, r2 worst %.2f u, mean count %.1f"
          % (precision, family, n, radius, (got["index"] != want["index"]).sum(), (got["within"] != want["within"]).sum(), dev.max(),
             got["within"].mean()))
    assert np.array_equal(got["index"], want["index"]), (precision, family, n, np.nonzero(got["index"] != want["index"])[0][:8])
    assert np.array_equal(got["within"], want["within"]), (precision, family, n, np.nonzero(got["within"] != want["within"])[0][:8])
    assert dev.max() <= R.R2_GATE, (precision, family, n, dev.max())
    # the identities of the header
    assert (got["r2"][got["index"]] <= got["r2"]).all()  # if index[i] == j then r2[j] <= r2[i]
    assert np.array_equal(nbx.mutual_pairs(got["index"]), want["pairs"])


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("family", ["box", "shifted"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference(nbx, precision, family, n):
    got = context_values(nbx, precision, family, n)
    check(nbx, got, precision, family, n)
    assert float(got["r2"].min()) == got["min_r2"]  # bit for bit nbx_timescale_t.min_r2
    assert len(ref(precision, family, n)["pairs"]) > 50  # mutual pairs are there to be found


@pytest.mark.parametrize("family", ["lattice", "lattice permuted"])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_gives_the_lowest_index_face_neighbour_and_one_r2(nbx, precision, family):
    k = R.LATTICE_K
    n = k ** 3
    index, faces = R.lattice_expected(k, perm=family == "lattice permuted")
    got = context_values(nbx, precision, family, n, R.LATTICE_RADIUS)
    assert np.array_equal(got["index"], index), np.nonzero(got["index"] != index)[0][:8]
    assert len(set(got["r2"].tobytes()[i * got["r2"].itemsize:(i + 1) * got["r2"].itemsize] for i in range(n))) == 1  # the same bits for every body
    assert abs(float(got["r2"][0]) - (1.0 / 64 + EPS2)) <= R.R2_GATE * R.U[precision] * (1.0 / 64 + EPS2)
    assert np.array_equal(got["within"], faces) and sorted(set(faces.tolist())) == [3, 4, 5, 6]
    check(nbx, got, precision, family, n, R.LATTICE_RADIUS)
    assert float(got["r2"].min()) == got["min_r2"]
    tie = context_values(nbx, precision, family, n, R.LATTICE_TIE_RADIUS)  # h2 is bit for bit the face neighbours' r2: <= counts them
    assert np.array_equal(tie["within"], faces) and np.array_equal(tie["index"], index) and np.array_equal(tie["r2"], got["r2"])
    assert R.DTYPE[precision](R.h2_of(R.LATTICE_TIE_RADIUS, precision)) == got["r2"][0]


@pytest.mark.parametrize("precision", [32, 64])
def test_one_body_has_no_partner_and_two_bodies_have_each_other(nbx, precision):
    for n in (1, 2):
        got = context_values(nbx, precision, "member", n)
        check(nbx, got, precision, "member", n)
        assert float(got["r2"].min()) == got["min_r2"]
    two = context_values(nbx, precision, "member", 2, 10.0)
    assert two["index"].tolist() == [1, 0] and two["within"].tolist() == [1, 1] and two["r2"][0] == two["r2"][1]
    with nbx.Context(2, precision) as c:  # radius +infinity: every partner, and neither the body itself nor a padding record
        c.upload(state(precision, "member", 2))
        assert c.neighbours(math.inf)["within"].tolist() == [1, 1]
        assert c.neighbours(0.0)["within"].tolist() == [0, 0]


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_reference_and_have_the_bits_of_a_context(nbx, precision, n):
    families = ("box", "shifted", "reversed")
    S = len(families)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload([state(precision, f, n) for f in families])
        full = e.neighbours(R.RADIUS)
        assert same(e.neighbours(R.RADIUS), full) and all(full[k].shape == (S, n) for k in R.KEYS)
        for m, f in enumerate(families):
            got = {k: full[k][m] for k in R.KEYS}
            check(nbx, got, precision, f, n)
            assert same(got, context_values(nbx, precision, f, n)), (precision, n, f)
        # a member's results are the same whatever first and count it was asked with: a sub-range, single members, empty ranges
        for first, count in ((1, 2), (0, 1), (1, 1), (2, 1), (0, 2), (S, 0), (0, 0)):
            part = e.neighbours(R.RADIUS, first, count)
            assert all(np.array_equal(part[k], full[k][first:first + count]) for k in R.KEYS), (first, count)
        assert same(e.neighbours(R.RADIUS, first=1), {k: full[k][1:] for k in R.KEYS})
        assert same(e.neighbours(R.RADIUS), full)


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    with nbx.Ragged(sizes, precision) as r:
        r.upload([state(precision, "member", n) for n in sizes])
        full = r.neighbours(R.RADIUS)
        assert len(full) == S and all(same(a, b) for a, b in zip(r.neighbours(R.RADIUS), full))
        for m, n in enumerate(sizes):
            check(nbx, full[m], precision, "member", n)
            assert same(full[m], context_values(nbx, precision, "member", n)), (precision, n)
        for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (0, 1), (1, 3), (5, 3), (S, 0), (3, 0)):
            part = r.neighbours(R.RADIUS, first, count)
            assert len(part) == count and all(same(a, b) for a, b in zip(part, full[first:first + count])), (first, count)
        assert all(same(a, b) for a, b in zip(r.neighbours(R.RADIUS, first=5), full[5:]))
        assert all(same(a, b) for a, b in zip(r.neighbours(R.RADIUS), full))  # a partial call leaves nothing behind that a full one sees
        # the layout is end to end, member `first` at element 0, and nothing is written behind the last member
        first, count = 2, 4
        total = sum(sizes[first:first + count])
        flat = [np.full(total + 8, -7, dtype=np.int32), np.full(total + 8, -7.25, dtype=R.DTYPE[precision]), np.full(total + 8, -7, dtype=np.int32)]
        assert nbx.load().nbx_ragged_neighbours(r._h, first, count, R.RADIUS, *[a.ctypes.data_as(ctypes.c_void_p) for a in flat]) == nbx.NBX_OK
        for a, k in zip(flat, R.KEYS):
            assert np.array_equal(a[:total], np.concatenate([full[m][k] for m in range(first, first + count)])), k
            assert (a[total:] == a.dtype.type(-7 if k != "r2" else -7.25)).all(), k
    # the same systems in another order: other neighbours, other offsets, other rows -- the same bits
    with nbx.Ragged(sizes[::-1], precision) as r:
        r.upload([state(precision, "member", n) for n in sizes][::-1])
        assert all(same(a, b) for a, b in zip(r.neighbours(R.RADIUS), full[::-1]))


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 4)] +
    [dict(kernel_variant="KERNEL_SGPRW", bodies_per_lane=2), dict(kernel_variant="KERNEL_JLANE", bodies_per_lane=4)] +
    [dict(j_split=s) for s in (1, 4, 32)] + [dict(kernel_variant="KERNEL_LDS", j_split=4)])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_bits_do_not_depend_on_the_contexts_options_and_a_sliced_context_returns_the_whole_ones(nbx, precision):
    n = 2049
    s = state(precision, "box", n)
    want = context_values(nbx, precision, "box", n)
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
            assert same(c.neighbours(R.RADIUS), want), (o, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    print("fp%d: %d of %d option sets made a context; distinct shapes: %d" % (precision, len(made), len(CONTEXT_OPTIONS), len(set(made))))
    assert {m[0] for m in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR} and {m[1] for m in made} == {nbx.ORDER_TREE, nbx.ORDER_REFERENCE}
    assert len(set(made)) >= 6
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # all n positions are resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as c:
            c.upload(s)
            got = c.neighbours(R.RADIUS)
            assert all(got[k].shape == (n,) for k in R.KEYS) and same(got, want), (i_begin, i_count)


def _raw(nbx, o, kind, radius, arrays, first=0, count=None):
    L = nbx.load()
    ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    if kind == "context":
        return L.nbx_neighbours(o._h, radius, *ptr)
    f = L.nbx_ensemble_neighbours if kind == "ensemble" else L.nbx_ragged_neighbours
    return f(o._h, first, o.members if count is None else count, radius, *ptr)


def _make(nbx, kind, precision=32):
    """An object of the kind with its states and the number of bodies a call over all of it returns."""
    sizes = (257, 2049, 513)
    if kind == "context":
        return nbx.Context(2049, precision), state(precision, "box", 2049), 2049
    if kind == "ensemble":
        return nbx.Ensemble(2049, 3, precision), [state(precision, f, 2049) for f in ("box", "shifted", "reversed")], 3 * 2049
    return nbx.Ragged(sizes, precision), [state(precision, "member", n) for n in sizes], sum(sizes)


def _flatten(res):
    if isinstance(res, dict):
        return {k: None if res[k] is None else res[k].reshape(-1) for k in R.KEYS}
    return {k: None if res[0][k] is None else np.concatenate([m[k] for m in res]) for k in R.KEYS}


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_null_output_is_skipped_alone_and_without_a_radius_the_count_is_not_asked_for(nbx, precision, kind):
    o, states, total = _make(nbx, kind, precision)
    T = R.DTYPE[precision]
    with o:
        o.upload(states)
        full = _flatten(o.neighbours(R.RADIUS))
        assert full["within"].sum() > 0
        for skip in range(3):
            arrays = [np.full(total, -7, dtype=np.int32), np.full(total, -7.25, dtype=T), np.full(total, -7, dtype=np.int32)]
            keep = list(arrays)
            arrays[skip] = None
            assert _raw(nbx, o, kind, R.RADIUS, arrays) == nbx.NBX_OK
            for k, a in enumerate(keep):
                if k == skip:
                    assert (a == a.dtype.type(-7.25 if k == 1 else -7)).all()  # never written
                else:
                    assert np.array_equal(a, full[R.KEYS[k]]), (skip, k)
        # all NULL: the arguments are checked, nothing is launched
        assert _raw(nbx, o, kind, R.RADIUS, [None] * 3) == nbx.NBX_OK
        assert _raw(nbx, o, kind, -1.0, [None] * 3) == nbx.NBX_ERR_ARG and b"radius is NaN or negative" in nbx.load().nbx_last_error()
        # radius=None: within is None, index and r2 are those of a call with a radius -- from the kernels compiled without the count
        plain = _flatten(o.neighbours())
        assert plain["within"] is None and np.array_equal(plain["index"], full["index"]) and np.array_equal(plain["r2"], full["r2"])
        other = _flatten(o.neighbours(0.05))
        assert np.array_equal(other["index"], full["index"]) and np.array_equal(other["r2"], full["r2"]) and other["within"].sum() < full["within"].sum()


def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


def _positions(down):
    if isinstance(down, dict):
        return [down[f] for f in K.FIELDS[:6]]
    return [d[f] for d in down for f in K.FIELDS[:6]]


UNTOUCHED = ("steps_done", "force_launches_timed", "force_ms_total", "launches_timed", "step_ms_total", "graph_replays")


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_the_call_is_on_the_stream_and_leaves_the_trajectory_and_every_counter_alone(nbx, kind):
    dt = 1.0 / 256
    o, states, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        n3 = _flatten(o.neighbours(R.RADIUS))
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        again = _flatten(o.neighbours(R.RADIUS))
        after = o.stats()
        assert {k: before[k] for k in UNTOUCHED if k in before} == {k: after[k] for k in UNTOUCHED if k in after} and before["steps_done"] == 3
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        ke_a = o.step(3, dt)
        a = _positions(o.download())
    assert same(n3, again)
    o, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.step(3, dt)  # synchronises
        o.sync()
        assert same(_flatten(o.neighbours(R.RADIUS)), n3)
    o, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        n0 = _flatten(o.neighbours(R.RADIUS))
        ke_b = o.step(6, dt)
        b = _positions(o.download())
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)  # the bits of later steps are as without the call
    assert not np.array_equal(n0["r2"], n3["r2"])


def test_state_errors(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    with nbx.Context(300, 32) as c:
        for radius in (R.RADIUS, None):
            with pytest.raises(nbx.NbxError) as err:
                c.neighbours(radius)
            assert err.value.code == nbx.NBX_ERR_STATE and "nbx_neighbours: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        assert c.neighbours(R.RADIUS)["index"].shape == (300,)
        for radius in (-0.5, math.nan):
            with pytest.raises(nbx.NbxError) as err:
                c.neighbours(radius)
            assert err.value.code == nbx.NBX_ERR_ARG and "nbx_neighbours: radius is NaN or negative" in str(err.value)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.neighbours(R.RADIUS)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_neighbours: a local step awaits nbx_commit" in str(err.value)
        assert _raw(nbx, c, "context", R.RADIUS, [None] * 3) == nbx.NBX_ERR_STATE  # the state comes before "nothing to do"
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_neighbours"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_neighbours")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.neighbours(R.RADIUS)
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.neighbours(R.RADIUS, first, count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value), (first, count)
            part = _flatten(o.neighbours(R.RADIUS, 0, 3))  # the uploaded members can be asked before the others arrive
            assert part["index"].shape == (sum(len(s["mass"]) for s in st[:3]),)
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.neighbours(R.RADIUS, first, count)
                assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value), (first, count)
            with pytest.raises(nbx.NbxError) as err:
                o.neighbours(-1.0, 0, S + 1)
            assert "radius is NaN or negative" in str(err.value)  # the radius comes before the range
            o.upload(st[3:], first=3)
            assert same(_flatten(o.neighbours(R.RADIUS, 0, 3)), part)


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32: one batch call against 16
    nbx_neighbours calls on contexts created and uploaded beforehand, in this process, rounds alternated
    (tools/neighbours_cost.py).  The pair work of the two arms is the same and one call issues 2 launches and 1 synchronisation
    where the contexts issue 32 and 16, so the gate has no further margin: ratio <= 1.0, the condition every batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import neighbours_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = neighbours_cost.measure(nbx, kind)
        print("%s fp32: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["batch_us"], r["contexts_us"], r["ratio"]))
        cells[kind] = r
    neighbours_cost.write(neighbours_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
