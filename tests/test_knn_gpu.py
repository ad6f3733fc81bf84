"""The k nearest neighbours of every body on the device (include/nbx_knn.h) against the fp64 numpy reference tests/knn_ref.py, as
a context, as members of an ensemble and as members of one ragged ensemble.

What is asked (knn_ref.differs): (a) every r2[i, q] within 8 u of the reference's q-th value, u the unit round-off of the
object's precision; (b) every returned j a partner, once per row, whose own r2 is within 8 u of the returned one; (c) index
EQUAL to the reference -- the states have no ambiguous body (no two consecutive values among a body's first k + 1 within a
relative 16 u), which each test asserts first and test_knn_cpu.py asserts with the reference alone; the one exception is
shifted(4097) in fp32 at k = 16, which has one such body and is held to (a) and (b).  On the lattices, whose r2 are exact and
tied, the index must equal the closed form on every body and every r2 must be the bits of its distance class.

Shapes, the smallest at which each part can go wrong: n = 257 (one split, two tiles, the last holding one body and 255 padding
records), n = 2049 (five columns, two splits of 5 and 4 tiles), n = 4097 (nine columns, four splits, the last one short),
lattice(13) = 2197 bodies (two splits meeting at j = 1280, so equal candidates arrive from both), lattice(33) = 35937 bodies
(71 columns x 15 splits: every row a 15-way merge of tied values), n = 1, 2, 5 and 17 (fewer partners than k)."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

import kick_ref as K
import knn_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

FAMILIES = {"box": R.box, "shifted": R.shifted, "reversed": R.reversed_box, "member": R.member}
_states, _refs, _ctx, _nb = {}, {}, {}, {}


def state(precision, family, n):
    key = (precision, family, n)
    if key not in _states:
        if family.startswith("lattice"):
            _states[key] = R.lattice(round(n ** (1.0 / 3)), precision, perm=family == "lattice permuted")
        else:
            _states[key] = FAMILIES[family](n, precision)
    return _states[key]


def ref(precision, family, n):
    """The reference's rows for k = 16 -- every smaller k is their prefix -- and the ambiguity gaps, computed once per state and
    left unchanged."""
    key = (precision, family, n)
    if key not in _refs:
        st = state(precision, family, n)
        r = R.knn(st, R.KNN_MAX, precision)
        r["gap"] = R.first_gap(st, precision)
        for a in r.values():
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def want_k(precision, family, n, k):
    r = ref(precision, family, n)
    return {"index": r["index"][:, :k], "r2": r["r2"][:, :k]}


def context_values(nbx, precision, family, n, k):
    """What a default context of n bodies holding the state returns for k, asked once: the bits the members are held to."""
    key = (precision, family, n, k)
    if key not in _ctx:
        with nbx.Context(n, precision) as c:
            c.upload(state(precision, family, n))
            for kk in R.KS:
                got = c.knn(kk)
                assert same(c.knn(kk), got)  # two calls in a row: the same bits
                _ctx[(precision, family, n, kk)] = got
            _nb[(precision, family, n)] = c.neighbours(R.RADIUS)
    return _ctx[key]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in R.KEYS)


def check(got, precision, family, n, k, index=True, exact=False):
    T = R.DTYPE[precision]
    assert got["index"].dtype == np.int32 and got["r2"].dtype == T and got["index"].shape == got["r2"].shape == (n, k)
    found = R.differs(got, want_k(precision, family, n, k), state(precision, family, n), precision, index=index, exact=exact,
                      gap=ref(precision, family, n)["gap"])
    assert not found, (precision, family, n, k, found)
    # the identities of the header: rows ascend in (r2, j)
    r2, j = got["r2"].astype(np.float64), got["index"].astype(np.int64)
    fin = np.isfinite(r2)
    both = fin[:, 1:] & fin[:, :-1]
    assert (r2[:, 1:][both] >= r2[:, :-1][both]).all()
    tie = both & (r2[:, 1:] == r2[:, :-1])
    assert (j[:, 1:][tie] > j[:, :-1][tie]).all()
    assert (~fin[:, :-1] <= ~fin[:, 1:]).all()  # the fill is at the end


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("family", ["box", "shifted", "reversed"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference_neighbours_and_its_own_prefixes(nbx, precision, family, n):
    st = state(precision, family, n)
    gap = ref(precision, family, n)["gap"]
    full = context_values(nbx, precision, family, n, 16)
    nb = _nb[(precision, family, n)]
    for k in R.KS:
        got = context_values(nbx, precision, family, n, k)
        amb = R.ambiguous(st, k, precision, gap)
        capped = (precision, family, n, k) == (32, "shifted", 4097, 16)  # one ambiguous body: (a) and (b) only
        assert amb == (1 if capped else 0), (precision, family, n, k, amb)
        check(got, precision, family, n, k, index=not capped)
        # column 0 is bit for bit nbx_neighbours' index and r2
        assert np.array_equal(got["index"][:, 0], nb["index"]) and np.array_equal(got["r2"][:, 0], nb["r2"]), k
        # the result for k is bit for bit the first k columns of the result for 16: 1 through capacity 4, 6 and 8 through 8
        assert np.array_equal(got["index"], full["index"][:, :k]) and np.array_equal(got["r2"], full["r2"][:, :k]), k
        # #(r2[i, :] <= h2) == min(within[i], k) with nbx_neighbours' h2 and within
        h2 = R.DTYPE[precision](R.N.h2_of(R.RADIUS, precision))
        assert np.array_equal((got["r2"] <= h2).sum(axis=1), np.minimum(nb["within"], k)), k
    if n == 4097:
        assert (nb["within"] > 16).any() and (nb["within"] < 16).any()  # both sides of the min


@pytest.mark.parametrize("precision", [32, 64])
def test_systems_with_fewer_partners_than_k_give_exact_fill(nbx, precision):
    for n in (1, 2, 5, 17):
        for k in (1, 6, 16):
            got = context_values(nbx, precision, "member", n, k)
            check(got, precision, "member", n, k)
            have = min(k, n - 1)
            assert (got["index"][:, have:] == -1).all() and np.isposinf(got["r2"][:, have:]).all()
            assert (got["index"][:, :have] >= 0).all() and np.isfinite(got["r2"][:, :have]).all()
            assert np.array_equal(got["index"], want_k(precision, "member", n, k)["index"])
    one = context_values(nbx, precision, "member", 1, 6)
    assert one["index"].tolist() == [[-1] * 6] and np.isposinf(one["r2"]).all()  # a system of one body is all fill


@pytest.mark.parametrize("family", ["lattice", "lattice permuted"])
@pytest.mark.parametrize("kk", [13, 33])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattices_give_the_closed_form_index_and_the_bits_of_every_distance_class(nbx, precision, kk, family):
    n = kk ** 3
    T = R.DTYPE[precision]
    perm = family == "lattice permuted"
    with nbx.Context(n, precision) as c:
        c.upload(state(precision, family, n))
        res = {k: c.knn(k) for k in (6, 16)}
        nb = c.neighbours()
    for k, got in res.items():
        exp = R.lattice_expected(kk, k, precision, perm)
        bad = np.nonzero((got["index"] != exp["index"]).any(axis=1))[0]
        assert not len(bad), (precision, kk, family, k, len(bad), bad[:8])
        assert np.array_equal(got["r2"], exp["r2"].astype(T)), (precision, kk, family, k)  # the bits of the distance class
        assert np.array_equal(got["index"][:, 0], nb["index"]) and np.array_equal(got["r2"][:, 0], nb["r2"])
    assert same({key: res[16][key][:, :6] for key in R.KEYS}, res[6])
    if kk == 13:
        for k in (6, 16):
            check(res[k], precision, family, n, k, exact=True)


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 4)] +
    [dict(kernel_variant="KERNEL_SGPRW", bodies_per_lane=2), dict(kernel_variant="KERNEL_JLANE", bodies_per_lane=4)] +
    [dict(j_split=s) for s in (1, 4, 32)] + [dict(kernel_variant="KERNEL_LDS", j_split=4)])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_bits_do_not_depend_on_the_contexts_options_and_a_sliced_context_returns_the_whole_ones(nbx, precision):
    n = 2049
    s = state(precision, "box", n)
    want = {k: context_values(nbx, precision, "box", n, k) for k in (6, 16)}
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
            for k in (6, 16):
                assert same(c.knn(k), want[k]), (o, k, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    assert {m[0] for m in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR} and {m[1] for m in made} == {nbx.ORDER_TREE, nbx.ORDER_REFERENCE}
    assert len(set(made)) >= 6
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # all n positions are resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as c:
            c.upload(s)
            for k in (6, 16):
                got = c.knn(k)
                assert got["index"].shape == (n, k) and same(got, want[k]), (i_begin, i_count, k)


@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_have_the_bits_of_a_context_over_the_whole_range_and_over_sub_ranges(nbx, precision):
    n, S = 2049, 16
    states = [state(precision, "box", n), state(precision, "shifted", n), state(precision, "reversed", n)]
    states += [K.make_state(400 + m, n, R.DTYPE[precision]) for m in range(3, S)]
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        full = {k: e.knn(k) for k in (6, 16)}
        for k in (6, 16):
            assert all(full[k][key].shape == (S, n, k) for key in R.KEYS) and same(e.knn(k), full[k])
            for m, f in enumerate(("box", "shifted", "reversed")):
                assert same({key: full[k][key][m] for key in R.KEYS}, context_values(nbx, precision, f, n, k)), (precision, k, f)
        check({key: full[6][key][0] for key in R.KEYS}, precision, "box", n, 6)
        for m in range(3, S):  # the members that are no cached state: a context of their own each
            with nbx.Context(n, precision) as c:
                c.upload(states[m])
                for k in (6, 16):
                    assert same({key: full[k][key][m] for key in R.KEYS}, c.knn(k)), (precision, k, m)
        # a member's rows are the same whatever first and count it was asked with: sub-ranges, single members, empty ranges
        for first, count in ((1, 2), (0, 1), (5, 7), (S - 1, 1), (S, 0), (0, 0)):
            part = e.knn(6, first, count)
            assert all(np.array_equal(part[key], full[6][key][first:first + count]) for key in R.KEYS), (first, count)
        assert same(e.knn(16, first=11), {key: full[16][key][11:] for key in R.KEYS})
        assert same(e.knn(6), full[6])


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    T = R.DTYPE[precision]
    with nbx.Ragged(sizes, precision) as r:
        r.upload([state(precision, "member", n) for n in sizes])
        full = {k: r.knn(k) for k in (6, 16)}
        for k in (6, 16):
            assert len(full[k]) == S and all(same(a, b) for a, b in zip(r.knn(k), full[k]))
            for m, n in enumerate(sizes):
                assert R.ambiguous(state(precision, "member", n), k, precision, ref(precision, "member", n)["gap"]) == 0
                check(full[k][m], precision, "member", n, k)
                assert same(full[k][m], context_values(nbx, precision, "member", n, k)), (precision, k, n)
        for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (0, 1), (1, 3), (5, 3), (S, 0), (3, 0)):
            part = r.knn(6, first, count)
            assert len(part) == count and all(same(a, b) for a, b in zip(part, full[6][first:first + count])), (first, count)
        assert all(same(a, b) for a, b in zip(r.knn(16, first=5), full[16][5:]))
        assert all(same(a, b) for a, b in zip(r.knn(6), full[6]))  # a partial call leaves nothing behind that a full one sees
        # the layout is end to end and body-major, member `first` at row 0, and nothing is written behind the last member
        first, count, k = 2, 4, 6
        total = sum(sizes[first:first + count]) * k
        flat = [np.full(total + 8, -7, dtype=np.int32), np.full(total + 8, -7.25, dtype=T)]
        assert nbx.load().nbx_ragged_knn(r._h, first, count, k, *[a.ctypes.data_as(ctypes.c_void_p) for a in flat]) == nbx.NBX_OK
        for a, key in zip(flat, R.KEYS):
            assert np.array_equal(a[:total], np.concatenate([full[k][m][key].reshape(-1) for m in range(first, first + count)])), key
            assert (a[total:] == a.dtype.type(-7 if key == "index" else -7.25)).all(), key
    # the same systems in another order: other offsets, other rows -- the same bits
    with nbx.Ragged(sizes[::-1], precision) as r:
        r.upload([state(precision, "member", n) for n in sizes][::-1])
        assert all(same(a, b) for a, b in zip(r.knn(16), full[16][::-1]))


def _raw(nbx, o, kind, k, arrays, first=0, count=None):
    L = nbx.load()
    ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    if kind == "context":
        return L.nbx_knn(o._h, k, *ptr)
    f = L.nbx_ensemble_knn if kind == "ensemble" else L.nbx_ragged_knn
    return f(o._h, first, o.members if count is None else count, k, *ptr)


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
        return {k: res[k].reshape(-1) for k in res}
    return {k: np.concatenate([m[k].reshape(-1) for m in res]) for k in res[0]}


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_null_output_is_skipped_alone_and_k_is_checked_even_when_nothing_is_asked_for(nbx, precision, kind):
    o, states, total = _make(nbx, kind, precision)
    T = R.DTYPE[precision]
    k = 6
    with o:
        o.upload(states)
        full = _flatten(o.knn(k))
        for skip in range(2):
            arrays = [np.full(total * k, -7, dtype=np.int32), np.full(total * k, -7.25, dtype=T)]
            keep = list(arrays)
            arrays[skip] = None
            assert _raw(nbx, o, kind, k, arrays) == nbx.NBX_OK
            for q, a in enumerate(keep):
                if q == skip:
                    assert (a == a.dtype.type(-7.25 if q == 1 else -7)).all()  # never written
                else:
                    assert np.array_equal(a, full[R.KEYS[q]]), (skip, q)
        assert _raw(nbx, o, kind, k, [None] * 2) == nbx.NBX_OK  # both NULL: the arguments are checked, nothing is launched
        for bad in (0, 17, -3):
            assert _raw(nbx, o, kind, bad, [None] * 2) == nbx.NBX_ERR_ARG and b"k is outside [1, 16]" in nbx.load().nbx_last_error()
            with pytest.raises(nbx.NbxError) as err:
                o.knn(bad)
            assert err.value.code == nbx.NBX_ERR_ARG


def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


def _positions(down):
    if isinstance(down, dict):
        return [down[f] for f in K.FIELDS[:6]]
    return [d[f] for d in down for f in K.FIELDS[:6]]


UNTOUCHED = ("steps_done", "force_launches_timed", "force_ms_total", "launches_timed", "step_ms_total", "graph_replays")


def _diag_values(o):
    d = o.diagnostics()
    return [sorted(x.items()) for x in (d if isinstance(d, list) else [d])]


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_the_call_is_on_the_stream_and_leaves_the_trajectory_and_every_counter_alone(nbx, kind):
    dt = 1.0 / 256
    o, states, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        k3 = _flatten(o.knn(6))
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        again = _flatten(o.knn(6))
        _flatten(o.knn(16))
        after = o.stats()
        assert {k: before[k] for k in UNTOUCHED if k in before} == {k: after[k] for k in UNTOUCHED if k in after} and before["steps_done"] == 3
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        diag_a = _diag_values(o)
        nb_a = _flatten(o.neighbours(R.RADIUS))
        ke_a = o.step(3, dt)
        a = _positions(o.download())
    assert same(k3, again)
    o, _, _ = _make(nbx, kind)
    with o:  # the same course without the call
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)
        o.sync()
        diag_b = _diag_values(o)
        nb_b = _flatten(o.neighbours(R.RADIUS))
        ke_b = o.step(3, dt)
        b = _positions(o.download())
        k6 = _flatten(o.knn(6))
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)  # the bits of later steps are as without the call
    assert diag_a == diag_b and all(np.array_equal(nb_a[k], nb_b[k]) for k in nb_a)
    assert not np.array_equal(k6["r2"], k3["r2"])  # and the call does follow the state


def test_state_errors(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.knn(6)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_knn: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        assert c.knn(6)["index"].shape == (300, 6)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.knn(6)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_knn: a local step awaits nbx_commit" in str(err.value)
        assert _raw(nbx, c, "context", 6, [None] * 2) == nbx.NBX_ERR_STATE  # the state comes before "nothing to do"
        assert _raw(nbx, c, "context", 0, [None] * 2) == nbx.NBX_ERR_ARG  # and k before the state
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_knn"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_knn")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.knn(6)
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.knn(6, first, count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value), (first, count)
            part = _flatten(o.knn(6, 0, 3))  # the uploaded members can be asked before the others arrive
            assert part["index"].shape == (6 * sum(len(s["mass"]) for s in st[:3]),)
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.knn(6, first, count)
                assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value), (first, count)
            with pytest.raises(nbx.NbxError) as err:
                o.knn(17, 0, S + 1)
            assert "k is outside [1, 16]" in str(err.value)  # k comes before the range
            o.upload(st[3:], first=3)
            assert all(np.array_equal(_flatten(o.knn(6, 0, 3))[k], part[k]) for k in part)


def test_the_size_bound_scales_with_k(nbx):
    """2^22 entries per call: 262144 bodies pass at k = 16 and 262145 do not; the same context is served at k = 8."""
    n = (1 << 18) + 1
    with nbx.Context(n, 32) as c:
        c.upload(K.make_state(77, n, np.float32))
        with pytest.raises(nbx.NbxError) as err:
            c.knn(16)
        assert err.value.code == nbx.NBX_ERR_ARG and "nbx_knn: n * k exceeds 4194304" in str(err.value)
        assert nbx.load().nbx_knn(c._h, 16, None, None) == nbx.NBX_ERR_ARG  # also when nothing is asked for
        assert nbx.load().nbx_knn(c._h, 8, None, None) == nbx.NBX_OK


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32, k = 6: one batch call against 16
    nbx_knn calls on contexts created and uploaded beforehand, in this process, rounds alternated (tools/knn_cost.py).  The pair
    work of the two arms is the same and one call issues 2 launches and 1 synchronisation where the contexts issue 32 and 16, so
    the gate has no further margin: ratio <= 1.0, the condition every batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import knn_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = knn_cost.measure(nbx, kind)
        print("%s fp32 k = %d: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["k"], r["batch_us"], r["contexts_us"], r["ratio"]))
        cells[kind] = r
    for kind, r in cells.items():
        assert r["members"] == 16 and r["k"] == 6 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
