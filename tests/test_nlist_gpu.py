"""Neighbour lists on the device (include/nbx_nlist.h) against the fp64 numpy reference tests/nlist_ref.py, as a context, as members
of an ensemble and as members of one ragged ensemble.

What is asked (nlist_ref.differs): offsets, total and index EQUAL to the reference's, every r2 within 8 u of it.  Every (state,
radius) compared that way is unambiguous -- no pair's r2 within 8 u of h2 -- which test_nlist_cpu.py shows for every one of them
with the reference alone (nlist_ref.cases, ensemble_states, ragged_states); the radii come from nlist_ref.pick_radius.  The exact
relations of the header are held against neighbours(), paircount(), knn(16) and fof() of the SAME object: integers and bit
patterns on both sides, no reference and no ambiguity argument.

Shapes, the smallest at which each part can go wrong: n = 1 and 2; 255, 256, 257 (one tile, a full tile, two tiles with padding);
511, 512, 513 (the lane's second body, then two columns); 1025; 2049 (two splits, and the scan's first block seam); 4097 (four
splits, the last one short, and two scan seams); +inf as the radius, where every list crosses every tile and split seam;
lattice(33) = 35937 bodies (71 columns x 15 splits, 18 scan blocks) and lattice(81) = 531441 bodies (260 scan blocks)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import kick_ref as K
import lattice_ref as L
import nlist_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

_refs, _ctx = {}, {}
BITS = {32: np.uint32, 64: np.uint64}


def ref(key, st, radius, precision):
    """The reference's lists for a case, computed once and left unchanged."""
    if key not in _refs:
        want = R.nlist(st, radius, precision)
        for k in ("offsets", "index", "r2"):
            want[k].setflags(write=False)
        _refs[key] = want
    return _refs[key]


def same(a, b):
    """The same bytes."""
    return (int(a["total"]) == int(b["total"]) and np.array_equal(a["offsets"], b["offsets"]) and a["index"].tobytes() == b["index"].tobytes() and
            a["r2"].tobytes() == b["r2"].tobytes())


def typed(got, bodies, precision):
    assert got["offsets"].dtype == np.int64 and got["offsets"].shape == (bodies + 1,) and got["index"].dtype == np.int32
    assert got["r2"].dtype == R.DTYPE[precision] and got["index"].shape == got["r2"].shape == (got["total"],)
    assert got["offsets"][0] == 0 and got["offsets"][-1] == got["total"]
    return got


def context_lists(nbx, key, st, radius, precision):
    """What a default context holding the state returns, asked once per case: the bits the members are held to."""
    if key not in _ctx:
        n = len(st["mass"])
        with nbx.Context(n, precision) as c:
            c.upload(st)
            _ctx[key] = typed(c.nlist(radius), n, precision)
    return _ctx[key]


def symmetric(nl, n, precision):
    """j in list(i) <=> i in list(j), with the same r2 bits."""
    e = R.body_of_entry(nl["offsets"])
    j = nl["index"].astype(np.int64)
    bits = nl["r2"].view(BITS[precision])
    if n <= 4097:  # dense
        there = np.zeros((n, n), dtype=bool)
        value = np.zeros((n, n), dtype=bits.dtype)
        there[e, j] = True
        value[e, j] = bits
        return bool(np.array_equal(there, there.T) and np.array_equal(value, value.T))
    key = e * n + j  # ascending as the lists are
    back = j * n + e
    order = np.argsort(back, kind="stable")
    return bool(np.array_equal(back[order], key) and np.array_equal(bits[order], bits))


def relations(o, nl, radius, n, precision, what):
    """The exact statements of the header, against the other analysis calls of the same context `o`."""
    off, idx, r2 = nl["offsets"], nl["index"].astype(np.int64), nl["r2"]
    cnt = np.diff(off)
    e = R.body_of_entry(off)
    nb = o.neighbours(radius)
    # every j is a body of the system and not the body itself; strictly ascending within a list
    assert ((idx >= 0) & (idx < n) & (idx != e)).all(), what
    if len(idx) > 1:
        assert (np.diff(idx)[e[1:] == e[:-1]] > 0).all(), what
    assert np.array_equal(cnt, nb["within"].astype(np.int64)), what
    assert nl["total"] == 2 * int(o.paircount([radius])[0]), what
    assert symmetric(nl, n, precision), what
    # the entry with the smallest (r2, j) is the nearest neighbour
    some = cnt > 0
    if some.any():
        starts = off[:-1][some]
        least = np.minimum.reduceat(r2, starts)
        is_least = r2 == np.repeat(least, cnt[some])
        first = np.minimum.reduceat(np.where(is_least, idx, n), starts)
        assert np.array_equal(first, nb["index"][some]) and least.tobytes() == nb["r2"][some].tobytes(), what
    # where within <= 16 the list as a set is the k-NN prefix, r2 bit for bit
    knn = o.knn(16)
    few = cnt <= 16
    place = np.arange(len(idx)) - off[e]
    m = few[e]
    mine_j = np.full((n, 16), n, dtype=np.int64)
    mine_b = np.zeros((n, 16), dtype=BITS[precision])
    mine_j[e[m], place[m]] = idx[m]
    mine_b[e[m], place[m]] = r2.view(BITS[precision])[m]
    cols = np.arange(16)[None, :] < cnt[:, None]
    theirs_j = np.where(cols, knn["index"].astype(np.int64), n)
    theirs_b = np.where(cols, np.ascontiguousarray(knn["r2"]).view(BITS[precision]), 0)
    order = np.argsort(theirs_j, axis=1, kind="stable")
    assert np.array_equal(np.take_along_axis(theirs_j, order, axis=1)[few], mine_j[few]), what
    assert np.array_equal(np.take_along_axis(theirs_b, order, axis=1)[few], mine_b[few]), what
    # the components of the graph are the friends-of-friends groups
    assert np.array_equal(R.components(nl, n), o.fof(radius)["label"].astype(np.int64)), what


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference_and_the_other_analysis_calls_at_five_radii(nbx, precision, n):
    for name, st, radius in R.cases(precision, n):
        key = (precision, n, name)
        want = ref(key, st, radius, precision)
        with nbx.Context(n, precision) as c:
            c.upload(st)
            got = typed(c.nlist(radius), n, precision)
            print("fp%d n = %d %s r = %.5f: total %d, %.2f per body" % (precision, n, name, radius, got["total"], got["total"] / n))
            found = R.differs(got, want, precision)
            assert not found, (key, found)
            relations(c, got, radius, n, precision, key)
        if name == "inf":
            assert got["total"] == n * (n - 1) and np.array_equal(np.diff(got["offsets"]), np.full(n, n - 1))
        if name == "zero":  # two planted coincident bodies list each other with r2 = eps2, nobody else lists anybody
            assert got["index"].tolist() == ([n - 1, 0] if n >= 2 else []) and (got["r2"] == R.DTYPE[precision](R.EPS2)).all()
        if name == "r1":
            _ctx[key] = got


def _raw(nbx, o, kind, radius, capacity, arrays, first=0, count=None):
    L_ = nbx.load()
    ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    if kind == "context":
        return L_.nbx_nlist(o._h, radius, capacity, *ptr)
    f = L_.nbx_ensemble_nlist if kind == "ensemble" else L_.nbx_ragged_nlist
    return f(o._h, first, o.members if count is None else count, radius, capacity, *ptr)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_two_call_protocol(nbx, precision):
    n = 2049
    T = R.DTYPE[precision]
    _, st, sparse = R.cases(precision, n)[1]
    dense = R.cases(precision, n)[2][2]  # about 40 per body: more than nlist()'s first guess of 16
    with nbx.Context(n, precision) as c:
        c.upload(st)
        for radius in (sparse, dense):
            want = ref((precision, n, radius), st, radius, precision)
            t = want["total"]
            got = typed(c.nlist(radius), n, precision)  # capacity None: one call, or two where 16 per body do not hold it
            assert not R.differs(got, want, precision) and (t > 16 * n) == (radius == dense)
            # the counting call: the same offsets and total as a filling call
            off, total = np.full(n + 1, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
            assert _raw(nbx, c, "context", radius, 0, [off, None, None, total]) == nbx.NBX_OK
            assert np.array_equal(off, got["offsets"]) and total[0] == t
            counted = c.nlist(radius, 0)
            assert counted["index"] is None and counted["r2"] is None and counted["total"] == t and np.array_equal(counted["offsets"], off)
            # capacity == total fills, and nothing behind the total is written
            index, r2 = np.full(t + 8, -7, dtype=np.int32), np.full(t + 8, -7.25, dtype=T)
            off[:], total[:] = -7, -7
            assert _raw(nbx, c, "context", radius, t, [off, index, r2, total]) == nbx.NBX_OK
            assert same({"offsets": off, "index": index[:t], "r2": r2[:t], "total": total[0]}, got)
            assert (index[t:] == -7).all() and (r2[t:] == T(-7.25)).all()
            # capacity == total - 1 leaves the lists untouched, writes offsets and total, and returns NBX_OK
            index[:], r2[:], off[:], total[:] = -7, -7.25, -7, -7
            assert _raw(nbx, c, "context", radius, t - 1, [off, index, r2, total]) == nbx.NBX_OK
            assert (index == -7).all() and (r2 == T(-7.25)).all() and np.array_equal(off, got["offsets"]) and total[0] == t
            assert c.nlist(radius, t - 1)["index"] is None and same(c.nlist(radius, t), got) and same(c.nlist(radius, t + 100), got)
            # index alone and r2 alone
            assert _raw(nbx, c, "context", radius, t, [off, index, None, total]) == nbx.NBX_OK
            assert index[:t].tobytes() == got["index"].tobytes() and (index[t:] == -7).all() and (r2 == T(-7.25)).all()
            index[:] = -7
            assert _raw(nbx, c, "context", radius, t, [off, None, r2, total]) == nbx.NBX_OK
            assert r2[:t].tobytes() == got["r2"].tobytes() and (r2[t:] == T(-7.25)).all() and (index == -7).all()
            # two calls in a row return the same bytes, also after a call at another radius
            c.nlist(dense if radius == sparse else sparse)
            assert same(c.nlist(radius), got)


@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_have_the_bits_of_a_context_and_offsets_continue_across_them(nbx, precision):
    S, n = R.ENSEMBLE
    T = R.DTYPE[precision]
    states, radius = R.ensemble_states(precision)
    alone = [context_lists(nbx, (precision, "ensemble", m), st, radius, precision) for m, st in enumerate(states)]
    for m, st in enumerate(states):
        assert not R.differs(alone[m], ref((precision, "ensemble", m), st, radius, precision), precision), m
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        for first, count in ((0, 3), (1, 2), (2, 1)):
            got = typed(e.nlist(radius, first=first, count=count), count * n, precision)
            want = R.concat(alone[first:first + count])  # offsets continue across members, j is member-local
            assert same(got, want), (first, count)
            assert got["index"].max() < n
            per = nbx.nlist_pairs(got, n)
            assert len(per) == count and all(np.array_equal(p[0], nbx.nlist_pairs(a)[0]) for p, a in zip(per, alone[first:first + count]))
            # nothing is written behind the range's own bodies and entries
            t, bodies = want["total"], count * n
            off, total = np.full(bodies + 1 + 8, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
            index, r2 = np.full(t + 8, -7, dtype=np.int32), np.full(t + 8, -7.25, dtype=T)
            assert _raw(nbx, e, "ensemble", radius, t + 8, [off, index, r2, total], first, count) == nbx.NBX_OK
            assert np.array_equal(off[:bodies + 1], want["offsets"]) and (off[bodies + 1:] == -7).all() and total[0] == t
            assert index[:t].tobytes() == want["index"].tobytes() and (index[t:] == -7).all() and (r2[t:] == T(-7.25)).all()
        assert same(e.nlist(radius), R.concat(alone))
        empty = e.nlist(radius, first=S, count=0)
        assert empty["total"] == 0 and empty["offsets"].tolist() == [0] and empty["index"].size == 0


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    states, radius = R.ragged_states(precision)
    alone = [context_lists(nbx, (precision, "ragged", m), st, radius, precision) for m, st in enumerate(states)]
    for m, st in enumerate(states):
        assert not R.differs(alone[m], ref((precision, "ragged", m), st, radius, precision), precision), sizes[m]
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        full = typed(r.nlist(radius), sum(sizes), precision)
        assert same(full, R.concat(alone)) and same(r.nlist(radius), full)
        for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (0, 1), (1, 3), (5, 3), (S, 0), (3, 0)):
            got = r.nlist(radius, first=first, count=count)
            want = R.concat(alone[first:first + count]) if count else {"offsets": np.zeros(1, np.int64), "index": np.zeros(0, np.int32),
                                                                       "r2": np.zeros(0, R.DTYPE[precision]), "total": 0}
            assert same(got, want), (first, count)
        per = nbx.nlist_pairs(full, sizes)
        assert all(np.array_equal(p[0], nbx.nlist_pairs(a)[0]) and p[1].tobytes() == nbx.nlist_pairs(a)[1].tobytes() for p, a in zip(per, alone))
        assert same(r.nlist(radius), full)  # a partial call leaves nothing behind that a full one sees
    # the same systems in another order: other offsets, other rows -- the same bits
    with nbx.Ragged(sizes[::-1], precision) as r:
        r.upload(states[::-1])
        assert same(r.nlist(radius), R.concat(alone[::-1]))


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 4)] + [dict(j_split=s) for s in (1, 4, 32)])


@pytest.mark.parametrize("precision", [32, 64])
def test_a_sliced_context_and_every_context_option_return_the_whole_default_contexts_lists(nbx, precision):
    n = 2049
    _, st, radius = R.cases(precision, n)[1]
    want = context_lists(nbx, (precision, n, "r1"), st, radius, precision)
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # all n positions are resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as c:
            c.upload(st)
            assert same(typed(c.nlist(radius), n, precision), want), (i_begin, i_count)
    made = 0
    for o in CONTEXT_OPTIONS:
        opts = {k: getattr(nbx, v) if isinstance(v, str) else v for k, v in o.items()}
        try:
            c = nbx.Context(n, precision, **opts)
        except nbx.NbxError as e:
            assert e.code == nbx.NBX_ERR_ARG, (o, str(e))  # not a shape this precision has
            continue
        with c:
            c.upload(st)
            assert same(c.nlist(radius), want), o
            made += 1
    assert made >= 6


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_after_steps_the_lists_describe_the_stepped_state_and_the_call_leaves_the_trajectory_alone(nbx, kind):
    dt = 1.0 / 256
    sizes = (257, 2049, 513)
    radius = 0.2
    states = [K.make_state(90 + k, n, np.float32) for k, n in enumerate(sizes)]
    if kind == "ensemble":
        states = [K.make_state(90 + k, 513, np.float32) for k in range(3)]
    make = {"context": lambda: nbx.Context(2049, 32), "ensemble": lambda: nbx.Ensemble(513, 3, 32), "ragged": lambda: nbx.Ragged(sizes, 32)}[kind]
    up = states[1] if kind == "context" else states
    with make() as o:
        o.upload(up)
        before = o.nlist(radius)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        after = o.nlist(radius)
        moved = o.download()
        steps = o.stats()["steps_done"]
        ke = o.step(2, dt)
        end_a = o.download()
    assert steps == 3 and not same(before, after)
    flat = lambda d: [d] if isinstance(d, dict) else list(d)
    # download() returns positions and velocities: a dict for a context, a dict of (members, n) arrays for an ensemble, a list
    if kind == "ragged":
        fresh = [dict(m, mass=u["mass"]) for m, u in zip(moved, up)]
    else:
        fresh = dict(moved, mass=up["mass"] if kind == "context" else np.stack([u["mass"] for u in up]))
    with make() as o:  # the downloaded state, uploaded afresh: the same lists
        o.upload(fresh)
        assert same(o.nlist(radius), after)
    with make() as o:  # the same course without the calls: the same trajectory and energies
        o.upload(up)
        o.step(3, dt, kenergy=False)
        assert np.array_equal(o.step(2, dt), ke)
        end_b = o.download()
    assert all(np.array_equal(a[f], b[f]) for a, b in zip(flat(end_a), flat(end_b)) for f in K.FIELDS[:6])


def test_state_errors_and_the_order_of_the_checks_on_a_live_object(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    off, total = np.zeros(4096, dtype=np.int64), np.zeros(1, dtype=np.int64)
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.nlist(0.2)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_nlist: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        assert c.nlist(0.2)["offsets"].shape == (301,)
        assert _raw(nbx, c, "context", 0.2, 2 ** 28 + 1, [off, None, None, total]) == nbx.NBX_ERR_ARG
        assert _raw(nbx, c, "context", 0.2, 8, [off, None, None, total]) == nbx.NBX_ERR_ARG
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.nlist(0.2)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_nlist: a local step awaits nbx_commit" in str(err.value)
        assert _raw(nbx, c, "context", -1.0, 0, [off, None, None, total]) == nbx.NBX_ERR_ARG  # the radius comes before the state
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_nlist"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_nlist")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.nlist(0.2)
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            with pytest.raises(nbx.NbxError) as err:
                o.nlist(0.2, first=2, count=2)
            assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value)
            part = o.nlist(0.2, first=0, count=3)  # the uploaded members can be asked before the others arrive
            for first, count in ((-1, 1), (0, 5), (4, 1), (0, -1), (5, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.nlist(0.2, first=first, count=count)
                assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value), (first, count)
            o.upload(st[3:], first=3)
            assert same(o.nlist(0.2, first=0, count=3), part)


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_of_35937_gives_the_geometric_neighbour_sets_and_one_bit_pattern_per_distance_class(nbx, precision, perm):
    k = 33
    n = k ** 3
    T = R.DTYPE[precision]
    with nbx.Context(n, precision) as c:
        c.upload(L.state(k, precision, perm))
        for m in (1, 2):  # the face neighbours; the face and the edge neighbours
            radius = L.radius_of(m)
            want = R.lattice_lists(k, m, precision, perm)
            got = typed(c.nlist(radius), n, precision)
            assert got["total"] == want["total"] == 2 * L.pair_counts(k, [m])[0]
            assert np.array_equal(got["offsets"], want["offsets"]) and np.array_equal(got["index"], want["index"]), (precision, perm, m)
            assert got["r2"].tobytes() == want["r2"].astype(T).tobytes()  # the bits of the distance class
            assert len(np.unique(got["r2"])) == m
            if m == 1:
                relations(c, got, radius, n, precision, (precision, perm, m))


@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_of_531441_matches_the_closed_form_across_260_scan_blocks(nbx, precision):
    k = 81
    n = k ** 3
    assert -(-n // R.SCAN_BLOCK) == 260
    radius = L.radius_of(1)
    want = R.lattice_lists(k, 1, precision)
    with nbx.Context(n, precision) as c:
        c.upload(L.state(k, precision))
        got = typed(c.nlist(radius), n, precision)
    assert got["total"] == want["total"] == 2 * L.pair_counts(k, [1])[0] == 6 * k * k * (k - 1)
    assert np.array_equal(got["offsets"], want["offsets"])  # every offsets[b]
    assert np.array_equal(got["index"], want["index"]) and got["r2"].tobytes() == want["r2"].astype(R.DTYPE[precision]).tobytes()


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32, a radius with about 6 neighbours
    per body: one batch call against 16 nbx_nlist calls on contexts created and uploaded beforehand, in this process, rounds
    alternated (tools/nlist_cost.py).  The pair work of the two arms is the same and one call issues 7 launches and 2
    synchronisations where the contexts issue 112 and 32, so the gate has no further margin: ratio <= 1.0, the condition every
    batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nlist_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = nlist_cost.measure(nbx, kind)
        print("%s fp32 %.2f per body: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["neighbours_per_body"], r["batch_us"],
                                                                                         r["contexts_us"], r["ratio"]))
        cells[kind] = r
    for kind, r in cells.items():
        assert r["members"] == 16 and r["precision"] == 32 and r["same_bytes_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert 3.0 < r["neighbours_per_body"] < 9.0, r  # about 6
        assert r["ratio"] <= 1.0, r
