"""Friends-of-friends groups on the device (include/nbx_fof.h) against the fp64 numpy reference tests/fof_ref.py, as a context, as
members of an ensemble and as members of one ragged ensemble.

What is asked (fof_ref.differs): label, size, groups and largest EQUAL to the union-find of the reference, and passes EQUAL to
the number its restatement of the pass scheme makes.  Every (state, radius) compared that way is unambiguous -- no pair's r2
within 64 u of h2 -- which test_fof_cpu.py shows for every one of them with the reference alone (fof_ref.reference_cases); the
radii come from fof_ref.pick_radius.  The statements that hold one device result against another need no such argument: the
same r2 bits are compared on both sides.

Shapes, the smallest at which each part can go wrong: n = 1 and 2; 257 (one split, two tiles, the last holding one body and 255
padding records); 513 (two columns); 1025 (one split of 5 tiles, three columns); 2049 (five columns, two splits of 5 and 4
tiles); 4097 (nine columns, four splits, the last one short); the chain of 4097, whose links cross every column and split seam;
ragged members of 5 and 8192 bodies side by side (one column and one split next to 16 columns and 8 splits: the neutral rows);
lattice(33) = 35937 bodies (71 columns x 15 splits)."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

import fof_ref as R
import kick_ref as K
from conftest import ROOT

pytestmark = pytest.mark.gpu

_refs, _ctx = {}, {}


def ref(key, st, radius, precision, close=None, pairs=None):
    """The reference's result and the restatement's passes for a case, computed once and left unchanged."""
    if key not in _refs:
        want = R.fof(st, radius, precision, pairs=pairs, close=close)
        again = R.restate(st, radius, precision, pairs=pairs, close=close)
        assert not R.differs(again, want, passes=False), key
        want["passes"] = again["passes"]
        for a in (want["label"], want["size"]):
            a.setflags(write=False)
        _refs[key] = want
    return _refs[key]


def same(a, b, passes=True):
    return not R.differs(a, b, passes=passes)


def typed(got, n):
    assert got["label"].dtype == np.int32 and got["size"].dtype == np.int32 and got["label"].shape == got["size"].shape == (n,)
    return got


def context_fof(nbx, key, st, radius, precision):
    """What a default context holding the state returns, asked once per case: the bits the members are held to."""
    if key not in _ctx:
        n = len(st["mass"])
        with nbx.Context(n, precision) as c:
            c.upload(st)
            got = typed(c.fof(radius), n)
            assert same(c.fof(radius), got), key  # two calls in a row: the same values, the same passes
        _ctx[key] = got
    return _ctx[key]


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference_and_the_restatements_passes_at_three_radii(nbx, precision, family, n):
    st, close, radii = R.sized(precision, family, n)
    for q, radius in enumerate(radii):
        key = (precision, family, n, q)
        assert not R.ambiguous(st, radius, precision, close), key
        want = ref(key, st, radius, precision, close=close)
        got = context_fof(nbx, key, st, radius, precision)
        print("fp%d %s(%d) r = %.5f: %d groups, largest %d, %d passes (restatement %d)" % (precision, family, n, radius, got["groups"], got["largest"],
                                                                                          got["passes"], want["passes"]))
        found = R.differs(got, want)
        assert not found, (key, found)
    if n == 1:
        one = context_fof(nbx, (precision, family, 1, 0), st, radii[0], precision)
        assert (one["label"].tolist(), one["size"].tolist(), one["groups"], one["largest"], one["passes"]) == ([0], [1], 1, 1, 1)


@pytest.mark.parametrize("order", R.CHAIN_ORDERS)
@pytest.mark.parametrize("precision", [32, 64])
def test_chains_are_one_group_in_the_restatements_passes_and_two_groups_with_one_link_cut(nbx, precision, order):
    n = R.CHAIN_N
    st = R.chain(n, precision, order)
    want = ref((precision, "chain", order), st, R.CHAIN_RADIUS, precision)
    got = context_fof(nbx, (precision, "chain", order), st, R.CHAIN_RADIUS, precision)
    print("fp%d chain(%d) %s: %d passes (restatement %d)" % (precision, n, order, got["passes"], want["passes"]))
    assert (got["groups"], got["largest"]) == (1, n) and (got["label"] == 0).all() and (got["size"] == n).all()
    assert not R.differs(got, want)
    assert want["passes"] == {"random": 9, "ascending": 2, "descending": 2, "zigzag": 3}[order]  # what the simulation of the scheme gives
    cut = n // 3
    st = R.chain(n, precision, order, cut=cut)
    want = ref((precision, "chain cut", order), st, R.CHAIN_RADIUS, precision)
    got = context_fof(nbx, (precision, "chain cut", order), st, R.CHAIN_RADIUS, precision)
    assert (got["groups"], got["largest"]) == (2, n - cut) and sorted(set(got["size"].tolist())) == [cut, n - cut]
    assert not R.differs(got, want)


@pytest.mark.parametrize("family", ["cloud", "clustered"])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_labels_agree_with_neighbours_and_knn_on_the_same_r2_bits(nbx, precision, family):
    """Exact device-to-device statements: no reference, no ambiguity argument."""
    for n in (257, 4097):
        st, _, radii = R.sized(precision, family, n)
        with nbx.Context(n, precision) as c:
            c.upload(st)
            knn = c.knn(16)
            for radius in radii + (0.0, 0.01):
                got = c.fof(radius)
                nb = c.neighbours(radius)
                label = got["label"]
                near = nb["within"] > 0  # the device's own r2[i] <= h2: the nearest partner is within the radius iff any is
                assert (label[near] == label[nb["index"][near]]).all(), (n, radius)
                assert (got["size"] >= nb["within"] + 1).all(), (n, radius)
                # nbx_knn.h: #(r2[i, :] <= h2) == min(within[i], k) and a row ascends -- the partners within the radius are its first ones
                friends = np.arange(16)[None, :] < np.minimum(nb["within"], 16)[:, None]
                assert (np.where(friends, label[np.clip(knn["index"], 0, None)], label[:, None]) == label[:, None]).all(), (n, radius)
                assert (got["groups"] == n) == (nb["within"] == 0).all(), (n, radius)
                # the partition is consistent in itself
                assert (label <= np.arange(n)).all() and (label[label] == label).all()
                counts = np.bincount(label, minlength=n)
                assert np.array_equal(got["size"], counts[label]) and got["groups"] == (label == np.arange(n)).sum() and got["largest"] == counts.max()


@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_at_the_tie_radius_is_one_group(nbx, precision):
    """h2 at radius 1/8 is bit for bit the r2 of a face neighbour, in both precisions: <= makes the lattice one group, < would
    leave 2197.  The device's own r2 says so first."""
    k = R.N.LATTICE_K
    n = k ** 3
    for perm in (False, True):
        with nbx.Context(n, precision) as c:
            c.upload(R.lattice(k, precision, perm))
            nb = c.neighbours(R.LATTICE_TIE)
            got = c.fof(R.LATTICE_TIE)
        exp_index, exp_within = R.N.lattice_expected(k, perm)
        assert np.array_equal(nb["within"], exp_within) and (nb["r2"] == nb["r2"][0]).all()
        assert (got["groups"], got["largest"]) == (1, n) and (got["label"] == 0).all()
        assert got["passes"] == R.restate(R.lattice(k, precision, perm), R.LATTICE_TIE, precision, pairs=R.lattice_pairs(k, perm))["passes"]


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 4)] +
    [dict(kernel_variant="KERNEL_SGPRW", bodies_per_lane=2), dict(kernel_variant="KERNEL_JLANE", bodies_per_lane=4)] +
    [dict(j_split=s) for s in (1, 4, 32)] + [dict(kernel_variant="KERNEL_LDS", j_split=4)])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_values_do_not_depend_on_the_contexts_options_and_a_sliced_context_returns_the_whole_ones(nbx, precision):
    n = 2049
    s, close, radii = R.sized(precision, "cloud", n)
    want = {q: context_fof(nbx, (precision, "cloud", n, q), s, radii[q], precision) for q in (1, 2)}
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
            for q in (1, 2):
                assert same(c.fof(radii[q]), want[q]), (o, q, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    assert {m[0] for m in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR} and {m[1] for m in made} == {nbx.ORDER_TREE, nbx.ORDER_REFERENCE}
    assert len(set(made)) >= 6
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # all n positions are resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as c:
            c.upload(s)
            for q in (1, 2):
                got = c.fof(radii[q])
                assert got["label"].shape == (n,) and same(got, want[q]), (i_begin, i_count, q)


def _member(res, m):
    return {k: res[k][m] for k in R.KEYS} if isinstance(res, dict) else res[m]


@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_reference_and_a_context_over_the_whole_range_and_over_sub_ranges(nbx, precision):
    n, S = R.ENSEMBLE_N, R.ENSEMBLE_MEMBERS
    states, radius = R.ensemble_states(precision)
    wants = [ref((precision, "ensemble", m), st, radius, precision) for m, st in enumerate(states)]
    lone = [context_fof(nbx, (precision, "ensemble", m), st, radius, precision) for m, st in enumerate(states)]
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        full = e.fof(radius)
        assert full["label"].shape == full["size"].shape == (S, n) and full["groups"].shape == full["largest"].shape == (S,)
        assert full["label"].dtype == full["size"].dtype == full["groups"].dtype == np.int32
        again = e.fof(radius)
        assert all(same(_member(again, m), _member(full, m), passes=False) for m in range(S)) and again["passes"] == full["passes"]
        for m in range(S):
            assert not R.differs(_member(full, m), wants[m], passes=False), (precision, m)
            assert same(_member(full, m), lone[m], passes=False), (precision, m)
        # every pass serves the whole range: the call makes as many as its slowest member
        assert full["passes"] == max(w["passes"] for w in wants) == max(c["passes"] for c in lone)
        assert len({w["passes"] for w in wants}) > 1  # and the members do differ
        for first, count in ((1, 2), (0, 1), (2, 4), (S - 1, 1), (S, 0), (0, 0)):
            part = e.fof(radius, first, count)
            assert part["label"].shape == (count, n) and part["groups"].shape == (count,)
            for key in R.KEYS:
                assert np.array_equal(part[key], full[key][first:first + count]), (first, count, key)
            assert part["passes"] == (max(w["passes"] for w in wants[first:first + count]) if count else 0), (first, count)
        assert np.array_equal(e.fof(radius, first=3)["label"], full["label"][3:])


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_a_context_of_their_size(nbx, precision):
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    states, radius = R.ragged_states(precision)
    wants = [ref((precision, "ragged", m), st, radius, precision) for m, st in enumerate(states)]
    lone = [context_fof(nbx, (precision, "ragged", m), st, radius, precision) for m, st in enumerate(states)]
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        full = r.fof(radius)
        assert len(full) == S and all(typed(full[m], sizes[m]) for m in range(S))
        for m in range(S):
            assert not R.differs(full[m], wants[m], passes=False), (precision, m, sizes[m])
            assert same(full[m], lone[m], passes=False), (precision, m)
            assert full[m]["passes"] == max(w["passes"] for w in wants)
        for first, count in ((0, 2), (1, 1), (0, 1), (2, 3), (3, 2), (S - 1, 1), (S, 0), (3, 0)):
            part = r.fof(radius, first, count)
            assert len(part) == count and all(same(a, b, passes=False) for a, b in zip(part, full[first:first + count])), (first, count)
            assert all(p["passes"] == max(w["passes"] for w in wants[first:first + count]) for p in part), (first, count)
        assert all(same(a, b) for a, b in zip(r.fof(radius), full))  # a partial call leaves nothing behind that a full one sees
        # the layout is end to end, member `first` at element 0, and nothing is written behind the last member
        first, count = 1, 3
        total = sum(sizes[first:first + count])
        flat = [np.full(total + 8, -7, dtype=np.int32), np.full(total + 8, -7, dtype=np.int32), np.full(2 * count + 8, -7, dtype=np.int32),
                np.full(9, -7, dtype=np.int32)]
        assert nbx.load().nbx_ragged_fof(r._h, first, count, radius, *[a.ctypes.data_as(ctypes.c_void_p) for a in flat]) == nbx.NBX_OK
        for a, key in zip(flat, ("label", "size")):
            assert np.array_equal(a[:total], np.concatenate([full[m][key] for m in range(first, first + count)])), key
            assert (a[total:] == -7).all(), key
        assert flat[2][:2 * count].tolist() == [v for m in range(first, first + count) for v in (full[m]["groups"], full[m]["largest"])]
        assert (flat[2][2 * count:] == -7).all() and (flat[3][1:] == -7).all() and flat[3][0] == max(w["passes"] for w in wants[first:first + count])
    # the same systems in another order: other offsets, other rows -- the same values
    with nbx.Ragged(sizes[::-1], precision) as r:
        r.upload(states[::-1])
        assert all(same(a, b) for a, b in zip(r.fof(radius), full[::-1]))


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_large_lattice_has_the_closed_forms_and_the_restatements_passes(nbx, precision, perm):
    k = 33
    n = k ** 3
    st = R.lattice(k, precision, perm)
    pairs = R.lattice_pairs(k, perm)
    assert not R.lattice_ambiguous(k, R.LATTICE_BELOW, precision) and not R.lattice_ambiguous(k, R.LATTICE_ABOVE, precision)
    with nbx.Context(n, precision) as c:
        c.upload(st)
        below, above = c.fof(R.LATTICE_BELOW), c.fof(R.LATTICE_ABOVE)
    assert (below["groups"], below["largest"], below["passes"]) == (n, 1, 1)
    assert np.array_equal(below["label"], np.arange(n)) and (below["size"] == 1).all()
    want = R.restate(st, R.LATTICE_ABOVE, precision, pairs=pairs)
    print("fp%d lattice(33) perm=%d: %d passes (restatement %d)" % (precision, perm, above["passes"], want["passes"]))
    assert (above["groups"], above["largest"]) == (1, n) and (above["label"] == 0).all() and (above["size"] == n).all()
    assert above["passes"] == want["passes"] == (5 if perm else 2)


def _raw(nbx, o, kind, radius, arrays, first=0, count=None):
    L = nbx.load()
    ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    if kind == "context":
        return L.nbx_fof(o._h, radius, *ptr)
    f = L.nbx_ensemble_fof if kind == "ensemble" else L.nbx_ragged_fof
    return f(o._h, first, o.members if count is None else count, radius, *ptr)


def _make(nbx, kind, precision=32):
    """An object of the kind with its states, the bodies and the systems a call over all of it returns."""
    sizes = (257, 2049, 513)
    if kind == "context":
        return nbx.Context(2049, precision), R.cloud(2049, precision), 2049, 1
    if kind == "ensemble":
        return nbx.Ensemble(2049, 3, precision), [R.cloud(2049, precision), R.clustered(2049, precision), R.N.reversed_box(2049, precision)], 3 * 2049, 3
    return nbx.Ragged(sizes, precision), [R.cloud(n, precision) for n in sizes], sum(sizes), 3


def _flatten(res):
    """label, size, {groups, largest} interleaved, passes -- the four arrays of the C call."""
    rows = [res] if isinstance(res, dict) else res
    info = np.stack([np.concatenate([np.atleast_1d(r["groups"]) for r in rows]), np.concatenate([np.atleast_1d(r["largest"]) for r in rows])], axis=1)
    return [np.concatenate([np.asarray(r["label"]).reshape(-1) for r in rows]), np.concatenate([np.asarray(r["size"]).reshape(-1) for r in rows]),
            info.reshape(-1).astype(np.int32), np.array([rows[0]["passes"]], dtype=np.int32)]


RADIUS = 0.1  # of the tests that compare device results with each other


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_null_output_is_skipped_alone_and_the_radius_is_checked_even_when_nothing_is_asked_for(nbx, precision, kind):
    o, states, total, systems = _make(nbx, kind, precision)
    with o:
        o.upload(states)
        full = _flatten(o.fof(RADIUS))
        for skip in range(4):
            arrays = [np.full(total, -7, dtype=np.int32), np.full(total, -7, dtype=np.int32), np.full(2 * systems, -7, dtype=np.int32),
                      np.full(1, -7, dtype=np.int32)]
            keep = list(arrays)
            arrays[skip] = None
            assert _raw(nbx, o, kind, RADIUS, arrays) == nbx.NBX_OK
            for q, a in enumerate(keep):
                if q == skip:
                    assert (a == -7).all()  # never written
                else:
                    assert np.array_equal(a, full[q]), (skip, q)
        passes = np.full(1, -7, dtype=np.int32)
        assert _raw(nbx, o, kind, RADIUS, [None, None, None, passes]) == nbx.NBX_OK and passes[0] == -7  # nothing launched, nothing written
        only = np.full(2 * systems, -7, dtype=np.int32)
        assert _raw(nbx, o, kind, RADIUS, [None, None, only, None]) == nbx.NBX_OK and np.array_equal(only, full[2])  # info alone is a call
        for bad in (-1.0, float("nan")):
            assert _raw(nbx, o, kind, bad, [None] * 4) == nbx.NBX_ERR_ARG and b"radius is NaN or negative" in nbx.load().nbx_last_error()
            with pytest.raises(nbx.NbxError) as err:
                o.fof(bad)
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
    dt = 1.0 / 4
    o, states, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        before_steps = _flatten(o.fof(RADIUS))
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        k3 = _flatten(o.fof(RADIUS))
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        again = _flatten(o.fof(RADIUS))
        _flatten(o.fof(2 * RADIUS))
        after = o.stats()
        assert {k: before[k] for k in UNTOUCHED if k in before} == {k: after[k] for k in UNTOUCHED if k in after} and before["steps_done"] == 3
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        diag_a = _diag_values(o)
        nb_a = o.neighbours(RADIUS)
        ke_a = o.step(3, dt)
        a = _positions(o.download())
    assert all(np.array_equal(x, y) for x, y in zip(k3, again))
    o, _, _, _ = _make(nbx, kind)
    with o:  # the same course without the call
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)
        o.sync()
        diag_b = _diag_values(o)
        nb_b = o.neighbours(RADIUS)
        ke_b = o.step(3, dt)
        b = _positions(o.download())
        down = o.download()
        f6 = _flatten(o.fof(RADIUS))
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)  # the bits of later steps are as without the call
    assert diag_a == diag_b
    for x, y in zip(nb_a if isinstance(nb_a, list) else [nb_a], nb_b if isinstance(nb_b, list) else [nb_b]):
        assert all(np.array_equal(x[k], y[k]) for k in x)
    assert not np.array_equal(f6[0], before_steps[0]) and not np.array_equal(k3[0], before_steps[0])  # the call does follow the state
    # after the steps the call describes the state after them: a context that is given the downloaded state says the same
    sts = down if isinstance(down, list) else ([down] if kind == "context" else [{f: down[f][m] for f in down} for m in range(3)])
    at = 0
    for m, d in enumerate(sts):
        n = len(d["pos_x"])
        with nbx.Context(n, 32) as c:
            c.upload(dict(d, mass=np.ones(n, dtype=np.float32)))
            lone = c.fof(RADIUS)
        assert np.array_equal(lone["label"], f6[0][at:at + n]) and np.array_equal(lone["size"], f6[1][at:at + n]), (kind, m)
        at += n


def test_state_errors(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.fof(RADIUS)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_fof: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        assert c.fof(RADIUS)["label"].shape == (300,)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.fof(RADIUS)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_fof: a local step awaits nbx_commit" in str(err.value)
        assert _raw(nbx, c, "context", RADIUS, [None] * 4) == nbx.NBX_ERR_STATE  # the state comes before "nothing to do"
        assert _raw(nbx, c, "context", -1.0, [None] * 4) == nbx.NBX_ERR_ARG  # and the radius before the state
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_fof"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_fof")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.fof(RADIUS)
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.fof(RADIUS, first, count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value), (first, count)
            part = _flatten(o.fof(RADIUS, 0, 3))  # the uploaded members can be asked before the others arrive
            assert part[0].shape == (sum(len(s["mass"]) for s in st[:3]),)
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.fof(RADIUS, first, count)
                assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value), (first, count)
            with pytest.raises(nbx.NbxError) as err:
                o.fof(-1.0, 0, S + 1)
            assert "radius is NaN or negative" in str(err.value)  # the radius comes before the range
            o.upload(st[3:], first=3)
            assert all(np.array_equal(x, y) for x, y in zip(_flatten(o.fof(RADIUS, 0, 3)), part))


def test_more_than_2_to_the_22_bodies_are_refused(nbx):
    n = (1 << 22) + 1
    with nbx.Context(n, 32) as c:
        c.upload(K.make_state(77, n, np.float32))
        with pytest.raises(nbx.NbxError) as err:
            c.fof(RADIUS)
        assert err.value.code == nbx.NBX_ERR_ARG and "nbx_fof: n exceeds 4194304" in str(err.value)
        assert nbx.load().nbx_fof(c._h, RADIUS, None, None, None, None) == nbx.NBX_ERR_ARG  # also when nothing is asked for
    with nbx.Ensemble(1 << 12, (1 << 10) + 1, 32) as e:  # nothing uploaded: the size comes before the state
        with pytest.raises(nbx.NbxError) as err:
            e.fof(RADIUS)
        assert err.value.code == nbx.NBX_ERR_ARG and "nbx_ensemble_fof: count * n exceeds 4194304" in str(err.value)
        with pytest.raises(nbx.NbxError) as err:
            e.fof(RADIUS, 0, 1 << 10)
        assert err.value.code == nbx.NBX_ERR_STATE  # a range within the bound reaches the state check


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32, one radius (pick_radius at the
    median nearest-neighbour distance): one batch call against 16 nbx_fof calls on contexts created and uploaded beforehand, in
    this process, rounds alternated (tools/fof_cost.py).  The batch call makes as many passes as its slowest member, each one
    launch of each kind and one read-back for all 16, where the contexts make the sum of theirs: ratio <= 1.0, the condition
    every batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fof_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = fof_cost.measure(nbx, kind)
        print("%s fp32 r = %.4f: batch %.1f us (%d passes), 16 contexts %.1f us (passes %r), ratio %.3f"
              % (kind, r["radius"], r["batch_us"], r["batch_passes"], r["contexts_us"], r["context_passes"], r["ratio"]))
        cells[kind] = r
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_values_from_both_arms"] and r["batch_passes"] == max(r["context_passes"]), kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
