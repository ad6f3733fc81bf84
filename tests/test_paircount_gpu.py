"""Pairs within each of a list of radii on the device (include/nbx_paircount.h) against the fp64 numpy reference
tests/paircount_ref.py, as a context, as members of an ensemble and as members of one ragged ensemble.

What is asked: lo <= got <= hi of paircount_ref.bracket at every radius -- the 8 u window of neighbours_ref on r2 against h2, u
the unit round-off of the object's precision -- which is exact equality in fp64 and, in fp32, wherever hi == lo;
test_paircount_cpu.py shows with the reference alone how narrow the bracket is (hi - lo <= 8 everywhere, exact at 8 or more of
the 20 radii).  Without any tolerance: counts[k] is half the sum of nbx_neighbours' within at the same radius; the lattice
counts follow from integer geometry; members, context options, slices and the two counting schemes give the same bits.

Shapes, the smallest at which each part can go wrong: n = 257 (one split, two tiles, the last holding one body and 255 padding
records), n = 2049 (five columns, two splits), n = 4097 (nine columns, four splits, the last one short), lattice(13) = 2197
bodies (two splits meeting at j = 1280), n = 1 and n = 2.  Twenty radii make two passes, E = 16 then E = 4."""
import ctypes
import json
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import kick_ref as K
import paircount_ref as P
from conftest import ROOT, PKG

pytestmark = pytest.mark.gpu

FAMILIES = {"box": P.box, "shifted": P.shifted, "reversed": P.reversed_box, "member": P.member}
_states, _refs, _ctx = {}, {}, {}


def state(precision, family, n):
    key = (precision, family, n)
    if key not in _states:
        _states[key] = P.lattice(P.LATTICE_K, precision) if family == "lattice" else FAMILIES[family](n, precision)
    return _states[key]


def ref(precision, family, n):
    """(plain counts, lo, hi) at RADII, computed once per state and left unchanged."""
    key = (precision, family, n)
    if key not in _refs:
        st = state(precision, family, n)
        r2 = P.pair_r2(st)
        out = (P.counts(st, P.RADII, precision, r2),) + P.bracket(st, P.RADII, precision, r2)
        for a in out:
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def context_values(nbx, precision, family, n):
    """What a default context of n bodies holding the state returns at RADII, asked once per state: the bits the members are held to."""
    key = (precision, family, n)
    if key not in _ctx:
        with nbx.Context(n, precision) as c:
            c.upload(state(precision, family, n))
            got = c.paircount(P.RADII)
            assert np.array_equal(c.paircount(P.RADII), got)  # two calls in a row: the same bits
        got.setflags(write=False)
        _ctx[key] = got
    return _ctx[key]


def check(got, precision, family, n):
    plain, lo, hi = ref(precision, family, n)
    assert got.dtype == np.uint64 and got.shape == (len(P.RADII),)
    diff = got.astype(np.int64) - plain.astype(np.int64)
    print("fp%d %s(%d): got - plain count %s; bracket widths %s" % (precision, family, n, diff.tolist(), (hi - lo).tolist()))
    assert (lo <= got).all() and (got <= hi).all(), (precision, family, n, np.nonzero((got < lo) | (got > hi))[0].tolist())
    assert (np.diff(got.astype(np.int64)) >= 0).all()  # monotone in the radius


@pytest.mark.parametrize("n", P.SIZES)
@pytest.mark.parametrize("family", ["box", "shifted"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference(nbx, precision, family, n):
    check(context_values(nbx, precision, family, n), precision, family, n)


@pytest.mark.parametrize("precision", [32, 64])
def test_counts_are_half_the_sum_of_the_neighbours_within_at_the_same_radius(nbx, precision):
    n = 2049
    got = context_values(nbx, precision, "box", n)
    with nbx.Context(n, precision) as c:
        c.upload(state(precision, "box", n))
        for k in (0, 7, 15, 16, 19):  # slots of both passes
            total = int(c.neighbours(P.RADII[k])["within"].sum(dtype=np.int64))
            assert total % 2 == 0 and int(got[k]) == total // 2, (k, int(got[k]), total)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_counts_are_the_geometrys_and_the_tie_counts(nbx, precision):
    k = P.LATTICE_K
    with nbx.Context(k ** 3, precision) as c:
        c.upload(state(precision, "lattice", k ** 3))
        assert np.array_equal(c.paircount(P.LATTICE_RADII), P.lattice_counts(k, 6))
        # h2 is bit for bit the face neighbours' r2: <= counts them
        assert P.DTYPE[precision](P.h2_of(P.LATTICE_TIE_RADIUS, precision)) == c.neighbours(P.LATTICE_TIE_RADIUS)["r2"][0]
        assert c.paircount([P.LATTICE_TIE_RADIUS]).tolist() == [P.lattice_face_pairs(k)]
        assert c.paircount([0.0, math.inf]).tolist() == [0, k ** 3 * (k ** 3 - 1) // 2]


@pytest.mark.parametrize("precision", [32, 64])
def test_edge_radii_radius_sets_and_the_smallest_systems(nbx, precision):
    for family, n in (("member", 1), ("member", 2), ("shifted", 257), ("box", 2049)):
        full = context_values(nbx, precision, family, n)
        with nbx.Context(n, precision) as c:
            c.upload(state(precision, family, n))
            # +infinity: every pair, and neither the body itself nor a padding record; 0: the coincident pairs, none here
            assert c.paircount([math.inf]).tolist() == [n * (n - 1) // 2], (family, n)
            assert c.paircount([0.0]).tolist() == [0]
            assert c.paircount([math.inf, 0.0, math.inf, P.RADII[5], math.inf]).tolist() == [n * (n - 1) // 2, 0, n * (n - 1) // 2, int(full[5]), n * (n - 1) // 2]
            if n == 1:
                assert not full.any()
                continue
            order = [7, 0, 19, 7, 3, 16, 16, 12, 1, 18, 4, 4, 9, 0, 2, 15, 17, 11]  # unsorted, repeated, across the seam
            assert np.array_equal(c.paircount([P.RADII[k] for k in order]), full[order]), (family, n)
            for k in (1, 4, 5, 16, 17, 20):  # every E and the pass seam: prefixes of the same values
                assert np.array_equal(c.paircount(P.RADII[:k]), full[:k]), (family, n, k)
            assert np.array_equal(c.paircount(P.RADII * 12 + P.RADII[:16]), np.concatenate([full] * 12 + [full[:16]]))  # 256 radii: 16 passes
            assert np.array_equal(nbx.shell_counts(full).cumsum(dtype=np.uint64), full)
    two = context_values(nbx, precision, "member", 2)
    assert set(two.tolist()) <= {0, 1} and (np.diff(two.astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_reference_and_have_the_bits_of_a_context(nbx, precision, n):
    families = ("box", "shifted", "reversed")
    S, B = len(families), len(P.RADII)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload([state(precision, f, n) for f in families])
        full = e.paircount(P.RADII)
        assert full.shape == (S, B) and full.dtype == np.uint64 and np.array_equal(e.paircount(P.RADII), full)
        for m, f in enumerate(families):
            check(full[m], precision, f, n)
            assert np.array_equal(full[m], context_values(nbx, precision, f, n)), (precision, n, f)
        assert np.array_equal(full[0], full[2])  # the same geometry in reverse order
        for first, count in ((1, 2), (0, 1), (1, 1), (2, 1), (0, 2), (S, 0), (0, 0)):
            part = e.paircount(P.RADII, first, count)
            assert part.shape == (count, B) and np.array_equal(part, full[first:first + count]), (first, count)
        assert np.array_equal(e.paircount(P.RADII, first=1), full[1:]) and np.array_equal(e.paircount(P.RADII[:5], 1, 2), full[1:3, :5])
        # member-major, member `first` at element 0, and nothing is written behind the last element
        flat = np.full(2 * B + 8, 7, dtype=np.uint64)
        radii = np.array(P.RADII, dtype=np.float64)
        assert nbx.load().nbx_ensemble_paircount(e._h, 1, 2, B, radii.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p)) == nbx.NBX_OK
        assert np.array_equal(flat[:2 * B].reshape(2, B), full[1:3]) and (flat[2 * B:] == 7).all()
        assert np.array_equal(e.paircount(P.RADII), full)


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = P.RAGGED_SIZES
    S, B = len(sizes), len(P.RADII)
    with nbx.Ragged(sizes, precision) as r:
        r.upload([state(precision, "member", n) for n in sizes])
        full = r.paircount(P.RADII)
        assert full.shape == (S, B) and full.dtype == np.uint64 and np.array_equal(r.paircount(P.RADII), full)
        for m, n in enumerate(sizes):
            check(full[m], precision, "member", n)
            assert np.array_equal(full[m], context_values(nbx, precision, "member", n)), (precision, n)
        for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (0, 1), (1, 3), (5, 3), (S, 0), (3, 0)):
            part = r.paircount(P.RADII, first, count)
            assert part.shape == (count, B) and np.array_equal(part, full[first:first + count]), (first, count)
        assert np.array_equal(r.paircount(P.RADII, first=5), full[5:]) and np.array_equal(r.paircount(P.RADII[:17], 2, 4), full[2:6, :17])
        assert np.array_equal(r.paircount(P.RADII), full)  # a partial call leaves nothing behind that a full one sees
        first, count = 2, 4
        flat = np.full(count * B + 8, 7, dtype=np.uint64)
        radii = np.array(P.RADII, dtype=np.float64)
        assert nbx.load().nbx_ragged_paircount(r._h, first, count, B, radii.ctypes.data_as(ctypes.c_void_p), flat.ctypes.data_as(ctypes.c_void_p)) == nbx.NBX_OK
        assert np.array_equal(flat[:count * B].reshape(count, B), full[first:first + count]) and (flat[count * B:] == 7).all()
    # the same systems in another order: other offsets, other rows -- the same bits
    with nbx.Ragged(sizes[::-1], precision) as r:
        r.upload([state(precision, "member", n) for n in sizes][::-1])
        assert np.array_equal(r.paircount(P.RADII), full[::-1])


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
            assert np.array_equal(c.paircount(P.RADII), want), (o, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    assert len(set(made)) >= 6
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # all n positions are resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as c:
            c.upload(s)
            assert np.array_equal(c.paircount(P.RADII), want), (i_begin, i_count)


CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import nbx, paircount_ref as P
out = {}
for precision in (32, 64):
    with nbx.Context(2049, precision) as c:
        c.upload(P.box(2049, precision))
        out["context %%d" %% precision] = c.paircount(P.RADII).tolist()
    with nbx.Ragged((257, 1, 513), precision) as r:
        r.upload([P.member(n, precision) for n in (257, 1, 513)])
        out["ragged %%d" %% precision] = r.paircount(P.RADII[:5]).tolist()
    with nbx.Ensemble(257, 2, precision) as e:
        e.upload([P.box(257, precision), P.shifted(257, precision)])
        out["ensemble %%d" %% precision] = e.paircount(P.RADII[:9]).tolist()
print(json.dumps(out))
""" % (PKG, os.path.join(ROOT, "tests"))


def test_the_lane_counters_and_the_wave_counters_give_equal_arrays(nbx):
    """NBX_PAIRCOUNT_SCHEME=lane and =wave, each in a fresh child process: every E, three kinds, both precisions."""
    got = {}
    for scheme in ("lane", "wave"):
        env = dict(os.environ, NBX_PAIRCOUNT_SCHEME=scheme)
        res = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, (scheme, res.stderr[-2000:])
        got[scheme] = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["lane"] == got["wave"] and len(got["lane"]) == 6
    for precision in (32, 64):
        assert got["lane"]["context %d" % precision] == context_values(nbx, precision, "box", 2049).tolist()


def _make(nbx, kind, precision=32):
    sizes = (257, 2049, 513)
    if kind == "context":
        return nbx.Context(2049, precision), state(precision, "box", 2049)
    if kind == "ensemble":
        return nbx.Ensemble(2049, 3, precision), [state(precision, f, 2049) for f in ("box", "shifted", "reversed")]
    return nbx.Ragged(sizes, precision), [state(precision, "member", n) for n in sizes]


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
    radii = P.RADII[:17]
    o, states = _make(nbx, kind)
    with o:
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        n3 = o.paircount(radii)
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        again = o.paircount(radii)
        after = o.stats()
        assert {k: before[k] for k in UNTOUCHED if k in before} == {k: after[k] for k in UNTOUCHED if k in after} and before["steps_done"] == 3
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        ke_a = o.step(3, dt)
        a = _positions(o.download())
    assert np.array_equal(n3, again)
    o, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.step(3, dt)  # synchronises
        o.sync()
        assert np.array_equal(o.paircount(radii), n3)
    o, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        n0 = o.paircount(radii)
        ke_b = o.step(6, dt)
        b = _positions(o.download())
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)  # the bits of later steps are as without the call
    assert not np.array_equal(n0, n3)


def test_state_and_argument_errors_in_the_headers_order(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.paircount(P.RADII)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_paircount: nbx_upload has not been called" in str(err.value)
        for radii, text in (([], "nradii is outside [1, 256] or radii is NULL"), ([0.1] * 257, "nradii is outside [1, 256] or radii is NULL"),
                            ([0.1, -0.5, math.nan], "radii[1] is NaN or negative"), ([0.1, 0.2, math.nan], "radii[2] is NaN or negative")):
            with pytest.raises(nbx.NbxError) as err:
                c.paircount(radii)
            assert err.value.code == nbx.NBX_ERR_ARG and "nbx_paircount: " + text in str(err.value)  # the arguments come before the state
        c.upload(states[0])
        assert c.paircount(P.RADII).shape == (20,) and c.paircount(0.25).shape == (1,)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.paircount(P.RADII)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_paircount: a local step awaits nbx_commit" in str(err.value)
        r = np.array(P.RADII)
        assert nbx.load().nbx_paircount(c._h, 20, r.ctypes.data_as(ctypes.c_void_p), None) == nbx.NBX_ERR_STATE  # the state comes before "nothing to do"
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_paircount"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_paircount")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.paircount(P.RADII)
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.paircount(P.RADII, first, count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value), (first, count)
            part = o.paircount(P.RADII, 0, 3)  # the uploaded members can be asked before the others arrive
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.paircount(P.RADII, first, count)
                assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value), (first, count)
            with pytest.raises(nbx.NbxError) as err:
                o.paircount([0.1, -1.0], 0, S + 1)
            assert "radii[1] is NaN or negative" in str(err.value)  # the radii come before the range
            with pytest.raises(nbx.NbxError) as err:
                o.paircount([], 0, S + 1)
            assert "nradii is outside [1, 256] or radii is NULL" in str(err.value)
            o.upload(st[3:], first=3)
            assert np.array_equal(o.paircount(P.RADII, 0, 3), part)
            r = np.array(P.RADII)
            assert getattr(nbx.load(), name)(o._h, 0, S, 20, r.ctypes.data_as(ctypes.c_void_p), None) == nbx.NBX_OK  # counts NULL: nothing to do


def test_one_call_costs_no_more_than_the_routes_it_replaces(nbx):
    """fp32, 16 radii, in this process, rounds alternated (tools/paircount_cost.py).  context: one nbx_paircount call on 8192
    bodies against 16 nbx_neighbours calls (index and r2 NULL) on the same context plus the host sums -- that arm walks the same
    pairs 16 times with 16 synchronisations, so equality is the condition and no margin is added.  ensemble (16 x 2048) and
    ragged (16 sizes over 512 ... 4096): one batch call against 16 nbx_paircount calls on contexts created and uploaded
    beforehand, the condition every batch call here carries.  All three: ratio <= 1.0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import paircount_cost
    cells = {}
    for kind in ("context", "ensemble", "ragged"):
        r = paircount_cost.measure_context(nbx) if kind == "context" else paircount_cost.measure(nbx, kind)
        a, b = (r[k] for k in (("paircount_us", "neighbours_x16_us") if kind == "context" else ("batch_us", "contexts_us")))
        print("%s fp32: one call %.1f us, the other route %.1f us, ratio %.3f" % (kind, a, b, r["ratio"]))
        cells[kind] = r
    paircount_cost.write(paircount_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["same_values_from_both_arms"] and r["nradii"] == 16, kind
        assert (r["members"], r["n_min"], r["n_max"]) == {"context": (1, 8192, 8192), "ensemble": (16, 2048, 2048), "ragged": (16, 512, 4096)}[kind]
        assert r["ratio"] <= 1.0, r
