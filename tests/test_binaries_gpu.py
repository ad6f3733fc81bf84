"""Most bound partner and bound count of every body on the device (include/nbx_binaries.h) against the fp64 numpy reference
tests/binaries_ref.py, as a context, as members of an ensemble and as members of one ragged ensemble.

What is asked (binaries_ref.compare): partner EQUALS the reference on every body -- the states have no ambiguous body at all,
which test_binaries_cpu.py asserts with the reference alone --; energy within GATE u (A + B) of the reference value of its own
pair and of the reference minimum, A and B the two terms e is the difference of, GATE the project's timescale gates, 32 in fp32
and 128 in fp64 (the header derives 6.5 u and at most 55.5 u to first order; the gate is not tightened to what is seen); bound
inside the bracket the same window around e = 0 allows, exact wherever the reference shows no pair inside it.  The largest
energy error seen goes to profiles/binaries_error.json, in units of u (A + B).

Shapes, the smallest at which each part can go wrong: n = 1 and 2, 255, 256, 257 (one column, one split; one tile, a full tile,
two tiles with 255 padding records), 513 (two columns), 1025, 2049 (five columns, two splits of 5 and 4 tiles), 4097 (nine columns,
four splits, the last one short), an ensemble of 3 x 2049, a ragged ensemble of neighbours_ref.RAGGED_SIZES, lattice(13) = 2197
bodies (two splits meeting at j = 1280, so equal candidates arrive from both)."""
import ctypes
import json
import math
import os
import sys
import zlib

import numpy as np
import pytest

import binaries_ref as R
import kick_ref as K
import neighbours_ref as NB
from conftest import ROOT

pytestmark = pytest.mark.gpu

ERROR_FILE = os.path.join(ROOT, "profiles", "binaries_error.json")
FAMILIES = {"cloud": R.cloud, "reversed": R.reversed_cloud, "clustered": R.clustered}
_states, _refs, _ctx, _worst = {}, {}, {}, {}


def state(precision, family, n):
    key = (precision, family, n)
    if key not in _states:
        if family.startswith("lattice"):
            _states[key] = R.lattice(precision, perm=family == "lattice permuted")
        elif family == "encounter":
            _states[key] = R.encounter(precision)
        else:
            _states[key] = FAMILIES[family](n, precision)
    return _states[key]


def ref(precision, family, n):
    """The reference's values, computed once per state and left unchanged."""
    key = (precision, family, n)
    if key not in _refs:
        r = R.binaries(state(precision, family, n), precision)
        for a in r.values():
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def same(a, b, keys=R.KEYS):
    return all(np.array_equal(a[k], b[k]) if a[k] is not None else b[k] is None for k in keys)


def context_values(nbx, precision, family, n):
    """What a default context of n bodies holding the state returns, asked once per state: the bits the members are held to."""
    key = (precision, family, n)
    if key not in _ctx:
        with nbx.Context(n, precision) as c:
            c.upload(state(precision, family, n))
            got = c.binaries()
            assert same(c.binaries(), got)  # two calls in a row: the same bits
            plain = c.binaries(bound=False)  # the kernels compiled without the count
            assert plain["bound"] is None and same(plain, got, ("partner", "energy"))
        _ctx[key] = got
    return _ctx[key]


def _record():
    out = {"what": ("largest deviation of energy[] of nbx_binaries / nbx_ensemble_binaries / nbx_ragged_binaries from the fp64 reference "
                    "tests/binaries_ref.py (the value of the body's own pair) seen by tests/test_binaries_gpu.py and, on its cloud of 35937 bodies, "
                    "tests/test_large_shapes_gpu.py, in units of u (A + B), "
                    "u = 2^-24 (fp32) or 2^-53 (fp64), A = |dv|^2 / 2 and B = G (m_i + m_j) / sqrt(r2) the two terms e is the "
                    "difference of; gates: 32 (fp32), 128 (fp64); first-order bounds of the header: 6.5 and 55.5")}
    if os.path.exists(ERROR_FILE):
        with open(ERROR_FILE) as f:
            out.update({k: v for k, v in json.load(f).items() if k != "what"})
    for precision, v in _worst.items():
        if v["u"] >= out.get("fp%d" % precision, {"u": -1.0})["u"]:
            out["fp%d" % precision] = v
    os.makedirs(os.path.dirname(ERROR_FILE), exist_ok=True)
    with open(ERROR_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def note_worst(precision, worst, n, family):
    """The largest energy deviation seen so far goes to profiles/binaries_error.json (tests/test_large_shapes_gpu.py feeds its
    cloud of 35 937 bodies through here too)."""
    if worst > _worst.get(precision, {"u": -1.0})["u"]:
        _worst[precision] = {"u": worst, "n": n, "state": family}
        _record()


def check(got, precision, family, n, partner=None):
    """`partner`: what partner is held to where it is not the reference's argmin (the lattice: the geometry's closed form)."""
    st = state(precision, family, n)
    want = ref(precision, family, n)
    if partner is not None:
        want = dict(want, partner=partner)
    assert got["partner"].dtype == np.int32 and got["bound"].dtype == np.int32 and got["energy"].dtype == R.DTYPE[precision]
    assert got["partner"].shape == got["energy"].shape == got["bound"].shape == (n,)
    if n == 1:  # no partner
        assert got["partner"].tolist() == [-1] and got["energy"].tolist() == [math.inf] and got["bound"].tolist() == [0]
        return
    problems, worst = R.compare(got, want, st, precision)
    exact = int((want["bound_lo"] == want["bound_hi"]).sum())
    print("fp%d %s(%d): %d partners differ, energy worst %.2f u (A + B) of %g, bound equal on %d bodies (%d are exact by the reference), mean %.1f, "
          "%d unbound" % (precision, family, n, (got["partner"] != want["partner"]).sum(), worst, R.GATE[precision],
                          (got["bound"] == want["bound"]).sum(), exact, got["bound"].mean(), (got["bound"] == 0).sum()))
    note_worst(precision, worst, n, family)
    assert not problems, (precision, family, n, problems)
    assert not R.identities(got), (precision, family, n, R.identities(got))  # the Consequences of the header


@pytest.mark.parametrize("n", R.CONTEXT_SIZES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference(nbx, precision, n):
    got = context_values(nbx, precision, "cloud", n)
    check(got, precision, "cloud", n)
    if n >= 255:
        assert 0 < got["bound"].min() and got["bound"].max() < n - 1  # every body has bound and unbound partners


@pytest.mark.parametrize("family,n", [("clustered", 513), ("clustered", 2049), ("encounter", 96)])
@pytest.mark.parametrize("precision", [32, 64])
def test_planted_binaries_the_triple_and_the_escapers_are_found(nbx, precision, family, n):
    got = context_values(nbx, precision, family, n)
    check(got, precision, family, n)
    st = state(precision, family, n)
    if family == "encounter":
        assert (got["bound"] == 0).sum() == (ref(precision, family, n)["bound"] == 0).sum() > 0
        return
    p = R.planted(n)
    cat = nbx.binary_catalogue(got["partner"], got["energy"], st["mass"], *[st[k] for k in R.POS + R.VEL])
    found = set(zip(cat["i"].tolist(), cat["j"].tolist()))
    for i, j in p["binaries"] + [p["triple"][:2]]:
        assert got["partner"][i] == j and got["partner"][j] == i and got["energy"][i] == got["energy"][j] < 0  # a mutual bound pair, exactly
        assert (min(i, j), max(i, j)) in found
    a, b, c = p["triple"]
    assert got["bound"][a] >= 2 and got["bound"][c] >= 1
    assert (got["bound"][list(p["escapers"])] == 0).all() and (got["energy"][list(p["escapers"])] > 0).all()
    planted_rows = [k for k in range(len(cat["i"])) if (int(cat["i"][k]), int(cat["j"][k])) in {(min(i, j), max(i, j)) for i, j in p["binaries"]}]
    assert len(planted_rows) == 3 and np.allclose(cat["a"][planted_rows], R.BINARY_SEP, rtol=1e-3) and (cat["ecc"][planted_rows] < 1e-2).all()


@pytest.mark.parametrize("precision", [32, 64])
def test_two_massless_bodies_moving_as_one_have_energy_zero_exactly_and_are_not_bound(nbx, precision):
    s = {k: np.array(v, dtype=R.DTYPE[precision]) for k, v in zip(K.FIELDS, ([0.25, 5.0], [1.0, 1.5], [-2.0, 0.5], [1.0, 1.0], [2.0, 2.0], [3.0, 3.0],
                                                                     [0.0, 0.0]))}
    with nbx.Context(2, precision) as c:
        c.upload(s)
        got = c.binaries()
        assert got["partner"].tolist() == [1, 0] and got["energy"].tolist() == [0.0, 0.0] and got["bound"].tolist() == [0, 0]  # < 0, not <= 0
        s["mass"][:] = 1.0 / R.G
        c.upload(s)
        got = c.binaries()
        assert got["partner"].tolist() == [1, 0] and got["bound"].tolist() == [1, 1] and got["energy"][0] == got["energy"][1] < 0


@pytest.mark.parametrize("family", ["lattice", "lattice permuted"])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_gives_the_lowest_index_face_neighbour_and_one_energy_per_distance_class(nbx, precision, family):
    k = R.LATTICE_K
    n = k ** 3
    index, faces = NB.lattice_expected(k, perm=family == "lattice permuted")
    got = context_values(nbx, precision, family, n)
    assert np.array_equal(got["partner"], index), np.nonzero(got["partner"] != index)[0][:8]  # the lowest index under 6-fold ties
    assert (got["bound"] == n - 1).all()  # at rest: every pair is bound
    size = got["energy"].itemsize
    assert len(set(got["energy"].tobytes()[i * size:(i + 1) * size] for i in range(n))) == 1  # one distance class, one bit pattern
    assert sorted(set(faces.tolist())) == [3, 4, 5, 6]
    check(got, precision, family, n, partner=index)


@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_reference_and_have_the_bits_of_a_context(nbx, precision):
    n = R.ENSEMBLE_N
    families = ("cloud", "clustered", "reversed")
    S = len(families)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload([state(precision, f, n) for f in families])
        full = e.binaries()
        assert same(e.binaries(), full) and all(full[k].shape == (S, n) for k in R.KEYS)
        for m, f in enumerate(families):
            got = {k: full[k][m] for k in R.KEYS}
            check(got, precision, f, n)
            assert same(got, context_values(nbx, precision, f, n)), (precision, n, f)
        # a member's results are the same whatever first and count it was asked with: a sub-range, single members, empty ranges
        for first, count in ((1, 2), (0, 1), (1, 1), (2, 1), (0, 2), (S, 0), (0, 0)):
            part = e.binaries(first=first, count=count)
            assert all(np.array_equal(part[k], full[k][first:first + count]) for k in R.KEYS), (first, count)
        assert same(e.binaries(first=1), {k: full[k][1:] for k in R.KEYS})
        plain = e.binaries(bound=False, first=1, count=2)
        assert plain["bound"] is None and all(np.array_equal(plain[k], full[k][1:3]) for k in ("partner", "energy"))
        assert same(e.binaries(), full)


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    with nbx.Ragged(sizes, precision) as r:
        r.upload([state(precision, "cloud", n) for n in sizes])
        full = r.binaries()
        assert len(full) == S and all(same(a, b) for a, b in zip(r.binaries(), full))
        for m, n in enumerate(sizes):
            check(full[m], precision, "cloud", n)
            assert same(full[m], context_values(nbx, precision, "cloud", n)), (precision, n)
        for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (0, 1), (1, 3), (5, 3), (S, 0), (3, 0)):
            part = r.binaries(first=first, count=count)
            assert len(part) == count and all(same(a, b) for a, b in zip(part, full[first:first + count])), (first, count)
        assert all(same(a, b) for a, b in zip(r.binaries(first=5), full[5:]))
        plain = r.binaries(bound=False, first=2, count=5)
        assert all(a["bound"] is None and same(a, b, ("partner", "energy")) for a, b in zip(plain, full[2:7]))
        assert all(same(a, b) for a, b in zip(r.binaries(), full))  # a partial call leaves nothing behind that a full one sees
        # the layout is end to end, member `first` at element 0, and nothing is written behind the last member
        first, count = 2, 4
        total = sum(sizes[first:first + count])
        flat = [np.full(total + 8, -7, dtype=np.int32), np.full(total + 8, -7.25, dtype=R.DTYPE[precision]), np.full(total + 8, -7, dtype=np.int32)]
        assert nbx.load().nbx_ragged_binaries(r._h, first, count, *[a.ctypes.data_as(ctypes.c_void_p) for a in flat]) == nbx.NBX_OK
        for a, k in zip(flat, R.KEYS):
            assert np.array_equal(a[:total], np.concatenate([full[m][k] for m in range(first, first + count)])), k
            assert (a[total:] == a.dtype.type(-7 if k != "energy" else -7.25)).all(), k
    # the same systems in another order: other offsets, other rows, partner stays member-local -- the same bits
    with nbx.Ragged(sizes[::-1], precision) as r:
        r.upload([state(precision, "cloud", n) for n in sizes][::-1])
        assert all(same(a, b) for a, b in zip(r.binaries(), full[::-1]))


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 4)] +
    [dict(kernel_variant="KERNEL_SGPRW", bodies_per_lane=2), dict(kernel_variant="KERNEL_JLANE", bodies_per_lane=4)] +
    [dict(j_split=s) for s in (1, 4, 32)] + [dict(kernel_variant="KERNEL_LDS", j_split=4)])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_bits_do_not_depend_on_the_contexts_options_and_a_sliced_context_is_refused(nbx, precision):
    n = 2049
    s = state(precision, "cloud", n)
    want = context_values(nbx, precision, "cloud", n)
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
            assert same(c.binaries(), want), (o, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    print("fp%d: %d of %d option sets made a context; distinct shapes: %d" % (precision, len(made), len(CONTEXT_OPTIONS), len(set(made))))
    assert {m[0] for m in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR} and {m[1] for m in made} == {nbx.ORDER_TREE, nbx.ORDER_REFERENCE}
    assert len(set(made)) >= 6
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # the velocities of the others are not resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as c:
            c.upload(s)
            for bound in (True, False):
                with pytest.raises(nbx.NbxError) as err:
                    c.binaries(bound)
                assert err.value.code == nbx.NBX_ERR_STATE and "nbx_binaries: the context owns a slice of the bodies" in str(err.value)
            assert nbx.load().nbx_binaries(c._h, None, None, None) == nbx.NBX_ERR_STATE  # the state comes before "nothing to do"


def _raw(nbx, o, kind, arrays, first=0, count=None):
    L = nbx.load()
    ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    if kind == "context":
        return L.nbx_binaries(o._h, *ptr)
    f = L.nbx_ensemble_binaries if kind == "ensemble" else L.nbx_ragged_binaries
    return f(o._h, first, o.members if count is None else count, *ptr)


def _make(nbx, kind, precision=32):
    """An object of the kind with its states and the number of bodies a call over all of it returns."""
    sizes = (257, 2049, 513)
    if kind == "context":
        return nbx.Context(2049, precision), state(precision, "cloud", 2049), 2049
    if kind == "ensemble":
        return nbx.Ensemble(2049, 3, precision), [state(precision, f, 2049) for f in ("cloud", "clustered", "reversed")], 3 * 2049
    return nbx.Ragged(sizes, precision), [state(precision, "cloud", n) for n in sizes], sum(sizes)


def _flatten(res):
    if isinstance(res, dict):
        return {k: None if res[k] is None else res[k].reshape(-1) for k in R.KEYS}
    return {k: None if res[0][k] is None else np.concatenate([m[k] for m in res]) for k in R.KEYS}


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
@pytest.mark.parametrize("precision", [32, 64])
def test_a_null_output_is_skipped_alone_and_without_bound_the_count_is_not_asked_for(nbx, precision, kind):
    o, states, total = _make(nbx, kind, precision)
    T = R.DTYPE[precision]
    with o:
        o.upload(states)
        full = _flatten(o.binaries())
        assert full["bound"].sum() > 0
        for skip in range(3):
            arrays = [np.full(total, -7, dtype=np.int32), np.full(total, -7.25, dtype=T), np.full(total, -7, dtype=np.int32)]
            keep = list(arrays)
            arrays[skip] = None
            assert _raw(nbx, o, kind, arrays) == nbx.NBX_OK
            for k, a in enumerate(keep):
                if k == skip:
                    assert (a == a.dtype.type(-7.25 if k == 1 else -7)).all()  # never written
                else:
                    assert np.array_equal(a, full[R.KEYS[k]]), (skip, k)  # skip == 2: the kernels compiled without the count
        only = [None, None, np.full(total, -7, dtype=np.int32)]
        assert _raw(nbx, o, kind, only) == nbx.NBX_OK and np.array_equal(only[2], full["bound"])
        assert _raw(nbx, o, kind, [None] * 3) == nbx.NBX_OK  # all NULL: the arguments are checked, nothing is launched
        plain = _flatten(o.binaries(bound=False))
        assert plain["bound"] is None and np.array_equal(plain["partner"], full["partner"]) and np.array_equal(plain["energy"], full["energy"])


def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


def _positions(down):
    if isinstance(down, dict):
        return [down[f] for f in K.FIELDS[:6]]
    return [d[f] for d in down for f in K.FIELDS[:6]]


UNTOUCHED = ("steps_done", "force_launches_timed", "force_ms_total", "launches_timed", "step_ms_total", "graph_replays")


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_the_call_is_on_the_stream_and_leaves_the_trajectory_and_every_counter_alone(nbx, kind):
    dt = 1.0 / 4096
    o, states, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        b3 = _flatten(o.binaries())
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        again = _flatten(o.binaries())
        after = o.stats()
        assert {k: before[k] for k in UNTOUCHED if k in before} == {k: after[k] for k in UNTOUCHED if k in after} and before["steps_done"] == 3
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        ke_a = o.step(3, dt)
        a = _positions(o.download())
    assert same(b3, again)
    o, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.step(3, dt)  # synchronises
        o.sync()
        assert same(_flatten(o.binaries()), b3)
    o, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        b0 = _flatten(o.binaries())
        ke_b = o.step(6, dt)
        b = _positions(o.download())
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)  # the bits of later steps are as without the call
    assert not np.array_equal(b0["energy"], b3["energy"])


def test_state_errors(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    with nbx.Context(300, 32) as c:
        for bound in (True, False):
            with pytest.raises(nbx.NbxError) as err:
                c.binaries(bound)
            assert err.value.code == nbx.NBX_ERR_STATE and "nbx_binaries: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        got = c.binaries()
        assert got["partner"].shape == (300,)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.binaries()
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_binaries: a local step awaits nbx_commit" in str(err.value)
        assert _raw(nbx, c, "context", [None] * 3) == nbx.NBX_ERR_STATE  # the state comes before "nothing to do"
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_binaries"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_binaries")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.binaries()
            assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value) and name in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.binaries(first=first, count=count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value), (first, count)
            part = _flatten(o.binaries(first=0, count=3))  # the uploaded members can be asked before the others arrive
            assert part["partner"].shape == (sum(len(s["mass"]) for s in st[:3]),)
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                with pytest.raises(nbx.NbxError) as err:
                    o.binaries(first=first, count=count)
                assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value), (first, count)
            o.upload(st[3:], first=3)
            assert same(_flatten(o.binaries(first=0, count=3)), part)


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32: one batch call against 16
    nbx_binaries calls on contexts created and uploaded beforehand, in this process, rounds alternated (tools/binaries_cost.py).
    The pair work of the two arms is the same and one call issues 2 launches and 1 synchronisation where the contexts issue 32
    and 16, so the gate has no further margin: ratio <= 1.0, the condition every batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import binaries_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = binaries_cost.measure(nbx, kind)
        print("%s fp32: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["batch_us"], r["contexts_us"], r["ratio"]))
        cells[kind] = r
    binaries_cost.write(binaries_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
