"""The field at caller-supplied points on the device (include/nbx_field.h) against tests/field_ref.py, as a context, as members
of an ensemble and as members of one ragged ensemble.  Every point of every case is checked.

Gates (field_ref): the acceleration's K = max_c |a^c - truth^c| / (u_T A) against 2 max(K_ref, 16), K_ref the CPU oracle's own K
on the points appended as massless bodies; the potential's K = |phi - truth| / (u_T |truth|) against 2 max(K_ref, 16), K_ref that of
a sequential sum in T.  Where A == 0 the acceleration must be exactly 0.  The largest K seen go to profiles/field_error.json.

Error budget behind the gates, to first order, u the unit round-off of T: a difference 1 u, r2 about 4 u, the reciprocal square
root 1 ulp (fp32: the hardware's; fp64: the seed corrected to second order, residual h^3 < 2^-70), cubed and multiplied: about
8 u on an acceleration term, 4 u on a potential term -- the K_TERM = 16 floor of force_ref covers either -- and the sums add
their length: a split's sequential sum in T over up to 1280 bodies, sqrt(1280) u ~ 36 u typical, less than the sequential sum
over all n that K_ref is measured on; the finish adds in fp64 and rounds once.

Cases, both precisions: field_ref.cases() -- the shapes (n, m) of field_ref.SHAPES with points uniform in the bounding box
("box"), the bodies' own positions where m <= n ("own"), 10^3 box sizes away ("far"), on a heavy body of force_ref's adversarial
state and 1e-4 beside it ("heavy"), and, for a state whose bodies all lie 50 away in every coordinate, the origin and its
neighbourhood ("origin": the padding records sit at the origin with G m = 0 and must add nothing)."""
import ctypes
import json
import os
import sys
import zlib

import numpy as np
import pytest

import field_ref as R
import force_ref as F
import kick_ref as K
from conftest import ROOT
from energy_ref import EPS2, gm_as_uploaded

pytestmark = pytest.mark.gpu

ERROR_FILE = os.path.join(ROOT, "profiles", "field_error.json")
PROBE_GATE = 32.0  # the potential probe's gate on nbx_diag_t.potential (tests/potential_ref.py)
_ctx, _worst = {}, {}


def same(a, b):
    """Two result dicts (or lists of arrays) hold the same bits."""
    ka = a.keys() if isinstance(a, dict) else range(len(a))
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).shape == np.asarray(b[k]).shape for k in ka)


def context_field(nbx, precision, state, points, key=None):
    """What a default context holding the state returns for the points, asked twice (the same bits); cached under `key`."""
    if key is not None and key in _ctx:
        return _ctx[key]
    with nbx.Context(len(state["mass"]), precision) as c:
        c.upload(state)
        r = c.field(*points)
        assert same(c.field(*points), r)  # two calls in a row
    if key is not None:
        _ctx[key] = r
    return r


def _record():
    out = {}
    if os.path.exists(ERROR_FILE):
        with open(ERROR_FILE) as f:
            out = json.load(f)
    out["what"] = ("largest K of nbx_field seen by tests/test_field_gpu.py over every point of every case, per precision and quantity: "
                   "acc: max_c |a^c - truth^c| / (u A), phi: |phi - truth| / (u |truth|), u = 2^-24 (fp32) or 2^-53 (fp64); gate and "
                   "k_ref are those of the case it was seen in (gate = 2 max(k_ref, 16), tests/field_ref.py)")
    for (precision, quantity), v in _worst.items():
        out.setdefault("fp%d" % precision, {})[quantity] = v
    os.makedirs(os.path.dirname(ERROR_FILE), exist_ok=True)
    with open(ERROR_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def check(result, c, precision, what):
    """Both gates over every point of case c; dtype and shape; exact zeros where A == 0."""
    m = len(c["points"][0])
    for k in R.KEYS:
        assert result[k].dtype == R.DTYPE[precision] and result[k].shape == (m,), (what, k)
    ka, kp = R.worst(result, c, precision)
    print("fp%d %s: acc K %.2f of %.1f (K_ref %.2f), phi K %.2f of %.1f (K_ref %.2f)"
          % (precision, what, ka, c["gate_acc"], c["kref_acc"], kp, c["gate_phi"], c["kref_phi"]))
    for quantity, k, gate, kref in (("acc", ka, c["gate_acc"], c["kref_acc"]), ("phi", kp, c["gate_phi"], c["kref_phi"])):
        if k > _worst.get((precision, quantity), {"K": -1.0})["K"]:
            _worst[(precision, quantity)] = {"K": k, "gate": gate, "k_ref": kref, "case": what}
    zero = c["truth"]["acc"][2] == 0
    for k in R.KEYS[:3]:
        assert (result[k][zero] == 0).all(), (what, k)
    assert ka <= c["gate_acc"], (precision, what, ka, c["gate_acc"])
    assert kp <= c["gate_phi"], (precision, what, kp, c["gate_phi"])


@pytest.mark.parametrize("n,m", R.SHAPES)
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_is_inside_both_gates_at_every_point(nbx, oracle, precision, n, m):
    for family in R.families_of(n, m):
        c = R.case(oracle, precision, n, m, family)
        r = context_field(nbx, precision, c["state"], c["points"], key=(precision, n, m, family))
        check(r, c, precision, "(n, m) = (%d, %d) %s" % (n, m, family))
    _record()


def test_every_family_and_every_split_shape_is_met():
    met = set(f for _, _, f in R.cases())
    assert met == set(R.FAMILIES)
    shapes = {(n, m): R.field_shape(m, n) for n, m in R.SHAPES}
    assert shapes[(4097, 4097)] == (9, 17, 4, 5) and shapes[(2049, 1025)] == (3, 9, 2, 5)  # several splits and columns
    assert shapes[(300, 2049)] == (5, 2, 1, 2)                                               # more columns than tiles
    assert shapes[(4097, 2)] == (1, 17, 4, 5) and shapes[(513, 1)] == (1, 3, 1, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# NULL outputs and the slack behind every array
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_null_outputs_are_skipped_and_nothing_is_written_beyond_m(nbx, oracle, precision):
    n, m, slack = 257, 513, 16
    c = R.case(oracle, precision, n, m, "box")
    full = context_field(nbx, precision, c["state"], c["points"], key=(precision, n, m, "box"))
    T = R.DTYPE[precision]
    L = nbx.load()
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    pts = [np.concatenate([p, np.full(slack, np.nan, dtype=T)]) for p in c["points"]]  # what lies behind the points is not read
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        for pick in ([0, 1, 2, 3], [0], [1], [2], [3], [0, 3], []):
            out = [np.full(m + slack, -7.25, dtype=T) for _ in range(4)]
            args = [ptr(out[k]) if k in pick else None for k in range(4)]
            assert L.nbx_field(ctx._h, m, *[ptr(p) for p in pts], *args) == nbx.NBX_OK, pick
            for k in range(4):
                assert (out[k][m:] == -7.25).all(), (pick, k)  # the slack
                if k in pick:
                    assert out[k][:m].tobytes() == full[R.KEYS[k]].tobytes(), (pick, k)
                else:
                    assert (out[k] == -7.25).all(), (pick, k)
        out = np.full(4, -7.25, dtype=T)
        assert L.nbx_field(ctx._h, 0, None, None, None, ptr(out), ptr(out), ptr(out), ptr(out)) == nbx.NBX_OK and (out == -7.25).all()  # m == 0


# ---------------------------------------------------------------------------------------------------------------------------
# bit contracts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_a_sliced_context_gives_the_bits_of_the_whole_one(nbx, oracle, precision):
    n, m = 2049, 1025
    c = R.case(oracle, precision, n, m, "box")
    whole = context_field(nbx, precision, c["state"], c["points"], key=(precision, n, m, "box"))
    for sl in (dict(i_begin=1000, i_count=300), dict(i_begin=0, i_count=512, n_alloc=2304), dict(i_begin=2048, i_count=1)):
        with nbx.Context(n, precision, **sl) as ctx:
            ctx.upload(c["state"])
            assert same(ctx.field(*c["points"]), whole), sl


@pytest.mark.parametrize("precision", [32, 64])
def test_a_small_call_after_a_large_one_equals_a_fresh_objects(nbx, oracle, precision):
    n = 4097
    big, small = R.case(oracle, precision, n, 4097, "box"), R.case(oracle, precision, n, 2, "box")
    want_big = context_field(nbx, precision, big["state"], big["points"], key=(precision, n, 4097, "box"))
    want_small = context_field(nbx, precision, small["state"], small["points"], key=(precision, n, 2, "box"))
    with nbx.Context(n, precision) as ctx:
        ctx.upload(small["state"])  # the same state in both cases: a family's state depends on n alone
        assert same(ctx.field(*small["points"]), want_small)  # the buffers are allocated small ...
        assert same(ctx.field(*big["points"]), want_big)      # ... grow ...
        assert same(ctx.field(*small["points"]), want_small)  # ... and serve a small call again
    assert all(np.array_equal(big["state"][f], small["state"][f]) for f in K.FIELDS)


def _member_state(precision, n, k):
    return K.make_state(7000 + 13 * k + n, n, R.DTYPE[precision])


def _member_points(precision, state, m, k):
    return R.make_points(precision, state, m, "box", seed=1 + k)


def _ranges(S):
    return [(0, S)] + [(k, 1) for k in range(S)] + [(1, S - 1)]


@pytest.mark.parametrize("n,m", [(257, 513), (2049, 1025)])
@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_have_the_bits_of_a_context(nbx, precision, n, m):
    S = 5
    states = [_member_state(precision, n, k) for k in range(S)]
    pts = [_member_points(precision, s, m, k) for k, s in enumerate(states)]
    want = [context_field(nbx, precision, s, p) for s, p in zip(states, pts)]
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        for first, count in _ranges(S):
            P = [np.stack([pts[k][c] for k in range(first, first + count)]) for c in range(3)]
            got = e.field(*P, first=first, count=count)
            for j in range(count):
                assert all(got[key].shape == (count, m) for key in R.KEYS)
                assert same({key: got[key][j] for key in R.KEYS}, want[first + j]), (first, count, j)


@pytest.mark.parametrize("m", [513, 3])
@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_have_the_bits_of_a_context_of_their_size(nbx, precision, m):
    """m = 513: the member of 2049 bodies has two j splits, every other member one -- its second row of workgroups returns at once
    for the others."""
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    assert sorted(set(R.field_shape(m, n)[2] for n in sizes)) == [1, 2]
    states = [_member_state(precision, n, k) for k, n in enumerate(sizes)]
    pts = [_member_points(precision, s, m, k) for k, s in enumerate(states)]
    want = [context_field(nbx, precision, s, p) for s, p in zip(states, pts)]
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        for first, count in _ranges(S):
            P = [np.stack([pts[k][c] for k in range(first, first + count)]) for c in range(3)]
            got = r.field(*P, first=first, count=count)
            for j in range(count):
                assert same({key: got[key][j] for key in R.KEYS}, want[first + j]), (first, count, j)


# ---------------------------------------------------------------------------------------------------------------------------
# the identities of the header
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4097])
@pytest.mark.parametrize("precision", [32, 64])
def test_at_the_bodies_own_positions_the_field_is_the_bodies_acceleration_and_potential(nbx, oracle, precision, n):
    c = R.case(oracle, precision, n, n, "own")
    st = c["state"]
    r = context_field(nbx, precision, st, c["points"], key=(precision, n, n, "own"))
    with nbx.Context(n, precision) as ctx:
        ctx.upload(st)
        acc = ctx.accel()
        U = ctx.diagnostics()["potential"]
    k_field = R.k_acc([r[k] for k in R.KEYS[:3]], c["truth"], precision).max()
    k_accel = R.k_acc(acc, c["truth"], precision).max()
    print("fp%d n = %d: K of field %.2f, of accel() %.2f, gate %.1f" % (precision, n, k_field, k_accel, c["gate_acc"]))
    assert k_field <= c["gate_acc"] and k_accel <= c["gate_acc"]  # both inside the gate of the same truth
    mass, gm = st["mass"].astype(np.float64), gm_as_uploaded(st["mass"])
    phi = r["phi"].astype(np.float64)
    got = 0.5 * float(np.sum(mass * (phi + gm / np.sqrt(EPS2))))
    u = F.U[precision]
    bound = u * (c["gate_phi"] * float(np.sum(0.5 * mass * np.abs(phi))) + PROBE_GATE * abs(U))
    print("fp%d n = %d: 1/2 sum m (phi + G m / eps) = %.17g, potential %.17g, |difference| %.3g of %.3g" % (precision, n, got, U, abs(got - U), bound))
    assert abs(got - U) <= bound
    if n == 1:
        assert U == 0.0 and r["phi"][0] < 0  # phi(x_0) = -G m_0 / eps: the point is not the body


# ---------------------------------------------------------------------------------------------------------------------------
# ordering and no side effects
# ---------------------------------------------------------------------------------------------------------------------------
def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


def _flat(down):
    if isinstance(down, dict):
        return [down[f] for f in K.FIELDS[:6]]
    return [d[f] for d in down for f in K.FIELDS[:6]]


def _make(nbx, kind, precision=32):
    sizes = (300, 2049, 513)
    T = R.DTYPE[precision]
    if kind == "context":
        st = K.make_state(40, 2049, T)
        return nbx.Context(2049, precision), st, _member_points(precision, st, 700, 0)
    if kind == "ensemble":
        sts = [K.make_state(40 + k, 2049, T) for k in range(3)]
    else:
        sts = [K.make_state(40 + k, n, T) for k, n in enumerate(sizes)]
    pts = [_member_points(precision, s, 700, k) for k, s in enumerate(sts)]
    P = [np.stack([p[c] for p in pts]) for c in range(3)]
    return (nbx.Ensemble(2049, 3, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)), sts, P


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_the_call_is_on_the_stream_and_leaves_the_trajectory_and_every_counter_alone(nbx, kind):
    dt = 1.0 / 256
    o, states, P = _make(nbx, kind)
    with o:
        o.upload(states)
        f0 = o.field(*P)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the call describes the state after these steps
        f3 = o.field(*P)
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        assert same(o.field(*P), f3)
        after = o.stats()
        assert before == after  # steps_done, every *_timed / *_ms_total field, graph replays: all of it
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        ke_a = o.step(3, dt)
        a = _flat(o.download())
        stats_a = o.stats()
    o, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.step(3, dt)  # synchronises
        o.sync()
        assert same(o.field(*P), f3)  # stepped, synchronised and asked then
    o, _, _ = _make(nbx, kind)
    with o:  # an object that never made the call
        o.upload(states)
        o.profile(True)
        o.step(3, dt, kenergy=False)
        o.sync()
        assert np.array_equal(o.step(0, dt), ke0) and np.array_equal(o.step(0, dt), ke0)  # twice, as above
        ke_b = o.step(3, dt)
        b = _flat(o.download())
        stats_b = o.stats()
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)
    timing = ("force_ms_total", "step_ms_total")  # measured times differ from run to run; the counts do not
    assert {k: v for k, v in stats_a.items() if k not in timing} == {k: v for k, v in stats_b.items() if k not in timing}
    assert not same(f0, f3)


# ---------------------------------------------------------------------------------------------------------------------------
# state and argument errors on real objects
# ---------------------------------------------------------------------------------------------------------------------------
def test_state_errors(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    p = _member_points(32, states[0], 7, 0)
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.field(*p)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_field: nbx_upload has not been called" in str(err.value)
        c.upload(states[0])
        assert c.field(*p)["phi"].shape == (7,)
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.field(*p)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_field: a local step awaits nbx_commit" in str(err.value)
    for make, name in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged_field"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble_field")):
        st = states if "ragged" in name else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        P = lambda count: [np.stack([p[c]] * count) if count > 0 else np.zeros((0, 7), dtype=np.float32) for c in range(3)]
        with make() as o:
            with pytest.raises(nbx.NbxError) as err:
                o.field(*P(4))
            assert err.value.code == nbx.NBX_ERR_STATE and (name + ": member 0 has not been uploaded") in str(err.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                with pytest.raises(nbx.NbxError) as err:
                    o.field(*P(count), first=first, count=count)
                assert err.value.code == nbx.NBX_ERR_STATE and "member 3 has not been uploaded" in str(err.value), (first, count)
            part = o.field(*P(3), first=0, count=3)  # the uploaded members can be asked before the others arrive
            assert part["phi"].shape == (3, 7)
            L = nbx.load()
            f = getattr(L, name)
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            q = P(4)
            out = np.full(4, -7.25, dtype=np.float32)
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                assert f(o._h, first, count, 7, *[ptr(a) for a in q], ptr(out), None, None, None) == nbx.NBX_ERR_ARG, (first, count)
            # more than 2^22 points in all: refused before the arrays are read
            assert f(o._h, 0, 3, (1 << 22) // 3 + 1, *[ptr(a) for a in q], ptr(out), None, None, None) == nbx.NBX_ERR_ARG
            assert L.nbx_last_error().decode() == name + ": count * m exceeds 4194304"
            assert f(o._h, 1, 0, 7, *[ptr(a) for a in q], ptr(out), ptr(out), ptr(out), ptr(out)) == nbx.NBX_OK  # count == 0
            assert (out == -7.25).all()
            o.upload(st[3:], first=3)
            assert same(o.field(*P(3), first=0, count=3), part)


# ---------------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_call_costs_no_more_than_what_it_replaces(nbx):
    """fp32, in this process, rounds alternated, medians (tools/field_cost.py): one nbx_field call for n = m = 4096 against upload
    + nbx_accel on a context of 8192 bodies created beforehand; one nbx_ensemble_field call over 16 x 2048 (m = 2048) and one
    nbx_ragged_field call over 16 sizes 512 ... 4096 (m = 1024) against 16 nbx_field calls on contexts created and uploaded
    beforehand.  The arm each replaces does strictly more pair work (four times the pairs) or more calls (16 uploads, 32 launches,
    16 synchronisations against 1, 2 and 1), so no further margin is claimed: ratio <= 1.0, the condition the sibling features use.
    The pair rate at n = m = 131072 against nbx_accel is recorded, not gated."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import field_cost
    cells = {"context": field_cost.measure_context(nbx)}
    r = cells["context"]
    print("context fp32 n = m = 4096: field %.1f us, upload + accel of 8192 bodies %.1f us, ratio %.3f" % (r["field_us"], r["workaround_us"], r["ratio"]))
    for kind in ("ensemble", "ragged"):
        r = cells[kind] = field_cost.measure(nbx, kind)
        print("%s fp32 m = %d: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["m"], r["batch_us"], r["contexts_us"], r["ratio"]))
    r = cells["context_n%d" % field_cost.LARGE_N] = field_cost.measure_large(nbx)
    print("context fp32 n = m = %d: field %.1f us (%.3g pair/s), accel %.1f us (%.3g pair/s), rate ratio %.2f"
          % (r["n"], r["field_us"], r["field_pairs_per_s"], r["accel_us"], r["accel_pairs_per_s"], r["pair_rate_ratio"]))
    field_cost.write(field_cost.OUT, cells)
    assert (cells["context"]["n"], cells["context"]["m"]) == (4096, 4096) and cells["context"]["accelerations_agree"]
    for kind in ("ensemble", "ragged"):
        r = cells[kind]
        assert r["members"] == 16 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"], r["m"]) == ((2048, 2048, 2048) if kind == "ensemble" else (512, 4096, 1024))
    for kind in ("context", "ensemble", "ragged"):
        assert cells[kind]["ratio"] <= 1.0, (kind, cells[kind]["ratio"])
