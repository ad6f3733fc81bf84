"""The tidal tensor on the device (include/nbx_tidal.h) against tests/tidal_ref.py, at caller-supplied points and at the bodies
themselves, as a context, as members of an ensemble and as members of one ragged ensemble.  Every point and body of every case
is checked, all six components.

Gate (tidal_ref): K = max_ab |T_ab - truth_ab| / (u_T A_ab) against 2 max(K_ref, floor), K_ref the K of a sequential sum in T with
a correctly rounded 1 / sqrt, floor the first-order error of one term derived in the header (30.5 u fp32, 24 u fp64).  Where
A_ab == 0 the value must be exactly 0.  The largest K seen go to profiles/tidal_error.json.

Measured on an MI355X (profiles/tidal_error.json holds the last run): largest K 44.9 of a gate of 110.4 in fp32 points mode
((n, m) = (2049, 1025), own), 40.1 of 912.3 in fp32 bodies mode (the lattice), 37.9 of 127.1 in fp64 points mode ((4097, 4097),
own), 38.6 of 77.2 in fp64 bodies mode (n = 1025, adversarial).  Nothing below depends on these figures.

Cases, both precisions.  Points mode: field_ref.cases() -- the shapes (n, m) of field_ref.SHAPES with points uniform in the
bounding box, at the bodies' own positions, 10^3 box sizes away, on a heavy body and 1e-4 beside it, and about the origin for a
state 50 away from it.  Bodies mode: tidal_ref.BODY_SIZES, both sides of every tile and column seam, on the kick_ref clouds and
force_ref's adversarial state (coincident bodies, twelve decades of mass, massless bodies)."""
import ctypes
import json
import os
import sys
import zlib

import numpy as np
import pytest

import field_ref as FR
import force_ref as F
import kick_ref as K
import lattice_ref as LR
import tidal_ref as R
from conftest import ROOT
from energy_ref import EPS2, gm_as_uploaded

pytestmark = pytest.mark.gpu

ERROR_FILE = os.path.join(ROOT, "profiles", "tidal_error.json")
KEYS = R.KEYS
_ctx, _worst = {}, {}


def same(a, b):
    """Two result dicts hold the same bits."""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).shape == np.asarray(b[k]).shape for k in KEYS)


def context_tidal(nbx, precision, state, points=None, key=None):
    """What a default context holding the state returns for the points (None: at its bodies), asked twice (the same bits); cached
    under `key`."""
    if key is not None and key in _ctx:
        return _ctx[key]
    with nbx.Context(len(state["mass"]), precision) as c:
        c.upload(state)
        ask = (lambda: c.tidal_bodies()) if points is None else (lambda: c.tidal(*points))
        r = ask()
        assert same(ask(), r)  # two calls in a row
    if key is not None:
        _ctx[key] = r
    return r


def _record():
    out = {}
    if os.path.exists(ERROR_FILE):
        with open(ERROR_FILE) as f:
            out = json.load(f)
    out["what"] = ("largest K seen by tests/test_tidal_gpu.py over every point or body of every case, per precision and mode: "
                   "K = max over the six components of |T_ab - truth_ab| / (u A_ab), u = 2^-24 (fp32) or 2^-53 (fp64); gate and k_ref are "
                   "those of the case it was seen in (gate = 2 max(k_ref, floor), floor 30.5 (fp32) or 24 (fp64), tests/tidal_ref.py)")
    for (precision, mode), v in _worst.items():
        out.setdefault("fp%d" % precision, {})[mode] = v
    os.makedirs(os.path.dirname(ERROR_FILE), exist_ok=True)
    with open(ERROR_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def check(result, c, precision, what, rows=None):
    """The gate over every point of case c (or its checked rows), all six components; dtype; exact zeros where A == 0."""
    for k in KEYS:
        assert result[k].dtype == R.DTYPE[precision], (what, k)
    k = float(R.k_metric(result, c["truth"], precision, rows=rows).max())
    print("fp%d %s: K %.2f of %.1f (K_ref %.2f)" % (precision, what, k, c["gate"], c["kref"]))
    mode = "bodies" if c["bodies"] else "points"
    if k > _worst.get((precision, mode), {"K": -1.0})["K"]:
        _worst[(precision, mode)] = {"K": k, "gate": c["gate"], "k_ref": c["kref"], "case": what}
    assert k <= c["gate"], (precision, what, k, c["gate"])  # inf where a value with A == 0 is not an exact zero
    return k


# ---------------------------------------------------------------------------------------------------------------------------
# the gates
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", FR.SHAPES)
@pytest.mark.parametrize("precision", [32, 64])
def test_points_mode_is_inside_the_gate_at_every_point_and_component(nbx, precision, n, m):
    for family in FR.families_of(n, m):
        c = R.case(precision, n, m, family)
        r = context_tidal(nbx, precision, c["state"], c["points"], key=(precision, n, m, family))
        assert all(r[k].shape == (m,) for k in KEYS)
        check(r, c, precision, "points (n, m) = (%d, %d) %s" % (n, m, family))
    _record()


@pytest.mark.parametrize("n", R.BODY_SIZES)
@pytest.mark.parametrize("precision", [32, 64])
def test_bodies_mode_is_inside_the_gate_at_every_body_and_both_sides_of_every_seam(nbx, precision, n):
    for family in R.BODY_FAMILIES:
        c = R.body_case(precision, n, family)
        r = context_tidal(nbx, precision, c["state"], key=(precision, n, "bodies", family))
        assert all(r[k].shape == (n,) for k in KEYS)
        check(r, c, precision, "bodies n = %d %s" % (n, family))
        seams = [i for s in range(256, n, 256) for i in (s - 1, s)]  # tile seams; every second one a column seam
        if seams:
            assert float(R.k_metric(r, c["truth"], precision)[seams].max()) <= c["gate"]
        if n == 1:
            assert all(r[k][0] == 0 for k in KEYS)  # no partner: six exact zeros
    _record()


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("precision", [32, 64])
def test_bodies_mode_is_points_mode_at_the_bodies_minus_the_self_term(nbx, precision, n):
    """Points mode at x_i = bodies mode at i - G m_i / eps^3 delta_ab, within the two gates added, relative to A of points mode
    (which holds the self term: the larger of the two scales)."""
    cp, cb = R.case(precision, n, n, "own"), R.body_case(precision, n, "cloud")
    assert all(np.array_equal(cp["state"][f], cb["state"][f]) for f in K.FIELDS)
    rp = context_tidal(nbx, precision, cp["state"], cp["points"], key=(precision, n, n, "own"))
    rb = context_tidal(nbx, precision, cb["state"], key=(precision, n, "bodies", "cloud"))
    self_term = gm_as_uploaded(cb["state"]["mass"]) / EPS2 ** 1.5
    got = R.as_array(rb).astype(np.float64)
    got[:, R.DIAG] -= self_term[:, None]
    diff = np.abs(got - R.as_array(rp).astype(np.float64))
    bound = F.U[precision] * (cp["gate"] + cb["gate"]) * cp["truth"][2]
    print("fp%d n = %d: largest |difference| / bound %.3f" % (precision, n, float((diff / bound).max())))
    assert (diff <= bound).all()
    assert (np.abs(R.as_array(rb)[:, 0]) < 0.1 * self_term).any()  # the self term would have drowned these


@pytest.mark.parametrize("precision", [32, 64])
def test_the_trace_is_minus_three_eps2_times_the_fifth_power_sum(nbx, precision):
    for c, r in ((R.case(precision, 2049, 1025, "box"), None), (R.body_case(precision, 2049, "cloud"), None)):
        pts = None if c["bodies"] else c["points"]
        r = context_tidal(nbx, precision, c["state"], pts, key=(precision, 2049, "bodies", "cloud") if c["bodies"] else (precision, 2049, 1025, "box"))
        want = R.trace_truth(c["state"], c["points"], precision, bodies=c["bodies"])
        got = sum(r[k].astype(np.float64) for k in ("t_xx", "t_yy", "t_zz"))
        A = c["truth"][2][:, R.DIAG].sum(axis=1)
        assert (want <= 0).all() and (got <= 0).all()
        worst = float((np.abs(got - want) / (F.U[precision] * A)).max())
        print("fp%d %s: trace within %.2f u of A_xx + A_yy + A_zz (gate %.1f)" % (precision, "bodies" if c["bodies"] else "points", worst, c["gate"]))
        assert worst <= c["gate"]


# ---------------------------------------------------------------------------------------------------------------------------
# NULL outputs and the slack behind every array
# ---------------------------------------------------------------------------------------------------------------------------
def _t6(arrays):
    return (ctypes.c_void_p * 6)(*[None if a is None else a.ctypes.data for a in arrays])


@pytest.mark.parametrize("bodies", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_null_outputs_are_skipped_and_nothing_is_written_beyond_the_results(nbx, precision, bodies):
    n, m, slack = 257, 513, 16
    T = R.DTYPE[precision]
    L = nbx.load()
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    if bodies:
        c = R.body_case(precision, n, "cloud")
        full, count = context_tidal(nbx, precision, c["state"], key=(precision, n, "bodies", "cloud")), n
    else:
        c = R.case(precision, n, m, "box")
        full, count = context_tidal(nbx, precision, c["state"], c["points"], key=(precision, n, m, "box")), m
        pts = [np.concatenate([p, np.full(slack, np.nan, dtype=T)]) for p in c["points"]]  # what lies behind the points is not read
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        call = (lambda t: L.nbx_tidal_bodies(ctx._h, t)) if bodies else (lambda t: L.nbx_tidal(ctx._h, m, *[ptr(p) for p in pts], t))
        for pick in ([0, 1, 2, 3, 4, 5], [0], [4], [5], [1, 3], []):
            out = [np.full(count + slack, -7.25, dtype=T) for _ in range(6)]
            assert call(_t6([out[k] if k in pick else None for k in range(6)])) == nbx.NBX_OK, pick
            for k in range(6):
                assert (out[k][count:] == -7.25).all(), (pick, k)  # the slack
                if k in pick:
                    assert out[k][:count].tobytes() == full[KEYS[k]].tobytes(), (pick, k)
                else:
                    assert (out[k] == -7.25).all(), (pick, k)
        assert call(None) == nbx.NBX_ERR_ARG and L.nbx_last_error().decode().endswith(": t is NULL")
        if not bodies:
            out = np.full(4, -7.25, dtype=T)
            assert L.nbx_tidal(ctx._h, 0, None, None, None, _t6([out] * 6)) == nbx.NBX_OK and (out == -7.25).all()  # m == 0


# ---------------------------------------------------------------------------------------------------------------------------
# bit contracts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_a_sliced_context_gives_the_bits_of_the_whole_one_in_both_modes(nbx, precision):
    n, m = 2049, 1025
    c, cb = R.case(precision, n, m, "box"), R.body_case(precision, n, "cloud")
    whole = context_tidal(nbx, precision, c["state"], c["points"], key=(precision, n, m, "box"))
    whole_b = context_tidal(nbx, precision, cb["state"], key=(precision, n, "bodies", "cloud"))
    for sl in (dict(i_begin=1000, i_count=300), dict(i_begin=0, i_count=512, n_alloc=2304), dict(i_begin=2048, i_count=1)):
        with nbx.Context(n, precision, **sl) as ctx:
            ctx.upload(c["state"])
            assert same(ctx.tidal(*c["points"]), whole), sl
            got = ctx.tidal_bodies()
            assert got["t_xx"].shape == (n,) and same(got, whole_b), sl  # all n bodies


@pytest.mark.parametrize("precision", [32, 64])
def test_a_small_call_after_a_large_one_equals_a_fresh_objects(nbx, precision):
    n = 4097
    big, small = R.case(precision, n, 4097, "box"), R.case(precision, n, 2, "box")
    want_big = context_tidal(nbx, precision, big["state"], big["points"], key=(precision, n, 4097, "box"))
    want_small = context_tidal(nbx, precision, small["state"], small["points"], key=(precision, n, 2, "box"))
    want_bodies = context_tidal(nbx, precision, big["state"], key=(precision, n, "bodies", "cloud"))
    with nbx.Context(n, precision) as ctx:
        ctx.upload(small["state"])  # the same state in all three: a family's state depends on n alone
        assert same(ctx.tidal(*small["points"]), want_small)  # the buffers are allocated small ...
        assert same(ctx.tidal(*big["points"]), want_big)      # ... grow ...
        assert same(ctx.tidal(*small["points"]), want_small)  # ... and serve a small call again,
        assert same(ctx.tidal_bodies(), want_bodies)          # the other mode,
        assert same(ctx.tidal(*small["points"]), want_small)  # and a small call after it
    assert all(np.array_equal(big["state"][f], small["state"][f]) for f in K.FIELDS)


def _member_state(precision, n, k):
    return K.make_state(7000 + 13 * k + n, n, R.DTYPE[precision])


def _member_points(precision, state, m, k):
    return FR.make_points(precision, state, m, "box", seed=1 + k)


def _ranges(S):
    return [(0, S)] + [(k, 1) for k in range(S)] + [(1, S - 1)]


@pytest.mark.parametrize("n,m", [(257, 513), (2049, 1025)])
@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_have_the_bits_of_a_context_in_every_sub_range(nbx, precision, n, m):
    S = 5
    states = [_member_state(precision, n, k) for k in range(S)]
    pts = [_member_points(precision, s, m, k) for k, s in enumerate(states)]
    want = [context_tidal(nbx, precision, s, p) for s, p in zip(states, pts)]
    want_b = [context_tidal(nbx, precision, s) for s in states]
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        for first, count in _ranges(S):
            P = [np.stack([pts[k][c] for k in range(first, first + count)]) for c in range(3)]
            got, got_b = e.tidal(*P, first=first, count=count), e.tidal_bodies(first=first, count=count)
            assert all(got[key].shape == (count, m) and got_b[key].shape == (count, n) for key in KEYS)
            for j in range(count):
                assert same({key: got[key][j] for key in KEYS}, want[first + j]), (first, count, j)
                assert same({key: got_b[key][j] for key in KEYS}, want_b[first + j]), (first, count, j)


@pytest.mark.parametrize("m", [513, 3])
@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_have_the_bits_of_a_context_of_their_size_in_both_modes(nbx, precision, m):
    """m = 513: the member of 2049 bodies has two j splits, every other member one -- its second row of workgroups returns at once
    for the others.  Bodies mode: members of 1 to 5 columns and 1 or 2 splits in one grid."""
    sizes = FR.RAGGED_SIZES
    S = len(sizes)
    assert sorted(set(FR.field_shape(m, n)[2] for n in sizes)) == [1, 2]
    assert sorted(set(FR.field_shape(n, n)[0] for n in sizes)) == [1, 2, 5] and sorted(set(FR.field_shape(n, n)[2] for n in sizes)) == [1, 2]
    states = [_member_state(precision, n, k) for k, n in enumerate(sizes)]
    pts = [_member_points(precision, s, m, k) for k, s in enumerate(states)]
    want = [context_tidal(nbx, precision, s, p) for s, p in zip(states, pts)]
    want_b = [context_tidal(nbx, precision, s) for s in states]
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        for first, count in _ranges(S):
            P = [np.stack([pts[k][c] for k in range(first, first + count)]) for c in range(3)]
            got = r.tidal(*P, first=first, count=count)
            got_b = r.tidal_bodies(first=first, count=count)
            at = np.concatenate([[0], np.cumsum(sizes[first:first + count])]).astype(int)
            assert all(got_b[key].shape == (at[-1],) for key in KEYS)  # one array per key, the members end to end
            for j in range(count):
                assert same({key: got[key][j] for key in KEYS}, want[first + j]), (first, count, j)
                assert same({key: got_b[key][at[j]:at[j + 1]] for key in KEYS}, want_b[first + j]), (first, count, j)


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


def _both(o, P):
    """The results of both modes as one list of arrays."""
    a, b = o.tidal(*P), o.tidal_bodies()
    return [a[k] for k in KEYS] + [b[k] for k in KEYS]


def _bits(arrays):
    return [np.asarray(a).tobytes() for a in arrays]


@pytest.mark.parametrize("kind", ["context", "ensemble", "ragged"])
def test_the_calls_are_on_the_stream_and_leave_the_trajectory_every_counter_the_field_and_the_tracers_alone(nbx, kind):
    dt = 1.0 / 256
    o, states, P = _make(nbx, kind)
    tracers = ([0.5 * p for p in P], [0.1 * p for p in P])
    with o:
        o.upload(states)
        o.tracers_upload(*tracers)
        t0 = _both(o, P)
        o.profile(True)
        o.step(3, dt, kenergy=False)  # asynchronous: the calls describe the state after these steps
        t3 = _both(o, P)
        o.sync()
        before = o.stats()
        ke0 = o.step(0, dt)
        field = o.field(*P)
        tr = o.tracers_download()
        assert _bits(_both(o, P)) == _bits(t3)
        after = o.stats()
        assert before == after  # steps_done, every *_timed / *_ms_total field, graph replays: all of it
        assert np.array_equal(o.step(0, dt), ke0)  # the kinetic-energy partials
        again = o.field(*P)
        assert all(again[k].tobytes() == field[k].tobytes() for k in FR.KEYS)  # nbx_field's buffers are its own
        assert _crc(_flat(o.tracers_download())) == _crc(_flat(tr))  # the tracers' bits
        ke_a = o.step(3, dt)
        a = _flat(o.download())
        stats_a = o.stats()
    o, _, _ = _make(nbx, kind)
    with o:
        o.upload(states)
        o.step(3, dt)  # synchronises
        o.sync()
        assert _bits(_both(o, P)) == _bits(t3)  # stepped, synchronised and asked then
    o, _, _ = _make(nbx, kind)
    with o:  # an object that never made the calls
        o.upload(states)
        o.tracers_upload(*tracers)
        o.profile(True)
        o.step(3, dt, kenergy=False)
        o.sync()
        assert np.array_equal(o.step(0, dt), ke0) and np.array_equal(o.step(0, dt), ke0)  # twice, as above
        field_b = o.field(*P)
        assert all(field_b[k].tobytes() == field[k].tobytes() for k in FR.KEYS)
        assert _crc(_flat(o.tracers_download())) == _crc(_flat(tr))
        ke_b = o.step(3, dt)
        b = _flat(o.download())
        stats_b = o.stats()
    assert _crc(a) == _crc(b) and np.array_equal(ke_a, ke_b)
    timing = ("force_ms_total", "step_ms_total")  # measured times differ from run to run; the counts do not
    assert {k: v for k, v in stats_a.items() if k not in timing} == {k: v for k, v in stats_b.items() if k not in timing}
    assert _bits(t0) != _bits(t3)


# ---------------------------------------------------------------------------------------------------------------------------
# state and argument errors on real objects, in the header's order
# ---------------------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors_come_in_the_headers_order(nbx):
    sizes = (300, 5, 1000, 64)
    states = [K.make_state(60 + k, n, np.float32) for k, n in enumerate(sizes)]
    p = _member_points(32, states[0], 7, 0)
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with nbx.Context(300, 32) as c:
        for call, name in ((lambda: c.tidal(*p), "nbx_tidal"), (lambda: c.tidal_bodies(), "nbx_tidal_bodies")):
            with pytest.raises(nbx.NbxError) as e:
                call()
            assert e.value.code == nbx.NBX_ERR_STATE and (name + ": nbx_upload has not been called") in str(e.value)
        # t NULL and the size bound come before the state
        assert L.nbx_tidal(c._h, 7, *[ptr(a) for a in p], None) == nbx.NBX_ERR_ARG and err() == "nbx_tidal: t is NULL"
        assert L.nbx_tidal_bodies(c._h, None) == nbx.NBX_ERR_ARG and err() == "nbx_tidal_bodies: t is NULL"
        out = np.full(8, -7.25, dtype=np.float32)
        assert L.nbx_tidal(c._h, (1 << 21) + 1, *[ptr(a) for a in p], _t6([out] * 6)) == nbx.NBX_ERR_ARG and err() == "nbx_tidal: m exceeds 2097152"
        c.upload(states[0])
        assert c.tidal(*p)["t_zz"].shape == (7,) and c.tidal_bodies()["t_zz"].shape == (300,)
        c.step_local(1.0 / 256)
        for call, name in ((lambda: c.tidal(*p), "nbx_tidal"), (lambda: c.tidal_bodies(), "nbx_tidal_bodies")):
            with pytest.raises(nbx.NbxError) as e:
                call()
            assert e.value.code == nbx.NBX_ERR_STATE and (name + ": a local step awaits nbx_commit") in str(e.value)
        assert (out == -7.25).all()
    for make, prefix in ((lambda: nbx.Ragged(sizes, 32), "nbx_ragged"), (lambda: nbx.Ensemble(300, 4, 32), "nbx_ensemble")):
        st = states if "ragged" in prefix else [K.make_state(70 + k, 300, np.float32) for k in range(4)]
        S = 4
        P = lambda count: [np.stack([p[c]] * count) if count > 0 else np.zeros((0, 7), dtype=np.float32) for c in range(3)]
        with make() as o:
            for call, name in ((lambda: o.tidal(*P(4)), prefix + "_tidal"), (lambda: o.tidal_bodies(), prefix + "_tidal_bodies")):
                with pytest.raises(nbx.NbxError) as e:
                    call()
                assert e.value.code == nbx.NBX_ERR_STATE and (name + ": member 0 has not been uploaded") in str(e.value)
            o.upload(st[:3])
            for first, count in ((0, 4), (2, 2), (3, 1)):
                for call in (lambda: o.tidal(*P(count), first=first, count=count), lambda: o.tidal_bodies(first=first, count=count)):
                    with pytest.raises(nbx.NbxError) as e:
                        call()
                    assert e.value.code == nbx.NBX_ERR_STATE and "member 3 has not been uploaded" in str(e.value), (first, count)
            part, part_b = o.tidal(*P(3), first=0, count=3), o.tidal_bodies(first=0, count=3)  # before the others arrive
            assert part["t_xx"].shape == (3, 7)
            f, fb = getattr(L, prefix + "_tidal"), getattr(L, prefix + "_tidal_bodies")
            q = P(4)
            out = np.full(4, -7.25, dtype=np.float32)
            t = _t6([out] + [None] * 5)
            for first, count in ((-1, 1), (0, S + 1), (S, 1), (0, -1), (S + 1, 0)):
                assert f(o._h, first, count, 7, *[ptr(a) for a in q], t) == nbx.NBX_ERR_ARG, (first, count)
                assert fb(o._h, first, count, t) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == prefix + "_tidal_bodies: members [first, first + count) are outside [0, members)"
            # t NULL before the range, the range before the size, the size before the arrays are read
            assert f(o._h, -1, 1, 7, *[ptr(a) for a in q], None) == nbx.NBX_ERR_ARG and err() == prefix + "_tidal: t is NULL"
            assert fb(o._h, -1, 1, None) == nbx.NBX_ERR_ARG and err() == prefix + "_tidal_bodies: t is NULL"
            assert f(o._h, 0, 3, (1 << 21) // 3 + 1, *[ptr(a) for a in q], t) == nbx.NBX_ERR_ARG
            assert err() == prefix + "_tidal: count * m exceeds 2097152"
            assert f(o._h, 1, 0, 7, *[ptr(a) for a in q], _t6([out] * 6)) == nbx.NBX_OK and fb(o._h, 1, 0, _t6([out] * 6)) == nbx.NBX_OK  # count == 0
            assert (out == -7.25).all()
            o.upload(st[3:], first=3)
            assert same(o.tidal(*P(3), first=0, count=3), part) and same(o.tidal_bodies(first=0, count=3), part_b)


# ---------------------------------------------------------------------------------------------------------------------------
# large launch shapes
# ---------------------------------------------------------------------------------------------------------------------------
def _sample(m, shape, count=1000):
    """All m points where m <= count; else the first and last, both sides of every column seam (and the lane's second point
    there) and of every split seam, and seeded random ones up to `count`."""
    if m <= count:
        return np.arange(m)
    columns, tiles, splits, per = shape
    s = {0, m - 1}
    for c in range(1, columns):
        s.update((c * 512 - 257, c * 512 - 256, c * 512 - 1, c * 512))
    for k in range(1, splits):
        s.update((k * per * 256 - 1, k * per * 256))
    rng = np.random.default_rng([17, m])
    while len(s) < count:
        s.add(int(rng.integers(0, m)))
    return np.array(sorted(i for i in s if 0 <= i < m), dtype=np.int64)


def _large_case(precision, state, points, bodies, shape):
    m = len(state["mass"]) if bodies else len(points[0])
    rows = _sample(m, shape)
    tr = R.truth(state, points, precision, bodies=bodies, rows=rows)
    pick = np.unique(np.linspace(0, len(rows) - 1, 32).astype(np.int64))  # K_ref on 32 of the rows: a sequential sum is O(n) each
    kref = float(R.k_metric(R.sequential(state, points, precision, bodies=bodies, rows=rows[pick]), tuple(v[pick] for v in tr), precision).max())
    return {"state": state, "points": points, "rows": rows, "truth": tr, "kref": kref, "gate": R.gate(kref, precision), "bodies": bodies}


@pytest.mark.parametrize("precision", [32, 64])
def test_points_mode_at_one_column_of_206_splits(nbx, precision):
    m, n = 300, 262657
    shape = FR.field_shape(m, n)
    assert shape == (1, 1027, 206, 5)
    state = FR.make_state(precision, n, "box")
    c = _large_case(precision, state, FR.make_points(precision, state, m, "box"), False, shape)
    r = context_tidal(nbx, precision, state, c["points"])
    assert len(c["rows"]) == m
    check(r, c, precision, "points (n, m) = (%d, %d) box, %d splits" % (n, m, shape[2]), rows=c["rows"])
    _record()


@pytest.mark.parametrize("precision", [32, 64])
def test_bodies_mode_on_the_lattice_of_71_columns_and_15_splits(nbx, precision):
    n = 33 ** 3
    shape = FR.field_shape(n, n)
    assert n == 35937 and shape == (71, 141, 15, 10)
    state = LR.state(33, precision, at_rest=True)
    c = _large_case(precision, state, None, True, shape)
    r = context_tidal(nbx, precision, state)
    assert len(c["rows"]) >= 1000 and {511, 512, 2559, 2560}.issubset(set(c["rows"].tolist()))  # a column seam and a split seam
    check(r, c, precision, "bodies lattice n = %d, %d columns x %d splits" % (n, shape[0], shape[2]), rows=c["rows"])
    _record()


# ---------------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_batch_call_costs_no_more_than_the_context_calls_it_replaces(nbx):
    """fp32, in this process, rounds alternated, medians (tools/tidal_cost.py): one nbx_ensemble_tidal call over 16 x 2048
    (m = 2048) and one nbx_ragged_tidal call over 16 sizes 512 ... 4096 (m = 1024) against 16 nbx_tidal calls on contexts created
    and uploaded beforehand: 16 uploads, 32 launches, 16 synchronisations against 1, 2 and 1, so ratio <= 1.0, the condition the
    sibling features use, both arms returning the same bits.  nbx_tidal against nbx_field at n = m = 131072 is recorded, not
    gated."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tidal_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = cells[kind] = tidal_cost.measure(nbx, kind)
        print("%s fp32 m = %d: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["m"], r["batch_us"], r["contexts_us"], r["ratio"]))
    r = cells["context_n%d" % tidal_cost.LARGE_N] = tidal_cost.measure_large(nbx)
    print("context fp32 n = m = %d: tidal %.1f us, field %.1f us, time ratio %.2f (packed VALU 20 / 13 = 1.54)"
          % (r["n"], r["tidal_us"], r["field_us"], r["time_ratio"]))
    tidal_cost.write(tidal_cost.OUT, cells)
    for kind in ("ensemble", "ragged"):
        r = cells[kind]
        assert r["members"] == 16 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"], r["m"]) == ((2048, 2048, 2048) if kind == "ensemble" else (512, 4096, 1024))
        assert r["ratio"] <= 1.0, (kind, r["ratio"])
