"""Velocity-only half steps on the device (include/nbx_kick.h): the kicked velocities must be v + fl(a * h) bit for bit with a the
object's own accel call, positions untouched, for every one-launch instance and for the other context shapes; members of an
ensemble, of a ragged ensemble and one-launch contexts must agree bit for bit; the energy must be the bits a step call of no
steps then reports; the counters, the profile and the trajectory of further steps must not see a kick; the two half kicks must
make stepping second order in the energy the diagnostics read out and time reversible, on the systems of tests/kick_ref.py whose
numpy restatement passes the same gates (tests/test_kick_cpu.py); groups; the documented errors; and one kick must cost no more
than the round trip through the host it replaces.

Figures measured on an MI355X are in the docstrings of the tests that gate them."""
import os
import sys

import numpy as np
import pytest

import kick_ref as K
from conftest import ROOT

pytestmark = pytest.mark.gpu

POS = ("pos_x", "pos_y", "pos_z")
VEL = ("vel_x", "vel_y", "vel_z")
MEMBERS = 3
# n = 1: one body (every other body of its wave shadows it); 63: a partial wave; 257 (n_alloc 512, 8 records per lane): one whole
# trip of the hand-scheduled loop; 600 (n_alloc 768, 12 records per lane): a whole trip plus the compiled 4-record remainder
SIZES = (1, 63, 257, 600)
KICKS = (0.05, -0.05, 0.1)

OPTIONS = ([(32, dict(bodies_per_lane=NB, inner_loop="LOOP_CXX")) for NB in (2, 4, 8, 16)] +
           [(32, dict(bodies_per_lane=NB, inner_loop="LOOP_ASM")) for NB in (2, 4, 8)] +
           [(64, dict(bodies_per_lane=NB)) for NB in (2, 4, 8)])
OPTION_IDS = ["f%d-%s" % (p, "-".join(str(v).replace("LOOP_", "").lower() for v in o.values())) for p, o in OPTIONS]


def _opts(nbx, opts):
    return {k: (getattr(nbx, v) if isinstance(v, str) else v) for k, v in opts.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def member_states(nbx, n, precision, members=MEMBERS):
    """`members` different systems of n bodies: consecutive slices of the seed-42 system of members * n bodies."""
    big = nbx.initial_conditions(members * n, precision)
    return [{f: big[f][m * n:(m + 1) * n].copy() for f in nbx.FIELDS} for m in range(members)]


def kicked(v, a, h):
    """v + fl(a * h) in the arrays' precision: numpy rounds the product and the sum separately."""
    T = v.dtype.type
    return v + a * T(h)


class Members:
    """An ensemble, a ragged ensemble or a list of contexts behind one per-member view: download() -> list of dicts,
    accel() -> list of [ax, ay, az]."""

    def __init__(self, nbx, obj):
        self.nbx, self.o = nbx, obj

    def download(self):
        d = self.o.download()
        if isinstance(self.o, self.nbx.Ensemble):
            return [{f: d[f][m] for f in d} for m in range(self.o.members)]
        return d if isinstance(d, list) else [d]

    def accel(self):
        a = self.o.accel()
        if isinstance(self.o, self.nbx.Ensemble):
            return [[c[m] for c in a] for m in range(self.o.members)]
        return a if isinstance(self.o, self.nbx.Ragged) else [a]


def kick_and_check(view, h, own=None, label=""):
    """One kick of view.o: velocities become v + fl(a * h) with a from the object's own accel call, positions keep their bits.
    own = (i_begin, i_count) of a context that owns a slice.  Returns the state after the kick."""
    acc, before = view.accel(), view.download()
    view.o.kick(h)
    after = view.download()
    for m, (a, s0, s1) in enumerate(zip(acc, before, after)):
        sl = slice(None) if own is None else slice(own[0], own[0] + own[1])
        for f, c in zip(VEL, a):
            assert same_bits(s1[f][sl], kicked(s0[f][sl], c[sl], h)), (label, m, f, h)
        for f in POS:
            assert same_bits(s1[f], s0[f]), (label, m, f, h)
    return after


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bits, every one-launch instance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,opts", OPTIONS, ids=OPTION_IDS)
def test_kicked_velocities_are_v_plus_a_h_and_members_equal_ragged_members_and_contexts(nbx, precision, opts):
    o = _opts(nbx, opts)
    states = {n: member_states(nbx, n, precision) for n in SIZES}
    final = {}
    with nbx.Ragged([n for n in SIZES for _ in range(MEMBERS)], precision, **o) as r:
        st = r.stats()
        assert all(st[k] == v for k, v in o.items()), st
        NB, loop = st["bodies_per_lane"], st["inner_loop"]
        r.upload([s for n in SIZES for s in states[n]])
        view = Members(nbx, r)
        for h in KICKS:
            out = kick_and_check(view, h, label="ragged")
        final["ragged"] = {n: out[i * MEMBERS:(i + 1) * MEMBERS] for i, n in enumerate(SIZES)}
    moved = 0.0
    for n in SIZES:
        with nbx.Ensemble(n, MEMBERS, precision, **o) as e:
            st = e.stats()
            assert (st["bodies_per_lane"], st["inner_loop"]) == (NB, loop) and st["n_alloc"] == -(-n // 256) * 256
            e.upload(states[n])
            view = Members(nbx, e)
            for h in KICKS:
                out = kick_and_check(view, h, label="ensemble n=%d" % n)
        for m in range(MEMBERS):
            with nbx.Context(n, precision, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
                cs = c.stats()
                assert cs["kernel_variant"] == nbx.KERNEL_JLANE and (cs["bodies_per_lane"], cs["inner_loop"]) == (NB, loop)
                c.upload(states[n][m])
                view = Members(nbx, c)
                for h in KICKS:
                    ctx = kick_and_check(view, h, label="context n=%d" % n)[0]
            for f in POS + VEL:
                assert same_bits(out[m][f], ctx[f]), ("ensemble / context", n, m, f)
                assert same_bits(out[m][f], final["ragged"][n][m][f]), ("ensemble / ragged", n, m, f)
            moved = max(moved, max(float(np.abs(out[m][f] - states[n][m][f]).max()) for f in VEL))
    assert moved > 0  # not a no-op against a no-op


# ---------------------------------------------------------------------------------------------------------------------------
# 2. contexts of the other shapes
# ---------------------------------------------------------------------------------------------------------------------------
# (label, precision, smallest legal n, options, what stats() must then say).  Two j-splits of the LDS kernel take two tiles of
# 256 records: n = 257; every other shape exists for one body.  Each shape also runs at 300 bodies -- more than one workgroup of
# kick_kernel, and accelerations that are not zero.
SHAPES = [
    ("sgprw", 32, 1, dict(kernel_variant="KERNEL_SGPRW"), dict(kernel_variant="KERNEL_SGPRW")),
    ("lds-2-splits", 32, 257, dict(kernel_variant="KERNEL_LDS", j_split=2), dict(kernel_variant="KERNEL_LDS", j_split=2)),
    ("sgpr-reference-order", 32, 1, dict(kernel_variant="KERNEL_SGPR", summation_order="ORDER_REFERENCE"),
     dict(kernel_variant="KERNEL_SGPR", summation_order="ORDER_REFERENCE")),
    ("exact", 32, 1, dict(kernel_variant="KERNEL_EXACT"), dict(kernel_variant="KERNEL_EXACT")),
    ("fp64-default", 64, 1, dict(), dict()),
    ("fp64-sgprw-2-splits", 64, 1, dict(kernel_variant="KERNEL_SGPRW", j_split=2), dict(kernel_variant="KERNEL_SGPRW")),
]


@pytest.mark.parametrize("label,precision,n_min,opts,want", SHAPES, ids=[s[0] for s in SHAPES])
def test_contexts_of_the_other_shapes(nbx, label, precision, n_min, opts, want):
    for n in (n_min, 300):
        state = member_states(nbx, n, precision, 2)[1]
        with nbx.Context(n, precision, **_opts(nbx, opts)) as c:
            st = c.stats()
            assert all(st[k] == v for k, v in _opts(nbx, want).items()), st
            c.upload(state)
            view = Members(nbx, c)
            for h in KICKS:
                out = kick_and_check(view, h, label="%s n=%d" % (label, n))[0]
            assert c.kick(0.05, kenergy=True) == c.step(0)
        if n > 1:
            assert max(float(np.abs(out[f] - state[f]).max()) for f in VEL) > 0


@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_that_owns_a_slice_kicks_only_that_slice(nbx, precision):
    n, i_begin, i_count = 600, 256, 256
    state = member_states(nbx, n, precision, 1)[0]
    with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count) as c:
        c.upload(state)
        view = Members(nbx, c)
        for h in KICKS:
            out = kick_and_check(view, h, own=(i_begin, i_count), label="slice")[0]
        outside = np.r_[0:i_begin, i_begin + i_count:n]
        for f in VEL:
            assert not out[f][outside].any(), f  # download reports the owned velocities only: nothing appeared elsewhere
            assert np.abs(out[f][i_begin:i_begin + i_count] - state[f][i_begin:i_begin + i_count]).max() > 0
        # the energy is the slice's
        T = state["mass"].dtype.type
        sl = slice(i_begin, i_begin + i_count)
        ke = c.kick(0.0, kenergy=True)
        terms = state["mass"][sl] * ((out["vel_x"][sl] * out["vel_x"][sl] + out["vel_y"][sl] * out["vel_y"][sl]) + out["vel_z"][sl] * out["vel_z"][sl])
        assert terms.dtype.type is T and abs(ke - 0.5 * float(terms.astype(np.float64).sum())) <= 1e-13 * ke


# ---------------------------------------------------------------------------------------------------------------------------
# 3. energy
# ---------------------------------------------------------------------------------------------------------------------------
def numpy_kenergy(state, mass):
    """0.5 * sum of the terms m * ((vx^2 + vy^2) + vz^2), each in the state's precision as the kernels evaluate it, added in fp64."""
    vx, vy, vz = (state[f] for f in VEL)
    terms = mass * ((vx * vx + vy * vy) + vz * vz)
    assert terms.dtype == mass.dtype
    return 0.5 * float(terms.astype(np.float64).sum())


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("kind", ["ensemble", "ragged", "context", "context-slabs"])
def test_the_energy_is_what_a_step_of_no_steps_reports_and_the_sum_of_the_same_terms(nbx, kind, precision):
    sizes = list(SIZES) if kind == "ragged" else [600] * (MEMBERS if kind == "ensemble" else 1)
    states = [member_states(nbx, n, precision, k + 1)[k] for k, n in enumerate(sizes)]
    obj = {"ensemble": lambda: nbx.Ensemble(600, MEMBERS, precision), "ragged": lambda: nbx.Ragged(sizes, precision),
           "context": lambda: nbx.Context(600, precision), "context-slabs": lambda: nbx.Context(600, precision, kernel_variant=nbx.KERNEL_SGPRW, j_split=2)}[kind]()
    with obj:
        obj.upload(states if kind in ("ensemble", "ragged") else states[0])
        view = Members(nbx, obj)
        assert np.all(np.asarray(obj.step(0)) == 0)  # nothing has written partials yet
        for h in (0.05, -0.1):
            ke = np.atleast_1d(obj.kick(h, kenergy=True))
            again = np.atleast_1d(obj.step(0))
            assert same_bits(ke, again), (h, ke, again)
            out = view.download()
            for m, s in enumerate(out):
                want = numpy_kenergy(s, states[m]["mass"])
                print("%s f%d member %d h %+.2f: kenergy %.17g, numpy %.17g, relative difference %.2e" % (kind, precision, m, h, ke[m], want, abs(ke[m] - want) / want))
                assert abs(ke[m] - want) <= 1e-13 * want, (m, h, ke[m], want)
        obj.step(2, kenergy=False)
        assert not same_bits(np.atleast_1d(obj.step(0)), ke)  # a step's partials replace the kick's
        obj.kick(0.05)                                          # without the energy: the partials are written all the same
        out = view.download()
        ke = np.atleast_1d(obj.step(0))
        for m, s in enumerate(out):
            want = numpy_kenergy(s, states[m]["mass"])
            assert abs(ke[m] - want) <= 1e-13 * want, (m, ke[m], want)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. no side effects
# ---------------------------------------------------------------------------------------------------------------------------
def make(nbx, kind, precision):
    if kind == "ensemble":
        return nbx.Ensemble(600, MEMBERS, precision), [600] * MEMBERS
    if kind == "ragged":
        return nbx.Ragged(SIZES, precision), list(SIZES)
    if kind == "context-graph":
        return nbx.Context(600, precision, use_graph=1), [600]
    return nbx.Context(600, precision, kernel_variant=nbx.KERNEL_SGPRW, j_split=2, use_graph=2), [600]


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("kind", ["ensemble", "ragged", "context-graph", "context-slabs"])
def test_a_kick_is_no_step_and_steps_after_it_are_those_of_an_upload_of_the_kicked_state(nbx, kind, precision):
    a, sizes = make(nbx, kind, precision)
    b, _ = make(nbx, kind, precision)
    batch = kind in ("ensemble", "ragged")
    states = [member_states(nbx, n, precision, k + 1)[k] for k, n in enumerate(sizes)]
    with a, b:
        a.upload(states if batch else states[0])
        a.profile(True)
        a.step(3, kenergy=False)                       # an odd number: the current buffer is the second one
        before = a.stats()
        assert before["steps_done"] == 3
        a.kick(0.05)
        a.kick(-0.02, kenergy=True)
        after = a.stats()
        assert after == before, (before, after)        # steps_done, launches_timed, *_ms_total, graph_replays: every field
        assert before["force_launches_timed" if not batch else "launches_timed"] == 3
        a.profile(False)
        # h = 0: the velocities compare equal, the positions keep their bits
        view = Members(nbx, a)
        s0 = view.download()
        a.kick(0.0)
        s1 = view.download()
        for x, y in zip(s0, s1):
            assert all(np.array_equal(x[f], y[f]) for f in VEL) and all(same_bits(x[f], y[f]) for f in POS)
        # kick; step(k) against upload(kicked state); step(k), k = 3 -- and 6, which a graph context replays as one captured window
        a.kick(0.05)
        for k in (3, 6):
            kicked_state = view.download()
            for s, s_in in zip(kicked_state, states):
                s["mass"] = s_in["mass"]
            b.upload(kicked_state if batch else kicked_state[0])
            ke_a, ke_b = a.step(k), b.step(k)
            assert same_bits(np.atleast_1d(ke_a), np.atleast_1d(ke_b)), (k, ke_a, ke_b)
            for x, y in zip(view.download(), Members(nbx, b).download()):
                assert all(same_bits(x[f], y[f]) for f in POS + VEL), k
            a.kick(-0.05)
        if kind == "context-graph":
            assert a.stats()["graph_replays"] == b.stats()["graph_replays"] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# 5. second order, 6. reversibility -- on the systems of kick_ref.py
# ---------------------------------------------------------------------------------------------------------------------------
def ref_states(precision):
    return [K.make_state(seed, dtype=np.float32 if precision == 32 else np.float64) for seed in K.SEEDS]


def energy_errors(obj, batch, states, inv_dt, leap):
    """|E(T) - E(0)| / |E(0)| per member; E = kenergy + potential of the object's diagnostics call."""
    obj.upload(states if batch else states[0])
    e0 = np.array([d["etotal"] for d in (obj.diagnostics() if batch else [obj.diagnostics()])])
    nsteps = int(round(K.T_END * inv_dt))
    (obj.leapfrog if leap else obj.step)(nsteps, 1.0 / inv_dt, kenergy=False)
    e1 = np.array([d["etotal"] for d in (obj.diagnostics() if batch else [obj.diagnostics()])])
    return np.abs(e1 - e0) / np.abs(e0)


ORDER_CASES = [("ensemble", 64), ("context", 64), ("ensemble", 32), ("ragged", 32)]


@pytest.mark.parametrize("kind,precision", ORDER_CASES, ids=["%s-f%d" % c for c in ORDER_CASES])
def test_the_half_kicks_make_the_energy_error_second_order(nbx, kind, precision):
    """n = 96, three members (the three systems of kick_ref.py), T = 0.5.  Plain stepping: ratio of the errors at dt = 1/64 and
    1/128 in [1.8, 2.2]; leapfrog: in [3.5, 4.5] (fp32: [3.3, 4.7]) and, in fp64, at most 1/20 of the plain error at 1/64.
    Measured: plain 1.973 / 1.986 / 1.989 in both precisions; leapfrog 4.000 / 3.966 / 4.038 in fp64 (errors 127 / 110 / 119
    times smaller than plain at 1/64), 4.052 / 3.905 / 4.081 in fp32 -- the restatement's figures to three digits."""
    states = ref_states(precision)
    batch = kind != "context"
    obj = {"ensemble": lambda: nbx.Ensemble(K.N, 3, precision), "ragged": lambda: nbx.Ragged([K.N] * 3, precision),
           "context": lambda: nbx.Context(K.N, precision)}[kind]()
    with obj:
        err = {(leap, inv): energy_errors(obj, batch, states, inv, leap) for leap in (False, True) for inv in (64, 128)}
    lo, hi = (3.5, 4.5) if precision == 64 else (3.3, 4.7)
    for m in range(len(err[True, 64])):
        plain, leap = err[False, 64][m] / err[False, 128][m], err[True, 64][m] / err[True, 128][m]
        print("%s f%d seed %d: plain %.3e %.3e ratio %.3f; leapfrog %.3e %.3e ratio %.3f; plain / leapfrog at 1/64: %.1f" % (
            kind, precision, K.SEEDS[m], err[False, 64][m], err[False, 128][m], plain, err[True, 64][m], err[True, 128][m], leap,
            err[False, 64][m] / err[True, 64][m]))
    for m in range(len(err[True, 64])):
        plain, leap = err[False, 64][m] / err[False, 128][m], err[True, 64][m] / err[True, 128][m]
        assert 1.8 <= plain <= 2.2, (m, plain)
        assert lo <= leap <= hi, (m, leap)
        if precision == 64:
            assert err[True, 64][m] <= err[False, 64][m] / 20, (m, err[True, 64][m], err[False, 64][m])


REVERSE_CASES = [("context", 64), ("ensemble", 64), ("context", 32), ("ensemble", 32), ("ragged", 32)]


@pytest.mark.parametrize("kind,precision", REVERSE_CASES, ids=["%s-f%d" % c for c in REVERSE_CASES])
def test_leapfrog_there_and_back_returns_to_the_start_and_plain_stepping_does_not(nbx, kind, precision):
    """leapfrog(32, 1/64) then leapfrog(32, -1/64): max |state - start| <= 1e-10 in fp64, <= 1e-4 in fp32; the same with plain
    steps: > 1e-3.  Measured: leapfrog 1.1 ... 3.1e-15 in fp64, 3.0 ... 9.4e-7 in fp32; plain 0.058 ... 0.166."""
    states = ref_states(precision)
    batch = kind != "context"
    obj = {"ensemble": lambda: nbx.Ensemble(K.N, 3, precision), "ragged": lambda: nbx.Ragged([K.N] * 3, precision),
           "context": lambda: nbx.Context(K.N, precision)}[kind]()
    N, dt = 32, 1.0 / 64
    dev = {}
    with obj:
        view = Members(nbx, obj)
        for leap in (True, False):
            obj.upload(states if batch else states[0])
            run = obj.leapfrog if leap else obj.step
            run(N, dt, kenergy=False)
            run(N, -dt, kenergy=False)
            dev[leap] = [max(float(np.abs(s[f].astype(np.float64) - s0[f].astype(np.float64)).max()) for f in POS + VEL)
                         for s, s0 in zip(view.download(), states)]
    print("%s f%d there and back: leapfrog %s, plain %s" % (kind, precision, ["%.2e" % d for d in dev[True]], ["%.2e" % d for d in dev[False]]))
    assert max(dev[True]) <= (1e-10 if precision == 64 else 1e-4), dev[True]
    assert min(dev[False]) > 1e-3, dev[False]


# ---------------------------------------------------------------------------------------------------------------------------
# 7. groups
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_group_of_four_logical_ranks_kicks_as_one_context(nbx):
    n = 1024
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, summation_order=nbx.ORDER_REFERENCE) as c, \
            nbx.Group(n, 32, n_ranks=4, devices=[0] * 4, summation_order=nbx.ORDER_REFERENCE) as g:
        assert g.info(0)[0] == 4 and g.info(3)[2]["i_count"] == 256 and g.info(3)[2]["summation_order"] == nbx.ORDER_REFERENCE
        c.upload(ic)
        g.upload(ic)
        for h in KICKS:
            assert c.kick(h) is None and g.kick(h) is None
            sc, sg = c.download(), g.download()
            assert all(same_bits(sc[f], sg[f]) for f in POS + VEL), h
        assert max(float(np.abs(sc[f] - ic[f]).max()) for f in VEL) > 0 and all(same_bits(sc[f], ic[f]) for f in POS)
        kc, kg = c.kick(0.05, kenergy=True), g.kick(0.05, kenergy=True)
        assert kc > 0 and abs(kc - kg) <= 1e-13 * kc, (kc, kg)
        assert g.step(0) == kg
        kc, kg = c.leapfrog(5, 1.0 / 64), g.leapfrog(5, 1.0 / 64)
        sc, sg = c.download(), g.download()
        assert all(same_bits(sc[f], sg[f]) for f in POS + VEL)
        assert abs(kc - kg) <= 1e-13 * kc, (kc, kg)
        assert g.info(0)[2]["steps_done"] == 5 == c.stats()["steps_done"]


def test_a_rank_group_of_one_kicks_as_one_context_and_gathers_the_energy(nbx):
    """The one-process-per-GPU form, as far as one GPU reaches: a world of one.  The energy goes through the all-gather that
    nbx_group_step uses."""
    n = 1024
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, use_graph=2) as c:
        c.upload(ic)
        want = [c.kick(0.05, kenergy=True), c.leapfrog(3, 1.0 / 64)]
        sc = c.download()
    with nbx.Group(n, 32, n_ranks=1, rank=0, unique_id=nbx.unique_id(), device=0) as g:
        g.upload(ic)
        got = [g.kick(0.05, kenergy=True), g.leapfrog(3, 1.0 / 64)]
        assert g.step(0) == got[1]
        sg = g.download()
    assert got == want and want[0] > 0, (got, want)  # one rank: the same partials through the same reduce
    assert all(same_bits(sc[f], sg[f]) for f in POS + VEL)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. errors on a device
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_objects_usable(nbx):
    states = member_states(nbx, 63, 32)
    with nbx.Context(63, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.kick(0.05)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_kick: nbx_upload has not been called" in str(err.value)
        with pytest.raises(nbx.NbxError) as err:
            c.kick(float("nan"))                     # the kick size before the state
        assert err.value.code == nbx.NBX_ERR_ARG and "nbx_kick: h is not finite" in str(err.value)
        c.upload(states[0])
        c.step_local(0.05)
        v0 = c.download()
        with pytest.raises(nbx.NbxError) as err:
            c.kick(0.05)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_kick: a local step awaits nbx_commit" in str(err.value)
        assert all(same_bits(v0[f], c.download()[f]) for f in VEL)
        c.commit()
        kick_and_check(Members(nbx, c), 0.05, label="after the errors")
    for obj, name in ((nbx.Ensemble(63, MEMBERS, 32), "nbx_ensemble_kick"), (nbx.Ragged([63] * MEMBERS, 32), "nbx_ragged_kick")):
        with obj:
            with pytest.raises(nbx.NbxError) as err:
                obj.kick(0.05)
            assert err.value.code == nbx.NBX_ERR_STATE and name + ": member 0 has not been uploaded" in str(err.value), str(err.value)
            obj.upload(states[:1])
            obj.upload(states[2:], first=2)           # member 1 is missing
            for ke in (False, True):
                with pytest.raises(nbx.NbxError) as err:
                    obj.kick(0.05, kenergy=ke)
                assert err.value.code == nbx.NBX_ERR_STATE and name + ": member 1 has not been uploaded" in str(err.value), str(err.value)
            with pytest.raises(nbx.NbxError) as err:
                obj.kick(float("inf"))
            assert err.value.code == nbx.NBX_ERR_ARG and name + ": h is not finite" in str(err.value)
            obj.upload(states[1:2], first=1)
            kick_and_check(Members(nbx, obj), 0.05, label=name)
    with nbx.Group(1024, 32, n_ranks=2, devices=[0, 0]) as g:
        with pytest.raises(nbx.NbxError) as err:
            g.kick(0.05)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_group_kick: nbx_group_upload has not been called" in str(err.value)
        g.upload(nbx.initial_conditions(1024))
        assert g.kick(0.05, kenergy=True) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------------
def _cost_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kick_cost
    return kick_cost


@pytest.mark.parametrize("population", ["ensemble", "ragged"])
def test_one_kick_costs_no_more_than_the_round_trip_through_the_host(nbx, population):
    """fp32, 16 x 2048 as an ensemble and 16 sizes spread evenly over 512 ... 4096 as a ragged ensemble: one kick call and a
    synchronisation against accel of all members, download, host update and upload (tools/kick_cost.py).  The kick saves a
    read-back, an upload and two synchronisations: ratio <= 1.0.  The kick-to-step ratio is printed, not gated.  Measured: 31.3 us
    against 337.7 (0.093) and 42.8 against 561.0 (0.076); one step launch 30.9 and 43.4 us (kick / step 1.01 and 0.99)."""
    tool = _cost_tool()
    r = (tool.measure_gate_ensemble if population == "ensemble" else tool.measure_gate_ragged)(nbx)
    print("%s fp32: kick %.1f us, host round trip %.1f us, ratio %.3f; one step launch %.1f us, kick / step %.3f" % (
        r["population"], r["kick_us"], r["host_round_trip_us"], r["ratio"], r["step_us"], r["kick_to_step"]))
    assert r["members"] == 16 and r["arms_agree_to_rounding"], r
    assert (r["n_min"], r["n_max"]) == ((2048, 2048) if population == "ensemble" else (512, 4096))
    assert r["ratio"] <= 1.0, r
