"""The moving probe: every step kernel, per body, with moving bodies and at time steps other than the reference's (float)0.1.

The step probe (tests/test_step_probe_gpu.py) starts from rest, so that v1 = fl(a dt) shows the acceleration -- and hides the
velocity a kernel reads -- and, like every other test of the suite, it steps at (float)0.1.  Here each case makes two runs from
the same positions and masses at a time step dt that is not 0.1:

  rest run     v0 = 0, one step: K of v1R / dt stays under the step probe's gate 2 max(K_ref, 16) (force_ref; K_ref is the CPU
               oracle's K on the same state and bodies), and p1R == fl(p0 + fl(v1R dt)).
  moving run   v0 = force_ref.moving_velocities(v1R), one step at the same dt, on the same context after a second upload.  On
               every owned body v1M == fl(v0 + v1R) and p1M == fl(p0 + fl(v1M dt)) bit for bit (euler_update of
               csrc/nbx_pair.hpp is add_rn(v, mul_rn(a, dt)), the kernels are deterministic and the acceleration depends on the
               positions only); bodies outside the slice have not moved; the returned energy is 0.5 sum m v1M^2 of the
               downloaded velocities to 1e-13.

tests/test_moving_probe_cpu.py shows on the CPU oracle that both identities hold at these time steps, and that each of: a
wrong body's or component's v0, 0.1 in place of dt in either update, a dt left as a double on fp32 data, and a fused velocity
update is caught by one of these checks in every state family (and names the blind spots).

Time steps: D1 = float32(0.013) and D2 = float32(-0.07): exact in float and in double, no powers of two, unlike 0.1 in magnitude
and in sign.  Instance idx of INSTANCES (the step probe's list of all 56 step instances, imported with its truth cache) runs at
D1 where (idx // 2) is even and at D2 where it is odd, while the small shape alternates with idx itself (n = 63 for even idx,
n = 5 for odd, as in the step probe): pairs of neighbours in the list share a time step and all four combinations of the two
occur.  The time step is part of each test's id and of each record of the report.  Shapes per instance: n = 4099 whole, the
slice [1000, +2077) of 4099 with n_alloc = 4608 through nbx_step_local / nbx_commit / nbx_kenergy_partial, and the small n;
families seed42 and adversarial each.  One fp32 and one fp64 instance of each kind (one launch per step, row epilogue, slab
plus integrate_kernel) also run dt = 0 and the double 0.1, which is no float.

Also here: ensemble and ragged members (every member a different family), groups of logical ranks against a single context,
exact mode against the CPU oracle at D1 and D2 over nine steps (what dt means, anchored to the reference's arithmetic), and
graph replay: a cached window must be keyed by its time step.

Every case's K_max, K_ref, gate, instance, dt and the number of bodies whose v1M differs from v0 go to moving_probe.json in the
GPU suite's report directory (OUT of tests/test_parity_gpu.py).

Measured on an MI355X when this module was written: every identity held on every body of all 400 recorded cases.  The worst
K / gate is 0.52 (force-f32-b2-sgpr-row-asm on the slice, seed42, at the double 0.1: 53.2 against the gate 102.4; reference-order
shapes sit at K_ref as in the step probe), 0.26 over the ensemble and ragged members; at least 79 % of a case's bodies end with
v1M != v0 (50 of 63; the others are the v0 = 0 and cancelling recipes).  The 56 instance tests take 4.5 s; this module and the
step probe together, sharing the truth cache, 11.7 s for 154 tests, and no test more than 1.5 s.
"""
import json
import os

import numpy as np
import pytest

import energy_ref
import force_ref as R
from test_step_probe_gpu import (EPI_ROW, EPI_SLAB, INST_FORCE, INST_JLANE, INSTANCES, JSRC_SGPR, LOOP_ASM, LOOP_CXX, SLICE, _round_up,
                                 instance_from_stats, instance_name, reference_of, shape_opts, state_of)

pytestmark = pytest.mark.gpu

D1 = float(np.float32(0.013))
D2 = float(np.float32(-0.07))
P, V = ("pos_x", "pos_y", "pos_z"), ("vel_x", "vel_y", "vel_z")
FAMS = ("seed42", "adversarial")


def dt_of(idx):
    return D1 if (idx // 2) % 2 == 0 else D2


def instance_cases(idx, k):
    """The probes of one instance: ragged n whole, a slice ragged on both ends with a spare tile, and below a wave."""
    small = 5 if idx % 2 else 63
    cases = []
    for n, sl in ((4099, {}), (4099, SLICE), (small, {})):
        opts = dict(shape_opts(k, sl.get("n_alloc", _round_up(n, 256))), **sl)
        for fam in FAMS:
            cases.append(dict(n=n, precision=k[1], family=fam, opts=opts, inst=k))
    return cases


# one instance of each kind and precision for dt = 0 and the double 0.1
SPECIAL = [(INST_JLANE, 32, 2, 0, 0, 0, 0, LOOP_CXX), (INST_JLANE, 64, 2, 0, 0, 0, 0, LOOP_CXX),
           (INST_FORCE, 32, 2, JSRC_SGPR, EPI_ROW, 1, 0, LOOP_ASM), (INST_FORCE, 64, 1, JSRC_SGPR, EPI_ROW, 0, 0, LOOP_CXX),
           (INST_FORCE, 32, 4, JSRC_SGPR, EPI_SLAB, 1, 1, LOOP_ASM), (INST_FORCE, 64, 4, JSRC_SGPR, EPI_SLAB, 0, 1, LOOP_CXX)]

RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    from test_parity_gpu import OUT  # where the GPU suite leaves its reports
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "moving_probe.json"), "w") as f:
        json.dump({"gate": "K_max <= %g * max(K_ref, %g)" % (R.M, R.K_TERM), "D1": D1, "D2": D2, "cases": RECORDS}, f, indent=1)


def _T(precision):
    return np.float32 if precision == 32 else np.float64


def _xyz(d, names, rows=slice(None)):
    return np.stack([np.asarray(d[f])[rows] for f in names], axis=1)


def _with_velocities(st0, v):
    return dict(st0, vel_x=np.ascontiguousarray(v[:, 0]), vel_y=np.ascontiguousarray(v[:, 1]), vel_z=np.ascontiguousarray(v[:, 2]))


def _one_step(c, state, dt, sliced):
    """upload, one step of dt, download: (the energy the step returned, the six arrays)"""
    c.upload(state)
    if sliced:
        c.step_local(dt)
        c.commit()
        ke = 0.5 * c.kenergy_partial()
    else:
        ke = c.step(1, dt)
    return ke, c.download()


def check_gate(label, K, rows, k_ref):
    g = R.gate(k_ref)
    bad = np.flatnonzero(~(K <= g))
    assert bad.size == 0, "%s: %d bodies over the gate %.1f (K_ref %.1f); worst %s" % (
        label, bad.size, g, k_ref, [(int(rows[i]), float(K[i])) for i in bad[np.argsort(-K[bad])][:10]])


def check_moving_run(label, st0, v0, v1r, d, ke, own, precision, dt):
    """The identities, the bodies outside the slice and the energy of one moving run; dt as the kernel holds it (a value of T)."""
    n = len(st0["mass"])
    p0, v1, p1 = _xyz(st0, P, own), _xyz(d, V, own), _xyz(d, P, own)
    bad_v, bad_p = R.moving_identity_failures(p0, v0[own], v1r[own], v1, p1, precision, dt)
    assert bad_v.size == 0, (label, "v1 != fl(v0 + v1_rest) at %d bodies" % bad_v.size, own[bad_v][:10].tolist())
    assert bad_p.size == 0, (label, "p1 != fl(p0 + fl(v1 dt)) at %d bodies" % bad_p.size, own[bad_p][:10].tolist())
    rest = np.setdiff1d(np.arange(n), own)
    for f in P:
        assert np.array_equal(np.asarray(d[f])[rest], np.asarray(st0[f])[rest]), (label, "a body outside the slice moved")
    want_ke = energy_ref.diagnostics(dict(d, mass=st0["mass"]), int(own[0]), len(own), potential_too=False)["kenergy"]
    assert abs(ke - want_ke) <= 1e-13 * abs(want_ke), (label, ke, want_ke)
    return int((v1 != v0[own]).any(axis=1).sum())


def two_runs(label, step, st0, own, tr, k_ref, precision, dt, seed, dt_kernel=None):
    """The rest run and the moving run through step(state) -> (energy, arrays); dt_kernel: dt as T holds it.  Returns the record."""
    dt_kernel = dt if dt_kernel is None else dt_kernel
    n = len(st0["mass"])
    zero = np.zeros((n, 3), dtype=_T(precision))
    ke_r, dr = step(_with_velocities(st0, zero))
    v1r = _xyz(dr, V)
    K = R.k_metric(R.accel_from_v1(v1r[own], precision, dt=dt_kernel), tr, precision)
    print("%-78s dt %-9.6g K_max %8.1f  K_ref %7.1f  gate %7.1f" % (label, dt, K.max(), k_ref, R.gate(k_ref)))
    check_gate(label + " (rest run)", K, own, k_ref)
    check_moving_run(label + " (rest run)", st0, zero, v1r, dr, ke_r, own, precision, dt_kernel)
    v0 = R.moving_velocities(v1r, precision, seed)
    ke_m, dm = step(_with_velocities(st0, v0))
    moved = check_moving_run(label, st0, v0, v1r, dm, ke_m, own, precision, dt_kernel)
    return dict(case=label, dt=dt, K_max=float(K.max()), K_ref=k_ref, gate=R.gate(k_ref), bodies=int(len(own)), bodies_v1_differs_from_v0=moved), v0


def probe(nbx, oracle, case, dt, special=False):
    n, precision, family, opts, inst = case["n"], case["precision"], case["family"], case["opts"], case["inst"]
    T = _T(precision)
    st0 = state_of(oracle, family, n, precision)
    lo = opts.get("i_begin", 0)
    cnt = opts.get("i_count", 0) or n - lo
    sliced = (lo, cnt) != (0, n)
    own = np.arange(lo, lo + cnt)
    label = "%s n=%d%s %s" % (instance_name(inst), n, " [%d,+%d)" % (lo, cnt) if sliced else "", family)
    tr_all, kref_all = reference_of(oracle, family, n, precision)
    tr, k_ref = tuple(t[own] for t in tr_all), float(kref_all[own].max())
    with nbx.Context(n, precision, **opts) as c:
        st = c.stats()
        assert instance_from_stats(st) == inst, (label, instance_name(instance_from_stats(st)), st)
        rec, v0 = two_runs(label, lambda state: _one_step(c, state, dt, sliced), st0, own, tr, k_ref, precision, dt,
                           seed=16 * INSTANCES.index(inst) + 2 * R.FAMILIES.index(family) + sliced, dt_kernel=float(T(dt)))
        rec.update(instance=instance_name(inst), n=n, precision=precision, family=family, i_begin=lo, i_count=cnt)
        RECORDS.append(rec)
        if special:  # dt = 0 changes nothing, and reports the energy of the velocities it was given
            moving = _with_velocities(st0, v0)
            ke, d = _one_step(c, moving, 0.0, sliced)
            for f in P + V:
                assert np.array_equal(np.asarray(d[f])[own], np.asarray(moving[f])[own]), (label, "dt = 0", f)
            for f in P:
                assert np.array_equal(d[f], st0[f]), (label, "dt = 0", f)
            want_ke = energy_ref.diagnostics(moving, lo, cnt, potential_too=False)["kenergy"]
            assert want_ke > 0 and abs(ke - want_ke) <= 1e-13 * want_ke, (label, "dt = 0", ke, want_ke)
    return rec


# ---- every step instance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(INSTANCES)), ids=["%s@%.3g" % (instance_name(k), dt_of(i)) for i, k in enumerate(INSTANCES)])
def test_step_instance_with_moving_bodies(nbx, oracle, idx):
    k = INSTANCES[idx]
    for case in instance_cases(idx, k):
        probe(nbx, oracle, case, dt_of(idx))


@pytest.mark.parametrize("k", SPECIAL, ids=[instance_name(k) for k in SPECIAL])
def test_a_zero_time_step_and_one_that_is_no_float(nbx, oracle, k):
    """The double 0.1: an fp32 context must step with float32(0.1), the round-to-nearest conversion, an fp64 context with the
    double itself -- the identities and v1R / dt are evaluated with exactly that value.  Then dt = 0 from the moving state."""
    assert k in INSTANCES and float(np.float32(0.1)) != 0.1
    for fam in FAMS:
        for sl in ({}, SLICE):
            opts = dict(shape_opts(k, sl.get("n_alloc", _round_up(4099, 256))), **sl)
            rec = probe(nbx, oracle, dict(n=4099, precision=k[1], family=fam, opts=opts, inst=k), 0.1, special=True)
            assert rec["bodies_v1_differs_from_v0"] > 0


# ---- batch objects ------------------------------------------------------------------------------------------------------------------
def _batch_two_runs(label, obj, states, truths, precision, dt, instance, split):
    """Members of an Ensemble or a Ragged: member m holds states[m]; split(download) -> one dict of six arrays per member."""
    T = _T(precision)
    M = len(states)

    def run(vels):
        obj.upload([_with_velocities(s, v) for s, v in zip(states, vels)])
        ke = obj.step(1, dt)
        return ke, split(obj.download())

    ke_r, dr = run([np.zeros((len(s["mass"]), 3), dtype=T) for s in states])
    v1r = [_xyz(d, V) for d in dr]
    v0 = [R.moving_velocities(v, precision, seed=100 + m) for m, v in enumerate(v1r)]
    ke_m, dm = run(v0)
    for m in range(M):
        n = len(states[m]["mass"])
        own = np.arange(n)
        tr, kref = truths[m]
        k_ref = float(kref.max())
        lab = "%s member %d %s n=%d" % (label, m, R.FAMILIES[m], n)
        K = R.k_metric(R.accel_from_v1(v1r[m], precision, dt=dt), tr, precision)
        print("%-78s dt %-9.6g K_max %8.1f  K_ref %7.1f  gate %7.1f" % (lab, dt, K.max(), k_ref, R.gate(k_ref)))
        check_gate(lab + " (rest run)", K, own, k_ref)
        check_moving_run(lab + " (rest run)", states[m], np.zeros((n, 3), dtype=T), v1r[m], dr[m], ke_r[m], own, precision, dt)
        moved = check_moving_run(lab, states[m], v0[m], v1r[m], dm[m], ke_m[m], own, precision, dt)
        RECORDS.append(dict(case=lab, instance=instance, n=n, precision=precision, family=R.FAMILIES[m], i_begin=0, i_count=n, dt=dt,
                            K_max=float(K.max()), K_ref=k_ref, gate=R.gate(k_ref), bodies=n, bodies_v1_differs_from_v0=moved))


@pytest.mark.parametrize("dt", [D1, D2], ids=["D1", "D2"])
@pytest.mark.parametrize("opts", [{}, dict(bodies_per_lane=16)], ids=["default", "nb16"])
def test_ensemble_members_with_moving_bodies(nbx, oracle, opts, dt):
    """Five members of n = 2000, member m of family m of force_ref.FAMILIES."""
    n = 2000
    states = [state_of(oracle, f, n, 32) for f in R.FAMILIES]
    truths = [reference_of(oracle, f, n, 32) for f in R.FAMILIES]
    with nbx.Ensemble(n, len(states), 32, **opts) as e:
        st = e.stats()
        if opts:
            assert st["bodies_per_lane"] == opts["bodies_per_lane"], st
        inst = (INST_JLANE, 32, st["bodies_per_lane"], 0, 0, 0, 0, st["inner_loop"] - 1)
        assert inst in INSTANCES, st
        _batch_two_runs("ensemble[%s]" % instance_name(inst), e, states, truths, 32, dt, "ensemble-" + instance_name(inst),
                        lambda d: [{f: d[f][m] for f in d} for m in range(len(states))])


RAGGED_SIZES = (5, 65, 257, 1000, 2000)


@pytest.mark.parametrize("dt", [D1, D2], ids=["D1", "D2"])
@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_with_moving_bodies(nbx, oracle, precision, dt):
    """Members of 5, 65, 257, 1000 and 2000 bodies, member m of family m of force_ref.FAMILIES."""
    states = [state_of(oracle, f, n, precision) for f, n in zip(R.FAMILIES, RAGGED_SIZES)]
    truths = [reference_of(oracle, f, n, precision) for f, n in zip(R.FAMILIES, RAGGED_SIZES)]
    with nbx.Ragged(RAGGED_SIZES, precision) as r:
        st = r.stats()
        inst = (INST_JLANE, precision, st["bodies_per_lane"], 0, 0, 0, 0, st["inner_loop"] - 1)
        assert inst in INSTANCES, st
        _batch_two_runs("ragged[%s]" % instance_name(inst), r, states, truths, precision, dt, "ragged-" + instance_name(inst), lambda d: d)


# ---- groups -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["equal-blocks", "weighted"])
@pytest.mark.parametrize("precision", [32, 64])
def test_group_of_logical_ranks_at_another_time_step(nbx, precision, weighted):
    """Four logical ranks on one device, three steps at D2 from the seed-42 initial conditions (which move): the same bits as a
    single context of the same launch shape and record array, as test_group_of_logical_ranks_bit_equal_to_single_context sets up."""
    n = 4099
    ic = nbx.initial_conditions(n, precision)
    assert any(np.any(ic[f]) for f in V)
    shape = dict(j_split=4, bodies_per_lane=2)
    with nbx.Group(n, precision, n_ranks=4, devices=[0] * 4, weighted=weighted, **shape) as g:
        Peff = g.info(0)[0]
        assert Peff > 1
        g.upload(ic)
        ke_g = [g.step(1, D2), g.step(2, D2)]
        dg = g.download()
        stats = [g.info(r)[2] for r in range(Peff)]
    assert stats[0]["i_begin"] == 0 and sum(s["i_count"] for s in stats) == n and all(s["steps_done"] == 3 for s in stats)
    with nbx.Context(n, precision, n_alloc=stats[0]["n_alloc"], **shape) as c:
        c.upload(ic)
        ke_c = [c.step(1, D2), c.step(2, D2)]
        dc = c.download()
    for f in dc:
        assert np.array_equal(dg[f], dc[f]), f
        assert not np.array_equal(dc[f], ic[f]), f
    assert all(abs(a / b - 1.0) < 1e-12 for a, b in zip(ke_g, ke_c)), (ke_g, ke_c)


# ---- exact mode against the CPU oracle: what dt means, in the reference's arithmetic ---------------------------------------------------
@pytest.mark.parametrize("dt", [D1, D2], ids=["D1", "D2"])
@pytest.mark.parametrize("precision", [32, 64])
def test_exact_mode_equals_the_oracle_at_other_time_steps(nbx, oracle, precision, dt):
    T = _T(precision)
    rng = np.random.default_rng([11, precision])
    for n in (3, 257, 1500):
        s = oracle.State(n, T)
        for f in P:
            getattr(s, f)[:] = (rng.random(n) * 4 - 2).astype(T)
        for f in V:
            getattr(s, f)[:] = (rng.standard_normal(n) * 1e-3).astype(T)
        s.mass[:] = (rng.random(n) * 1e3).astype(T)
        st = {f: getattr(s, f).copy() for f in nbx.FIELDS}
        with nbx.Context(n, precision, kernel_variant=nbx.KERNEL_EXACT) as c:
            c.upload(st)
            c.step(9, dt=dt, kenergy=False)
            d = c.download()
        oracle.run(s, 9, dt=dt)
        for f in d:
            assert np.array_equal(d[f], getattr(s, f)), (n, f, int((d[f] != getattr(s, f)).sum()))
        for f in P:  # the nine steps were taken: a dt may stay below an ulp of a velocity at n = 3, v dt seldom below one of a position
            assert (d[f] != st[f]).mean() > 0.6, (n, f)


# ---- graph replay must follow dt ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,precision", [(777, 32), (2304, 32), (16384, 32), (2304, 64)])
def test_graph_replay_follows_the_time_step(nbx, n, precision):
    """n = 777: the one-launch kernel; n = 16384: the wave-split kernel plus integrate_kernel, two nodes per step that carry dt.  A
    context that replays windows from a hipGraph and one that launches plainly go through the same calls with three time steps,
    a cache hit at the same parity and a second upload: every energy and the final arrays must be the same bits."""
    ic = nbx.initial_conditions(n, precision)
    assert any(np.any(ic[f]) for f in V)
    out = {}
    for g in (1, 2):
        with nbx.Context(n, precision, use_graph=g) as c:
            c.upload(ic)
            kes, replays = [], []
            for steps, dt in ((8, D1), (6, D2), (8, D1), (5, D2), (4, R.DT), (None, None), (8, D2)):
                if steps is None:
                    c.upload(ic)
                    continue
                kes.append(c.step(steps, dt))
                replays.append(c.stats()["graph_replays"])
            out[g] = (kes, replays, c.download(), c.stats())
    assert out[1][3]["use_graph"] == 1 and out[2][3]["use_graph"] == 0, (out[1][3], out[2][3])
    assert all(b > a for a, b in zip([0] + out[1][1], out[1][1])), out[1][1]
    assert out[2][1] == [0] * 6
    assert out[1][0] == out[2][0], (out[1][0], out[2][0])
    assert len(set(out[1][0])) == 6  # no two calls came to the same energy: neither dt nor the upload was ignored
    for f in out[1][2]:
        assert np.array_equal(out[1][2][f], out[2][2][f]), f
    with nbx.Context(n, precision, use_graph=1) as a, nbx.Context(n, precision, use_graph=1) as b:
        a.upload(ic)
        b.upload(ic)
        trace = a.step_trace(6, D2)
        singles = [b.step(1, D2) for _ in range(6)]
        assert trace.tolist() == singles
        da, db = a.download(), b.download()
        for f in da:
            assert np.array_equal(da[f], db[f]), f
