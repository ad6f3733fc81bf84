"""The parts of the moving probe (tests/test_moving_probe_gpu.py) that need no device: the two identities

    v1 == fl(v0 + v1_rest)        v1_rest = fl(a dt): what the same step leaves from rest
    p1 == fl(p0 + fl(v1 dt))

hold bit for bit where the arithmetic is known to be the reference's (the CPU oracle's accelerations and its Euler update), at
time steps other than the reference's (float)0.1, and the faults the probe is there for break them.

- Identities on the oracle: one oracle.accel plus oracle.integrate step from rest and from force_ref.moving_velocities, fp32
  (n = 4099) and fp64 (n = 1000), all five families, at float32(0.013), float32(-0.07), float32(0.1) and 2.5.  Both hold on
  every body, and K of v1_rest / dt is within one unit of the oracle's own K, so the gate of the step probe needs no new margin.
- Injected faults: the probe's procedure (rest run, velocities drawn from its result, moving run, the checks) run on a model
  of euler_update with one fault each.  Every fault must be caught on at least one body in every family, at both time steps.
  What catches it differs and is printed: a wrong body's or component's v0, a C double dt on float data and a fused velocity
  update break the velocity identity; 0.1 in the position update breaks the position identity; 0.1 in the velocity update
  alone breaks neither -- both runs carry the same wrong fl(a 0.1) -- and is caught by the gate, K of v1_rest / dt being off
  by |0.1 / dt - 1| |a| / (u A).
- Blind spots, stated and not hidden: a FUSED POSITION update (p1 = fl(p0 + v1 dt), one rounding) is seen on seed42,
  adversarial and lattice only.  On offset1000 the positions near 1000 swamp v dt -- an ulp of p is 6e-5 in fp32 against
  |v dt| <= 0.07 carried to 4e-9 -- and it shows on no body at these time steps; on signedbox (|p| up to 100) on a handful at
  most.  The count per family is printed, and nothing is asserted on those two.  Bodies of recipe 4 (v0 = 0) cannot see a
  fused velocity update; those of recipe 3 (v0 = -v1_rest) see it best, since fl(a dt - fl(a dt)) is the rounding error of
  the product and not zero.  A body with a == 0 sees no dt fault at all.
"""
import numpy as np
import pytest

import force_ref as R
import test_moving_probe_gpu as G
import test_step_probe_gpu as S

D1 = float(np.float32(0.013))
D2 = float(np.float32(-0.07))
SIZES = {32: 4099, 64: 1000}
P, V = ("pos_x", "pos_y", "pos_z"), ("vel_x", "vel_y", "vel_z")

FAULTS = ("v0 read from body i - 1", "x and y of v0 swapped", "0.1 in the velocity update only", "0.1 in the position update only",
          "velocity update fused")
DOUBLE_DT = "dt not converted to T"  # fp32 data, the double 0.1: C promotes `v += a * dt` to double, one rounding at the store


def _T(prec):
    return np.float32 if prec == 32 else np.float64


def _fma(a, b, c, prec):
    """fl(a b + c) with one rounding: in fp64 for fp32 values (the product is exact, the double rounding of the sum is the one
    an fp32 FMA can differ by only when the fp64 sum lies within 2^-29 ulp of a tie), by two-product / two-sum for fp64 values."""
    if prec == 32:
        return (np.asarray(a, dtype=np.float64) * np.float64(b) + np.asarray(c, dtype=np.float64)).astype(np.float32)
    b = np.broadcast_to(np.float64(b), np.shape(a))
    p, e = R._two_prod(np.asarray(a, dtype=np.float64), b)
    s, t = R._two_sum(np.asarray(c, dtype=np.float64), p)
    return s + (t + e)


def model_step(acc, p0, v0, prec, dt, fault=None):
    """euler_update (csrc/nbx_pair.hpp) in numpy: v1 = fl(v0 + fl(a dt)), p1 = fl(p0 + fl(v1 dt)), all in T; with one fault."""
    T = _T(prec)
    dt_v = dt_p = T(dt)
    if fault == "v0 read from body i - 1":
        v0 = np.roll(v0, 1, axis=0)
    elif fault == "x and y of v0 swapped":
        v0 = v0[:, [1, 0, 2]]
    elif fault == "0.1 in the velocity update only":
        dt_v = T(R.DT)
    elif fault == "0.1 in the position update only":
        dt_p = T(R.DT)
    if fault == DOUBLE_DT:
        assert prec == 32
        v1 = (v0.astype(np.float64) + acc.astype(np.float64) * np.float64(dt)).astype(T)
        return v1, (p0.astype(np.float64) + v1.astype(np.float64) * np.float64(dt)).astype(T)
    v1 = _fma(acc, dt_v, v0, prec) if fault == "velocity update fused" else (v0 + (acc * dt_v).astype(T)).astype(T)
    p1 = _fma(v1, dt_p, p0, prec) if fault == "position update fused" else (p0 + (v1 * dt_p).astype(T)).astype(T)
    return v1.astype(T), p1.astype(T)


_CACHE = {}


def _case(oracle, fam, prec):
    """(state, p0 (n, 3), oracle accelerations (n, 3) in T, truth, K of the oracle per body), once per family and precision"""
    key = (fam, prec)
    if key not in _CACHE:
        st = R.make_state(oracle, fam, SIZES[prec], prec)
        acc = R.oracle_accel(oracle, st)
        tr = R.state_truth(st)
        _CACHE[key] = (st, np.stack([st[f] for f in P], axis=1), acc, tr, R.k_metric(acc, tr, prec))
    return _CACHE[key]


def _oracle_step(oracle, st, acc, v0, dt):
    """One oracle.integrate of the state with the accelerations `acc` and velocities v0: (v1, p1, sum m v1^2)."""
    n, T = len(st["mass"]), st["mass"].dtype.type
    s = oracle.State(n, T)
    for f in P + ("mass",):
        getattr(s, f)[:] = st[f]
    for c, ax in enumerate("xyz"):
        getattr(s, "vel_" + ax)[:] = v0[:, c]
        getattr(s, "acc_" + ax)[:] = acc[:, c]
    e = oracle.integrate(s, dt)
    return np.stack([getattr(s, f) for f in V], axis=1), np.stack([getattr(s, f) for f in P], axis=1), e


def run_probe(step, p0, tr, k_ref, prec, dt, seed, dt_check=None):
    """The probe's procedure on step(v0) -> (v1, p1): (K_max of v1_rest / dt, gate, bodies failing the velocity identity,
    bodies failing the position identity in either run, bodies whose v1 differs from v0)."""
    dt_check = dt if dt_check is None else dt_check
    zero = np.zeros_like(p0)
    v1r, p1r = step(zero)
    K = R.k_metric(R.accel_from_v1(v1r, prec, dt=dt_check), tr, prec)
    v0 = R.moving_velocities(v1r, prec, seed)
    v1m, p1m = step(v0)
    bad_v, bad_p = R.moving_identity_failures(p0, v0, v1r, v1m, p1m, prec, dt_check)
    bad_pr = R.moving_identity_failures(p0, zero, v1r, v1r, p1r, prec, dt_check)[1]
    return float(K.max()), R.gate(k_ref), bad_v, np.union1d(bad_p, bad_pr), int((v1m != v0).any(axis=1).sum())


@pytest.mark.parametrize("prec", [32, 64])
def test_both_identities_hold_on_the_oracle_at_other_time_steps(oracle, prec):
    T = _T(prec)
    for fam in R.FAMILIES:
        st, p0, acc, tr, K_acc = _case(oracle, fam, prec)
        for dt in (D1, D2, R.DT, 2.5):
            def step(v0):
                v1, p1, _ = _oracle_step(oracle, st, acc, v0, dt)
                # the numpy model the fault table is built on is the oracle's update, bit for bit
                m1, q1 = model_step(acc, p0, v0, prec, dt)
                assert np.array_equal(v1, m1) and np.array_equal(p1, q1), (fam, dt)
                return v1, p1
            K, g, bad_v, bad_p, moved = run_probe(step, p0, tr, K_acc.max(), prec, dt, seed=7)
            print("fp%d %-12s dt %-9.6g K(v1_rest / dt) %6.2f  K_ref %6.2f  gate %6.1f; %d of %d bodies with v1 != v0" % (
                prec, fam, dt, K, K_acc.max(), g, moved, len(p0)))
            assert bad_v.size == 0, (fam, dt, "v1 != fl(v0 + v1_rest) at bodies", bad_v[:10].tolist())
            assert bad_p.size == 0, (fam, dt, "p1 != fl(p0 + fl(v1 dt)) at bodies", bad_p[:10].tolist())
            assert abs(K - K_acc.max()) <= 1.0 and K <= g, (fam, dt, K, K_acc.max())
            assert T(dt) == dt  # every one of these time steps is a value of T


def test_moving_velocities_follow_the_five_recipes(oracle):
    for prec in (32, 64):
        st, p0, acc, tr, _ = _case(oracle, "seed42", prec)
        v1r = model_step(acc, p0, np.zeros_like(p0), prec, D1)[0]
        v0 = R.moving_velocities(v1r, prec, seed=3)
        assert v0.dtype == _T(prec) and v0.shape == v1r.shape
        assert np.array_equal(v0, R.moving_velocities(v1r, prec, seed=3)) and not np.array_equal(v0, R.moving_velocities(v1r, prec, seed=4))
        i = np.arange(len(v0))
        assert np.abs(v0[i % 5 == 0]).max() <= 1 and np.abs(v0[i % 5 == 0]).mean() > 0.4
        ratio = v0[i % 5 == 1] / v1r[i % 5 == 1]
        assert np.abs(ratio).max() <= 4.000001 and np.abs(ratio).mean() > 1.5
        assert np.array_equal(v0[i % 5 == 2], -v1r[i % 5 == 2]) and not v0[i % 5 == 3].any()
        assert not R.velocity_identity(v0, v1r, prec)[i % 5 == 2].any()
        big = np.abs(v0[i % 5 == 4] / v1r[i % 5 == 4])
        assert 100 < np.median(big) < 2000
        # no two bodies and no two components of a body share a drawn value
        drawn = v0[(i % 5 != 3)].ravel()
        assert len(np.unique(drawn)) == drawn.size


@pytest.mark.parametrize("prec", [32, 64])
def test_every_injected_fault_is_caught_in_every_family(oracle, prec):
    n = SIZES[prec]
    faults = FAULTS + ((DOUBLE_DT,) if prec == 32 else ())
    print("\nfp%d n = %d: bodies failing the velocity / the position identity (G: over the gate), per fault" % (prec, n))
    fused = {}
    for fam in R.FAMILIES:
        st, p0, acc, tr, K_acc = _case(oracle, fam, prec)
        for fault in faults + ("position update fused",):
            # a double dt shows only where the double is no value of T: the double 0.1 on fp32 data, checked with float32(0.1)
            for dt, dt_check in (((0.1, R.DT),) if fault == DOUBLE_DT else ((D1, D1), (D2, D2))):
                K, g, bad_v, bad_p, _ = run_probe(lambda v0: model_step(acc, p0, v0, prec, dt, fault), p0, tr, K_acc.max(), prec, dt,
                                                  seed=7, dt_check=dt_check)
                print("  %-12s %-34s dt %-9.6g velocity %5d  position %5d  %s" % (fam, fault, dt, bad_v.size, bad_p.size, "G" if K > g else ""))
                if fault == "position update fused":
                    fused[fam, dt] = bad_p.size
                    assert bad_v.size == 0 and K <= g  # it touches nothing else
                    continue
                assert bad_v.size or bad_p.size or K > g, (fam, fault, dt, "passes the probe")
                if fault in ("v0 read from body i - 1", "x and y of v0 swapped", "velocity update fused", DOUBLE_DT):
                    assert bad_v.size, (fam, fault, dt)
                if fault == "velocity update fused":  # a body at rest cannot show it; one whose v0 cancels v1_rest nearly always does
                    assert not (bad_v % 5 == 3).any()
                    assert (bad_v % 5 == 2).sum() > n // 10, (fam, dt, (bad_v % 5 == 2).sum())
                if fault == "0.1 in the position update only":
                    # the bodies of recipe 1, a fifth of all, move by |v (0.1 - dt)| ~ 0.04: far above an ulp of any position here
                    assert bad_p.size > n // 10 and bad_v.size == 0 and K <= g, (fam, dt, bad_p.size)
                if fault == "0.1 in the velocity update only":
                    assert K > g and bad_v.size == 0, (fam, dt, K, g)
    # the blind spot of the docstring: asserted where the fused position update is visible, printed where it is not
    for fam in ("seed42", "adversarial", "lattice"):
        for dt in (D1, D2):
            assert fused[fam, dt] > 0, (fam, dt)
    print("  position update fused, bodies seen: " + ", ".join("%s %s" % (fam, [fused[fam, d] for d in (D1, D2)]) for fam in R.FAMILIES))


def test_the_time_step_keyword_leaves_the_defaults_unchanged(oracle):
    for prec in (32, 64):
        st, p0, acc, tr, _ = _case(oracle, "seed42", prec)
        v = model_step(acc, p0, np.zeros_like(p0), prec, R.DT)[0]
        assert np.array_equal(R.accel_from_v1(v, prec), R.accel_from_v1(v, prec, dt=R.DT))
        assert np.array_equal(R.position_identity(p0, v, prec), R.position_identity(p0, v, prec, dt=R.DT))
        assert not np.array_equal(R.accel_from_v1(v, prec), R.accel_from_v1(v, prec, dt=D1))
        assert not np.array_equal(R.position_identity(p0, v, prec), R.position_identity(p0, v, prec, dt=D1))
        # and the defaults are still the reference's (float)0.1
        assert np.array_equal(R.accel_from_v1(v, prec), v.astype(np.longdouble if prec == 64 and R.HAVE_LONGDOUBLE else np.float64) / np.float32(0.1))


# ---- the case table of the GPU module ---------------------------------------------------------------------------------------------
def test_the_case_table_runs_every_instance_at_a_time_step_other_than_the_reference_s():
    assert (G.D1, G.D2) == (D1, D2) and R.DT not in (D1, D2) and len(S.INSTANCES) == 56
    for d in (D1, D2):  # values of float, hence of double, and no powers of two
        assert float(np.float32(d)) == d and np.frexp(abs(d))[0] != 0.5
    assert {(G.dt_of(i), 5 if i % 2 else 63) for i in range(56)} == {(D1, 63), (D1, 5), (D2, 63), (D2, 5)}
    # every shape is one of the step probe's own cases, so what tests/test_step_probe_cpu.py shows with the host-only planner --
    # each case is planned to the instance it names, and together they are all 56 -- holds for this table too
    planned = {(c["n"], c["precision"], S.planner_row(c), c["inst"]) for c in S.CASES}
    for idx, k in enumerate(S.INSTANCES):
        cases = G.instance_cases(idx, k)
        small = 5 if idx % 2 else 63
        assert [(c["n"], bool(c["opts"].get("i_count")), c["family"]) for c in cases] == [
            (n, sl, fam) for n, sl in ((4099, False), (4099, True), (small, False)) for fam in ("seed42", "adversarial")]
        for c in cases:
            assert (c["n"], c["precision"], S.planner_row(c), k) in planned, (S.instance_name(k), c)
    kinds = {(k[0] == S.INST_JLANE, k[0] == S.INST_FORCE and k[4] == S.EPI_ROW, k[1]) for k in G.SPECIAL}
    assert len(kinds) == 6 and all(k in S.INSTANCES for k in G.SPECIAL)
