"""The parts of the step probe (tests/test_step_probe_gpu.py) that need no device: the reference and metric of
tests/force_ref.py bite, the probe itself is sound, and the GPU module's case table reaches every compiled step instance.

- Fault injection: known index and constant faults applied to the fp64 term matrix, with the oracle's own rounding error on
  top, must land over the gate 2 max(K_ref, 16).  Two blind spots are expected and stated, not hidden: the signed box cannot see a
  wrong eps^2 (r >> eps), and a family whose bodies 0, n - 1 and tile edges are light cannot see a dropped record -- which is why
  force_ref's adversarial family puts heavy bodies there.
- Oracle probe: one oracle step from zero velocities gives v1 / dt within one unit of K of the oracle's own accelerations, and
  the position identity p1 == fl(p0 + fl(v1 dt)) bit for bit.
- Coverage: the host-only planner (csrc/nbx_plan.hpp through tests/plan_driver.cpp) plans every case of the GPU module's table
  to the instance the case names; together they are kInstances minus the four INST_EXACT rows, each with a ragged n and on a slice.
"""
import os
import subprocess

import numpy as np
import pytest

import force_ref as R
import test_step_probe_gpu as G
from conftest import ROOT
from energy_ref import EPS2, gm_as_uploaded

CSRC = os.path.join(ROOT, "nbody-demo-2023_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "plan_driver.cpp")

INDEX_FAULTS = ("last record dropped", "record 0 twice", "tail tile skipped, last 64 bodies", "bodies 2k and 2k+1 swapped",
                "lane 63 misses four records")
FAULTS = INDEX_FAULTS + ("eps^2 off by 1e-3",)


def _faulty_accelerations(st, tr):
    """name -> (n, 3) fp64 accelerations with one fault each, built from the fp64 term matrix."""
    n = len(st["mass"])
    pos, gm = (st["pos_x"], st["pos_y"], st["pos_z"]), gm_as_uploaded(st["mass"])
    a = tr[0] + tr[1]
    tail0 = (n - 1) // 256 * 256  # first record of the ragged tail tile
    first, last, tail, four = (np.zeros((n, 3)) for _ in range(4))
    for lo in range(0, n, 512):
        rows = np.arange(lo, min(lo + 512, n))
        for c, t in enumerate(R.term_rows(pos, gm, rows)):
            first[rows, c], last[rows, c] = t[:, 0], t[:, n - 1]
            tail[rows, c] = t[:, tail0:].sum(axis=1)
            four[rows, c] = t[:, n - 4:].sum(axis=1)
    out = {"last record dropped": a - last, "record 0 twice": a + first}
    f = a.copy()
    f[n - 64:] -= tail[n - 64:]
    out["tail tile skipped, last 64 bodies"] = f
    f = a.copy()
    k = np.arange(n - n % 2)
    f[k] = a[k ^ 1]
    out["bodies 2k and 2k+1 swapped"] = f
    f = a.copy()
    f[63::64] -= four[63::64]
    out["lane 63 misses four records"] = f
    wrong = R.state_truth(st, eps2=EPS2 + 1e-3)
    out["eps^2 off by 1e-3"] = wrong[0] + wrong[1]
    return out


@pytest.mark.parametrize("n", [1000, 4099])
def test_the_gate_rejects_injected_faults(oracle, n):
    seen = {f: [] for f in FAULTS}
    print("\nn = %d: K_max of each fault (oracle rounding on top) against the gate" % n)
    print("%-12s %7s %7s  " % ("family", "K_ref", "gate") + "  ".join("%-12.12s" % f for f in FAULTS))
    for fam in R.FAMILIES:
        st = R.make_state(oracle, fam, n, 32)
        tr = R.state_truth(st)
        a_or = R.oracle_accel(oracle, st).astype(np.float64)
        k_ref = R.k_metric(a_or, tr, 32).max()
        g = R.gate(k_ref)
        assert k_ref <= g / R.M  # the reference arithmetic itself passes
        rounding = a_or - (tr[0] + tr[1])
        cells = []
        for name, a in _faulty_accelerations(st, tr).items():
            K = R.k_metric(a + rounding, tr, 32).max()
            cells.append("%11.3g%s" % (K, "*" if K > g else " "))
            if K > g:
                seen[name].append(fam)
        print("%-12s %7.1f %7.1f  " % (fam, k_ref, g) + "  ".join(cells))
    print("(* = rejected)")
    for name, fams in seen.items():
        assert len(fams) >= 3, (name, "rejected only on", fams)
        assert {"seed42", "offset1000", "lattice"} <= set(fams), (name, fams)
    for name in INDEX_FAULTS:
        assert "signedbox" in seen[name], (name, seen[name])
        assert "adversarial" in seen[name], (name, "the heavy bodies at 0, n - 1 and the tile edges are there to show this", seen[name])


def test_bodies_nothing_pulls_at_must_stay_at_rest_exactly():
    tr = (np.zeros((2, 3)), np.zeros((2, 3)), np.array([0.0, 1.0]))
    assert R.k_metric(np.zeros((2, 3)), tr, 32).tolist() == [0.0, 0.0]
    K = R.k_metric(np.array([[1e-30, 0, 0], [2.0 ** -24, 0, 0]]), tr, 32)
    assert np.isinf(K[0]) and K[1] == 1.0
    for prec in (32, 64):
        for name, st, want in R.hand_placed(prec):
            tr = R.state_truth(st)
            assert (R.k_metric(want, tr, prec) <= 4).all(), (name, prec)  # the closed forms and the direct sum agree to rounding
            if name in ("n1", "n2_massless"):
                assert tr[2][0] == 0 and not want[0].any()


def test_double_double_fallback_agrees_with_long_double(oracle):
    """Where np.longdouble is a double, fp64 states are judged against a two-sum / two-product evaluation; where both exist
    they must agree far below one unit of K."""
    for fam in ("seed42", "adversarial", "lattice"):
        st = R.make_state(oracle, fam, 257, 64)
        pos, gm = (st["pos_x"], st["pos_y"], st["pos_z"]), gm_as_uploaded(st["mass"])
        dd = R.truth(pos, gm, np.arange(257), 64, force_dd=True)
        K = R.k_metric(R.oracle_accel(oracle, st), dd, 64)
        assert 1 < K.max() < 64, K.max()  # the oracle's fp64 arithmetic, seen through the fallback
        if R.HAVE_LONGDOUBLE:
            ld = R.truth(pos, gm, np.arange(257), 64)
            diff = np.abs((dd[0] - ld[0]) + (dd[1] - ld[1])).max(axis=1) / (R.U[64] * ld[2])
            assert diff.max() < 0.01, (fam, diff.max())
            assert np.allclose(dd[2], ld[2], rtol=1e-12)


@pytest.mark.parametrize("n,prec,fams", [(257, 32, R.FAMILIES), (4099, 32, R.FAMILIES), (16384, 32, ("seed42", "lattice")),
                                         (257, 64, R.FAMILIES), (4099, 64, ("seed42", "adversarial"))])
def test_the_probe_on_the_oracle_itself(oracle, n, prec, fams):
    """oracle.run(s, 1) from zero velocities: v1 / dt is the oracle's acceleration to one unit of K, positions obey the identity."""
    T = np.float32 if prec == 32 else np.float64
    for fam in fams:
        st = R.make_state(oracle, fam, n, prec)
        tr = R.state_truth(st)
        K_acc = R.k_metric(R.oracle_accel(oracle, st), tr, prec)
        s = oracle.State(n, T)
        for f in ("pos_x", "pos_y", "pos_z", "mass"):
            getattr(s, f)[:] = st[f]
        oracle.run(s, 1)
        v1 = np.stack([s.vel_x, s.vel_y, s.vel_z], axis=1)
        K_probe = R.k_metric(R.accel_from_v1(v1, prec), tr, prec)
        print("n %6d fp%d %-12s K_ref max %6.1f median %5.1f; through the probe %6.1f" % (n, prec, fam, K_acc.max(), np.median(K_acc), K_probe.max()))
        assert np.abs(K_probe - K_acc).max() <= 1.0, (fam, np.abs(K_probe - K_acc).max())
        for ax, v in zip("xyz", (s.vel_x, s.vel_y, s.vel_z)):
            assert np.array_equal(getattr(s, "pos_" + ax), R.position_identity(st["pos_" + ax], v, prec)), (fam, ax)


# ---- coverage of the case table ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def test_the_case_table_reaches_every_step_instance(driver):
    declared = [tuple(map(int, line.split())) for line in
                subprocess.run([driver, "instances"], capture_output=True, text=True, check=True).stdout.splitlines()]
    want = {k for k in declared if k[0] != G.INST_EXACT}
    assert len(declared) == 60 and len(want) == 56
    assert set(G.INSTANCES) == want and len(G.INSTANCES) == 56  # the list written out in the GPU module is the header's

    rows = "".join(G.planner_row(c) + "\n" for c in G.CASES)
    out = subprocess.run([driver, "both", "256"], input=rows, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(G.CASES)
    step_seen, accel_seen, ragged, sliced = set(), set(), set(), set()
    for case, line in zip(G.CASES, out):
        v = line.split()
        assert v[0] == "P", (case, line)
        v = list(map(int, v[1:]))
        plan = dict(zip(("variant", "order", "B", "S", "jps", "math", "epi", "loop", "grid_x", "grid_y", "use_graph", "pairs"), v[:12]))
        step, accel = tuple(v[12:20]), tuple(v[20:28])
        assert step == case["inst"], (G.planner_row(case), G.instance_name(step), G.instance_name(case["inst"]))
        # what the device test reads from nbx_stats names the same instance
        stats = dict(precision=case["precision"], kernel_variant=plan["variant"], bodies_per_lane=plan["B"], fused_epilogue=plan["epi"],
                     inner_loop=plan["loop"] + 1, j_split=plan["S"], force_grid_x=plan["grid_x"], force_grid_y=plan["grid_y"])
        assert G.instance_from_stats(stats) == step, (stats, step)
        for f, val in case.get("stats", {}).items():
            assert stats[f] == val, (case.get("id"), f, stats[f], val)
        step_seen.add(step)
        accel_seen.add(accel)
        if case["n"] % 256:
            ragged.add(step)
        if case["opts"].get("i_count"):
            sliced.add(step)
    # an instance no nbx_opts reaches would show up here by name
    assert step_seen == want, sorted(G.instance_name(k) for k in want - step_seen)
    assert ragged == want, sorted(G.instance_name(k) for k in want - ragged)
    assert sliced == want, sorted(G.instance_name(k) for k in want - sliced)
    slab_forms = {k for k in want if k[0] == G.INST_JLANE or k[4] == G.EPI_SLAB}
    assert slab_forms <= accel_seen, sorted(G.instance_name(k) for k in slab_forms - accel_seen)
    assert all(k[0] == G.INST_JLANE or k[4] == G.EPI_SLAB for k in accel_seen)
    print("\n%d cases; step instances reached: %d of %d (ragged n: %d, on a slice: %d); nbx_accel forms reached: %d" % (
        len(G.CASES), len(step_seen), len(want), len(ragged), len(sliced), len(accel_seen)))
    for k in G.INSTANCES:
        print("  %-32s %3d cases" % (G.instance_name(k), sum(c["inst"] == k for c in G.CASES)))


def test_sampled_bodies_of_a_large_shape_include_the_edges():
    for lo, cnt, per_wg in ((0, 262144, 512), (917504, 131072, 512), (65536, 65536, 256), (229376, 32768, 256), (0, 16384, 256)):
        rows = G.sample_bodies(lo, cnt, per_wg)
        assert len(rows) == 256 == len(set(rows.tolist())) and rows.min() == lo and rows.max() == lo + cnt - 1
        last_wg = lo + (cnt - 1) // per_wg * per_wg
        assert {lo + per_wg - 1, lo + per_wg, last_wg - 1, last_wg, lo + 255, lo + 256} <= set(rows.tolist())
