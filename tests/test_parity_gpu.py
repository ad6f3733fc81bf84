"""T4/T5/T7: the HIP path (through the C-ABI) against the oracle, the reference's golden traces
and size-independent properties.  Everything here needs an MI355X: `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu

# Exact mode reproduces the reference's positions and velocities bit for bit, but sums m*v^2 in fp64 in a fixed order
# where the reference adds floats in OpenMP thread order (ver7/GSimulation.cpp:179,196): the reference's own kenergy
# moves by 1e-6..5e-6 with the thread count (3.0e-6 measured against the n = 262144 x 200 fixture).
# One bound for every "same trajectory, different energy sum" comparison in fp32:
EXACT_MODE_ENERGY_TOL_F32 = 1e-5

OUT = os.path.join(ROOT, "gpurun_out")


def _oracle_acc(oracle, n, dtype=np.float32):
    s = oracle.init_state(n).astype(dtype)
    oracle.accel(s)
    return s


def _gpu_acc(nbx, n, precision=32, **opts):
    with nbx.Context(n, precision, **opts) as c:
        c.upload(nbx.initial_conditions(n, precision))
        ax, ay, az = c.accel()
        st = c.stats()
    return ax, ay, az, st


def _acc_err(got, ref):
    scale = max(np.abs(ref.acc_x).max(), np.abs(ref.acc_y).max(), np.abs(ref.acc_z).max())
    scale = scale if scale > 0 else 1.0  # n == 1: the only pair is j == i, which contributes exactly 0
    return max(np.abs(got[0].astype(np.float64) - ref.acc_x).max(), np.abs(got[1].astype(np.float64) - ref.acc_y).max(),
               np.abs(got[2].astype(np.float64) - ref.acc_z).max()) / scale


# ---- per-body accelerations after the first force evaluation (fp32: 1e-5 of |a|inf) -------------
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 255, 256, 257, 1000, 2000, 4099, 16384])
def test_accel_fp32_vs_oracle(nbx, oracle, n):
    ref = _oracle_acc(oracle, n)
    ax, ay, az, _ = _gpu_acc(nbx, n)
    assert _acc_err((ax, ay, az), ref) < 1e-5


@pytest.mark.parametrize("n", [5, 65, 2000, 4099])
def test_accel_fp64_vs_oracle(nbx, oracle, n):
    ref = _oracle_acc(oracle, n, np.float64)
    ax, ay, az, _ = _gpu_acc(nbx, n, 64)
    assert _acc_err((ax, ay, az), ref) < 1e-12


# ---- T5: results do not depend on the launch shape ----------------------------------------------
SHAPES = [dict(bodies_per_lane=b, j_split=s, kernel_variant=k, fused_epilogue=2)
          for b in (1, 2, 4, 8) for s in (1, 3, 16) for k in (1, 2, 3) if not (k == 3 and b == 8)]


def test_accel_invariant_to_launch_shape(nbx, oracle):
    n = 4099
    ref = _oracle_acc(oracle, n)
    worst = 0.0
    for o in SHAPES:
        ax, ay, az, st = _gpu_acc(nbx, n, **o)
        assert st["bodies_per_lane"] == o["bodies_per_lane"] and st["kernel_variant"] == o["kernel_variant"]
        worst = max(worst, _acc_err((ax, ay, az), ref))
    assert worst < 1e-5, worst


def test_fused_and_split_steps_agree(nbx):
    n = 2000
    ic = nbx.initial_conditions(n)
    traces = []
    for o in (dict(j_split=1, fused_epilogue=1, kernel_variant=1), dict(j_split=1, fused_epilogue=2, kernel_variant=1),
              dict(j_split=4), dict(j_split=1, fused_epilogue=1, kernel_variant=2, bodies_per_lane=4),
              dict(j_split=1, fused_epilogue=1), dict(j_split=7, kernel_variant=3, bodies_per_lane=1)):
        with nbx.Context(n, 32, **o) as c:
            c.upload(ic)
            traces.append(c.step_trace(60))
    for t in traces[1:]:
        assert rel_err(t, traces[0]).max() < 2e-6
    # fused vs separate epilogue with the same force kernel: the very same arithmetic
    assert np.array_equal(traces[0], traces[1])


# ---- one launch per step for launch-bound sizes: a wave owns NB bodies, its lanes split j (NBX_KERNEL_JLANE) ----------
@pytest.mark.parametrize("NB", [2, 4, 8, 16])
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 255, 257, 1000, 2000, 4099])
def test_jlane_accelerations_vs_oracle(nbx, oracle, n, NB):
    ref = _oracle_acc(oracle, n)
    ax, ay, az, st = _gpu_acc(nbx, n, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB)
    assert st["kernel_variant"] == nbx.KERNEL_JLANE and st["bodies_per_lane"] == NB and st["j_split"] == 1
    assert _acc_err((ax, ay, az), ref) < 1e-5


@pytest.mark.parametrize("NB", [2, 4, 8])
@pytest.mark.parametrize("n", [1, 5, 65, 257, 2000, 4099])
def test_jlane_fp64_accelerations_vs_oracle(nbx, oracle, n, NB):
    ref = _oracle_acc(oracle, n, np.float64)
    ax, ay, az, st = _gpu_acc(nbx, n, 64, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB)
    assert st["kernel_variant"] == nbx.KERNEL_JLANE and st["bodies_per_lane"] == NB and st["precision"] == 64
    assert _acc_err((ax, ay, az), ref) < 1e-12


@pytest.mark.parametrize("name", ["ver7_f64_n5_s20.json", "ver7_f64_n2000_s500.json", "ver7_f64_n4099_s40.json"])
def test_jlane_fp64_traces_against_the_reference_fp64_build(nbx, name):
    """The fp64 variant's gate (1e-10) with the one-launch kernel, which is the default at these sizes; graph replay on."""
    g = load_golden(name)
    n, steps = g["n"], g["nsteps"]
    with nbx.Context(n, 64) as c:
        c.upload(nbx.initial_conditions(n, 64))
        ke = c.step_trace(steps)
        assert c.stats()["kernel_variant"] == nbx.KERNEL_JLANE
    assert rel_err(ke, g["kenergy"]).max() < 1e-10
    with nbx.Context(n, 64, use_graph=1) as c, nbx.Context(n, 64, kernel_variant=nbx.KERNEL_SGPRW) as t:
        ic = nbx.initial_conditions(n, 64)
        c.upload(ic)
        t.upload(ic)
        assert c.step(steps) == ke[-1]                       # replayed from a graph: same bits
        assert abs(t.step(steps) / ke[-1] - 1.0) < 1e-12     # the two-launch tree shape: another tree, same answer


@pytest.mark.parametrize("n,steps,NB", [(2000, 500, 0), (4099, 40, 0), (1000, 100, 16), (65, 20, 4), (5, 20, 2), (8192, 30, 0), (15000, 100, 0)])
def test_jlane_trajectory_matches_the_two_launch_tree_shape_and_the_reference(nbx, n, steps, NB):
    """force + Euler + energy in one launch: kinetic energy within rounding of the SGPRW + integrate_kernel pair at every step,
    against the reference's fixture where one exists, bitwise reproducible, and identical under hipGraph replay."""
    ic = nbx.initial_conditions(n)
    opts = dict(kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB)
    with nbx.Context(n, 32, use_graph=2, **opts) as c:
        c.upload(ic)
        ke = c.step_trace(steps)
        fin = c.download()
        st = c.stats()
    assert st["kernel_variant"] == nbx.KERNEL_JLANE and st["fused_epilogue"] == 1 and st["force_grid_y"] == 1
    with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_SGPRW, use_graph=2) as c:
        c.upload(ic)
        assert rel_err(ke, c.step_trace(steps)).max() < 5e-6
    name = "ver7_f32_n%d_s%d.json" % (n, steps)
    if os.path.exists(os.path.join(ROOT, "tests", "golden", name)):
        assert rel_err(ke, load_golden(name)["kenergy"]).max() < 1e-5
    with nbx.Context(n, 32, use_graph=1, **opts) as c:  # replayed from a graph, energy asked once at the end
        c.upload(ic)
        ke_last = c.step(steps)
        fin2 = c.download()
        assert c.stats()["graph_replays"] > 0 or steps < 4
    assert ke_last == ke[-1]
    for f in fin:
        assert np.array_equal(fin[f], fin2[f]), f


@pytest.mark.parametrize("name", ["ver7_f32_n4096_s200.json", "ver7_f32_n8192_s200.json", "ver7_f32_n12288_s100.json", "ver7_f32_n15000_s100.json"])
def test_jlane_sizes_against_the_reference_binary(nbx, name):
    """The sizes the one-launch kernel serves by default (NB = 2, 4, 8) against fixtures produced by the reference's own
    ver7 binary: kinetic energy at every printed step (s % 50 == 0) within the north-star gate of 1e-4, and the exact mode
    on the reference's bits at the end of the run."""
    g = load_golden(name)
    n, steps = g["n"], g["nsteps"]
    ref = np.array(g["kenergy"])
    with nbx.Context(n, 32) as c:
        c.upload(nbx.initial_conditions(n))
        ke = c.step_trace(steps)
        assert c.stats()["kernel_variant"] == nbx.KERNEL_JLANE
    e = rel_err(ke, ref)
    _dump("parity_jlane_%s" % name, {"max": float(e.max()), "printed": {str(k): float(e[k - 1]) for k in range(50, steps + 1, 50)},
                                      "all_steps": [float(x) for x in e]})
    for k in range(50, steps + 1, 50):
        assert e[k - 1] < 1e-4, (k, e[k - 1])
    with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_EXACT) as c:
        c.upload(nbx.initial_conditions(n))
        c.step(steps, kenergy=False)
        d = c.download()
    for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert _crc(d[f]) == g["final"][f]["crc32"], f


@pytest.mark.parametrize("NB", [2, 4, 8])
@pytest.mark.parametrize("n,steps", [(5, 10), (300, 30), (2000, 40), (2048, 20), (4099, 20), (8192, 10), (12288, 6), (768, 25), (15000, 5), (16383, 4)])
def test_jlane_hand_scheduled_main_loop_is_bit_equal_to_the_compiled_one(nbx, n, steps, NB):
    """Whole trips of 8 records per lane through the generated loop (nbx_jlane_loop.inc), the remainder through the compiled
    one: same bits as the all-compiled kernel -- sizes with 0 trips (n <= 256), with and without a 4-record remainder."""
    ic = nbx.initial_conditions(n)
    res = []
    for loop in (nbx.LOOP_ASM, nbx.LOOP_CXX):
        with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
            c.upload(ic)
            acc = c.accel()
            ke = c.step_trace(steps)
            st = c.stats()
            assert st["inner_loop"] == loop and st["kernel_variant"] == nbx.KERNEL_JLANE and st["bodies_per_lane"] == NB
            res.append((acc, ke, c.download()))
    for q in range(3):
        assert np.array_equal(res[0][0][q], res[1][0][q]), q
    assert np.array_equal(res[0][1], res[1][1])
    for f in res[0][2]:
        assert np.array_equal(res[0][2][f], res[1][2][f]), f


def test_jlane_is_the_default_for_launch_bound_sizes_and_shards_like_the_others(nbx):
    for n, want in ((2000, nbx.KERNEL_JLANE), (8192, nbx.KERNEL_JLANE), (16384, nbx.KERNEL_SGPRW), (262144, nbx.KERNEL_SGPR)):
        with nbx.Context(n, 32) as c:
            assert c.stats()["kernel_variant"] == want, n
    # round 3: also between 12288 and 16384 bodies (6-15 % ahead of the two-launch shape there), 8 bodies per wave with the generated
    # loop; 16384 itself -- BASELINE configs[1] -- keeps the wave-split kernel whose summation tree its fixture was validated with
    for n, nb in ((12288, 4), (13000, 8), (15000, 8), (16383, 8)):
        with nbx.Context(n, 32) as c:
            st = c.stats()
            assert (st["kernel_variant"], st["bodies_per_lane"]) == (nbx.KERNEL_JLANE, nb), (n, st)
            assert st["inner_loop"] == (nbx.LOOP_ASM if nb == 8 else st["inner_loop"])
    for n, want in ((2000, nbx.KERNEL_JLANE), (12288, nbx.KERNEL_JLANE), (16384, nbx.KERNEL_SGPRW)):  # fp64 form, same threshold
        with nbx.Context(n, 64) as c:
            assert c.stats()["kernel_variant"] == want, n
    # 4 logical ranks of a small system: every rank owns <= 12288 bodies, so every rank steps with one launch; bit-equal to one context
    n = 4099
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, use_graph=2) as c, nbx.Group(n, 32, n_ranks=4, devices=[0] * 4) as g:
        c.upload(ic)
        g.upload(ic)
        assert g.info(1)[2]["kernel_variant"] == nbx.KERNEL_JLANE
        k1, k2 = c.step(25), g.step(25)
        d1, d2 = c.download(), g.download()
    assert abs(k1 / k2 - 1.0) < 1e-13
    for f in d1:
        assert np.array_equal(d1[f], d2[f]), f


# ---- kinetic-energy traces against the reference's own output -----------------------------------
def _trace(nbx, n, steps, precision=32, **opts):
    with nbx.Context(n, precision, **opts) as c:
        c.upload(nbx.initial_conditions(n, precision))
        ke = c.step_trace(steps)
        fin = c.download()
    return ke, fin


def _dump(name, obj):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, name), "w") as f:
        json.dump(obj, f)


@pytest.mark.parametrize("name", ["ver7_f32_n5_s20.json", "ver7_f32_n63_s20.json", "ver7_f32_n64_s20.json",
                                  "ver7_f32_n65_s20.json", "ver7_f32_n1000_s100.json", "ver7_f32_n4099_s40.json",
                                  "ver7_f32_n65536_s20.json"])
def test_kenergy_trace_fp32_small_and_ragged(nbx, name):
    g = load_golden(name)
    ke, fin = _trace(nbx, g["n"], g["nsteps"])
    err = rel_err(ke, g["kenergy"])
    assert err.max() < 1e-5, err.max()
    k = len(g["final"]["pos_x"]["first"])
    assert np.allclose(fin["pos_x"][:k], g["final"]["pos_x"]["first"], rtol=1e-4, atol=1e-6)
    assert np.allclose(fin["vel_z"][:k], g["final"]["vel_z"]["first"], rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("name,steps,shape", [
    ("ver7_f32_n65536_s20.json", 20, dict(bodies_per_lane=1, inner_loop=2)),   # two j records per packed operation, one workgroup per CU
    ("ver7_f32_n65536_s20.json", 20, dict(bodies_per_lane=2, inner_loop=4)),   # two bodies per lane + L2 prefetch, 256-record trips
    ("ver7_f32_n65536_s20.json", 20, dict(bodies_per_lane=4, inner_loop=4)),
    ("ver7_f32_n4099_s40.json", 40, dict(bodies_per_lane=1, inner_loop=2)),    # ragged n: 17 workgroups, padding records in the last trip
    ("ver7_f32_n1000_s100.json", 100, dict(bodies_per_lane=1, inner_loop=2)),
    ("ver7_f32_n16384_s500.json", 200, dict(bodies_per_lane=1, inner_loop=2)),  # configs[1]'s size up to where it turns chaotic
    ("ver7_f32_n262144_s7.json", 7, dict(bodies_per_lane=1, inner_loop=2)),     # four workgroups per CU: the loop off its home ground
])
def test_round4_loops_against_the_reference_binary_s_own_traces(nbx, name, steps, shape):
    """The loops added in round 4 -- one body per lane with two j records per packed operation, and the L2-prefetch variant of the two- /
    four-bodies-per-lane loop -- are bit-equal to the other reference-order shapes (tested elsewhere); here they face the REFERENCE:
    per-step kenergy of its own binary (tests/golden/, oracle/gen_golden.py) within 1e-5 in reference summation order."""
    g = load_golden(name)
    ke, fin = _trace(nbx, g["n"], steps, summation_order=nbx.ORDER_REFERENCE, kernel_variant=nbx.KERNEL_SGPR, **shape)
    err = rel_err(ke, g["kenergy"][:steps])
    assert err.max() < 1e-5, (int(err.argmax()) + 1, err.max())
    if steps == g["nsteps"]:
        k = len(g["final"]["pos_x"]["first"])
        assert np.allclose(fin["pos_x"][:k], g["final"]["pos_x"]["first"], rtol=1e-4, atol=1e-6)


def test_kenergy_trace_config0_n2000_s500(nbx):
    """BASELINE.json configs[0]: kenergy at every step (not only the 10 printed ones) within 1e-4."""
    g = load_golden("ver7_f32_n2000_s500.json")
    ke, _ = _trace(nbx, 2000, 500)
    err = rel_err(ke, g["kenergy"])
    _dump("parity_n2000_s500.json", {"max_rel": float(err.max()), "printed": [float(err[s - 1]) for s in range(50, 501, 50)]})
    assert err.max() < 1e-4, err.max()
    printed = [float("%.5g" % ke[s - 1]) for s in range(50, 501, 50)]
    assert printed == [0.1432, 2.4341, 8.1256, 17.877, 32.966, 55.786, 91.132, 150.12, 264.78, 571.53]


@pytest.mark.parametrize("variant", [0, 1], ids=["default-sgprw", "lds-tile-256"])
def test_kenergy_trace_config1_n16384_s500(nbx, variant):
    """BASELINE.json configs[1] ("LDS j-tile=256" is variant 1; the default kernel is variant 0).  The system is chaotic after the bounce (step ~53): two builds of the
    reference itself drift to 1.3e-4 by step 450, so the gate is 1e-4 on every
    printed step (s = 50..500) and on all of the first 200 steps, and a loose 2e-3 bound on the unprinted late
    steps; the whole error-vs-step curve is written to gpurun_out/ and summarised in DESIGN.md."""
    g = load_golden("ver7_f32_n16384_s500.json")
    ke, _ = _trace(nbx, 16384, 500, kernel_variant=variant)
    err = rel_err(ke, g["kenergy"])
    _dump("parity_n16384_s500%s.json" % ("_lds" if variant == 1 else ""), {"max_rel": float(err.max()), "per_step": [float(e) for e in err]})
    printed = {s: float(err[s - 1]) for s in range(50, 501, 50)}
    assert err[:200].max() < 1e-4, err[:200].max()
    assert max(printed.values()) < 1e-4, printed          # the north-star gate: every printed step
    assert err.max() < 2e-3, err.max()                    # unprinted late steps: chaotic drift, bounded


def test_config1_launch_shape_is_frozen(nbx):
    """VERDICT r2 item 4a.  configs[1] runs 450 steps past the bounce; which side of 1e-4 a late printed row lands on depends
    on the summation tree (profiles/r02_config1_by_kernel.txt: SGPRW 7.7e-5, LDS 8.5e-5, jlane 1.7e-4 at the same step).  The
    shape that passes is therefore part of the contract for n = 16384: a retune of csrc/nbx_plan.hpp that changes ANY of these must
    come with test_kenergy_trace_config1_n16384_s500 still green -- this test makes such a change visible instead of silent."""
    with nbx.Context(16384) as c:
        st = c.stats()
    assert st["cu_count"] == 256
    got = {k: st[k] for k in ("kernel_variant", "bodies_per_lane", "j_split", "inner_loop", "summation_order", "fused_epilogue", "force_grid_x", "force_grid_y")}
    assert got == {"kernel_variant": nbx.KERNEL_SGPRW, "bodies_per_lane": 4, "j_split": 32, "inner_loop": nbx.LOOP_ASM, "summation_order": nbx.ORDER_TREE,
                   "fused_epilogue": 0, "force_grid_x": 64, "force_grid_y": 32}, got


@pytest.mark.parametrize("n,S,grid_x", [(16384, 32, 64), (20000, 16, 79), (24576, 8, 96), (32768, 4, 128), (49152, 4, 192),
                                        (50000, 32, 196), (65536, 2, 256), (98304, 2, 384), (131072, 1, 512)])
def test_balanced_j_split_rule(nbx, n, S, grid_x):
    """Round 3: tree-order shapes above 16384 owned bodies take the j-split that loads every CU evenly with
    the fewest slabs (csrc/nbx_plan.hpp: balanced_j_split; measured in profiles/r03_band_sweep.txt), in whole 256-record tiles so
    that the hand-scheduled loop serves every n; up to 16384 the round-1 rule stays (configs[1]'s tree is pinned)."""
    with nbx.Context(n) as c:
        st = c.stats()
    assert st["kernel_variant"] == nbx.KERNEL_SGPRW and st["summation_order"] == nbx.ORDER_TREE and st["bodies_per_lane"] == 4
    assert (st["j_split"], st["force_grid_x"], st["force_grid_y"]) == (S if n != 50000 else st["j_split"], grid_x, st["j_split"]), st
    if n > 16384:
        assert st["inner_loop"] == nbx.LOOP_ASM  # also for n = 50000, whose 32 splits of 1568 records used to fall back to the compiled loop
    if n == 50000:
        assert st["j_split"] == 28  # 32 asked for by the cost model; 28 whole-tile splits of 1792 records cover the 50176 records


def test_config1_divergence_curve_beside_the_reference_vs_reference_spread(nbx):
    """configs[1] against TWO builds of the reference's unmodified source -- the pinned -O2 build (the
    oracle) and the -O3 / AVX2 / FMA build (tests/golden/ver7_f32o3_n16384_s500.json).  The north-star gate (1e-4 on the rows
    the program prints) is asserted against the pinned build by test_kenergy_trace_config1_n16384_s500; here the whole curve
    is put beside the reference-vs-reference spread: over all 500 steps the GPU is no farther from the pinned build than
    1.5x the largest distance between the two reference builds (measured: 3.7e-4 vs 3.0e-4), and it leaves the 1e-5 band
    no earlier than 50 steps before they leave it with respect to each other."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g, g2 = load_golden("ver7_f32_n16384_s500.json"), load_golden("ver7_f32o3_n16384_s500.json")
    ke, _ = _trace(nbx, 16384, 500)
    d = bench.divergence_vs_reference_builds([float(x) for x in ke], g["kenergy"], g2["kenergy"])
    _dump("config1_divergence.json", d)
    m = d["max_over_all_steps"]
    assert d["max_over_printed_rows"]["gpu_vs_pinned_build"] < 1e-4
    assert m["gpu_vs_pinned_build"] < 1.5 * m["second_build_vs_pinned_build"], m
    f = d["first_step_above_1e-5"]
    assert f["gpu_vs_pinned_build"] > f["second_build_vs_pinned_build"] - 50, f


def test_kenergy_trace_config2_n262144_first_steps(nbx):
    """BASELINE.json configs[2] (n=262144): the reference needs ~65 s per step in the build container, so the
    fixture holds its first 7 steps (they agree with the 7 the survey captured)."""
    g = load_golden("ver7_f32_n262144_s7.json")
    ke, _ = _trace(nbx, 262144, 7)
    err = rel_err(ke, g["kenergy"])
    _dump("parity_n262144_s7.json", {"per_step": [float(e) for e in err]})
    assert err.max() < 1e-4, err


@pytest.mark.parametrize("name,tol", [("ver7_f64_n5_s20.json", 1e-12), ("ver7_f64_n2000_s500.json", 1e-10),
                                      ("ver7_f64_n4099_s40.json", 1e-11), ("ver7_f64_n16384_s60.json", 1e-10),
                                      ("ver7_f64_n262144_s3.json", 1e-10)])  # the last one IS BASELINE.json configs[4]
def test_kenergy_trace_fp64(nbx, name, tol):
    g = load_golden(name)
    ke, _ = _trace(nbx, g["n"], g["nsteps"], 64)
    err = rel_err(ke, g["kenergy"])
    _dump("parity_" + name, {"max_rel": float(err.max())})
    assert err.max() < tol, err.max()


# ---- C-ABI contract on the device (T3) ----------------------------------------------------------
def test_step_k_equals_k_single_steps_and_is_deterministic(nbx):
    n = 3000
    ic = nbx.initial_conditions(n)
    with nbx.Context(n) as a, nbx.Context(n) as b, nbx.Context(n) as c:
        for x in (a, b, c):
            x.upload(ic)
        ka = a.step(25)
        for _ in range(25):
            kb = b.step(1)
        kc = c.step_trace(25)[-1]
        assert ka == kb == kc
        da, db = a.download(), b.download()
        for f in da:
            assert np.array_equal(da[f], db[f]), f


@pytest.mark.parametrize("n,steps", [(2000, 50), (2000, 7), (777, 45), (4099, 23), (16384, 4), (2000, 120), (16384, 101)])
def test_graph_replay_is_bit_equal_to_plain_launches(nbx, n, steps):
    """nbx_step replays launch-bound windows from a hipGraph; it must be the same launches, same bits."""
    ic = nbx.initial_conditions(n)
    out = []
    for g in (1, 2):
        with nbx.Context(n, use_graph=g) as c:
            c.upload(ic)
            k1 = c.step(steps)
            k2 = c.step(steps)       # second call starts from the other buffer parity when steps is odd
            c.step(3, kenergy=False)
            k3 = c.step(0)
            st = c.stats()
            out.append((k1, k2, k3, c.download(), st))
    assert out[0][4]["use_graph"] == 1 and out[0][4]["graph_replays"] >= 2 and out[1][4]["graph_replays"] == 0
    assert out[0][4]["steps_done"] == out[1][4]["steps_done"] == 2 * steps + 3
    assert out[0][:3] == out[1][:3]
    for f in out[0][3]:
        assert np.array_equal(out[0][3][f], out[1][3][f]), f


def test_upload_download_roundtrip_and_state_errors(nbx):
    n = 777
    ic = nbx.initial_conditions(n)
    with nbx.Context(n) as c:
        with pytest.raises(nbx.NbxError) as e:
            c.step(1)
        assert e.value.code == nbx.NBX_ERR_STATE
        c.upload(ic)
        d = c.download()
        for f in d:
            assert np.array_equal(d[f], ic[f]), f
        assert c.step(0) == 0.0  # no step since the upload: there is no energy to report yet
        ke1 = c.step(3)
        assert c.step(0) == ke1  # zero further steps: the energy after the last one, again
        # a fresh upload starts a new trajectory: the partial sums of the old one must not leak into it
        c.upload(ic)
        assert c.step(0) == 0.0 and c.kenergy_partial() == 0.0
        assert c.step(3) == ke1
        with pytest.raises(nbx.NbxError):
            c.commit()
    with nbx.Context(n, i_begin=0, i_count=100, n_alloc=1024) as c:
        c.upload(ic)
        with pytest.raises(nbx.NbxError) as e:
            c.step(1)
        assert e.value.code == nbx.NBX_ERR_STATE


@pytest.mark.parametrize("n,kernel", [(777, 0), (2304, 0), (16384, 0), (16384, 1)])
def test_reupload_then_cached_graph_replay_still_reports_the_energy(nbx, n, kernel):
    """upload; step(10); upload; step(10) with graph replay on.  The second step(10) enqueues nothing through
    enqueue_step (the window's graph is cached), so the count of energy partials has to come from the replay itself --
    it used to stay at the zero nbx_upload leaves and the energy came back as 0.0."""
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, use_graph=1, kernel_variant=kernel) as c:
        c.upload(ic)
        ke1 = c.step(10)
        assert c.stats()["graph_replays"] == 1 and ke1 > 0.0
        c.upload(ic)
        assert c.step(0) == 0.0
        ke2 = c.step(10)
        assert c.stats()["graph_replays"] == 2
        assert ke2 == ke1
        assert c.step(0) == ke1 and 0.5 * c.kenergy_partial() == ke1
    with nbx.Context(n, use_graph=2, kernel_variant=kernel) as c:  # plain launches: the same number
        c.upload(ic)
        assert c.step(10) == ke1


def test_stats_and_profile(nbx):
    n = 8192
    with nbx.Context(n) as c:
        c.upload(nbx.initial_conditions(n))
        c.profile(True)
        c.step(10)
        st = c.stats()
    assert st["steps_done"] == 10 and st["force_launches_timed"] == 10 and st["force_ms_total"] > 0
    assert st["cu_count"] == 256 and st["pairs_per_launch"] == float(n) * n
    assert "gfx950" in st["device_name"] or "MI355" in st["device_name"]


# ---- sharded stepping: P logical ranks on ONE device, exchange by device-to-device copies --------
def _hip():
    import ctypes
    return ctypes.CDLL("libamdhip64.so.7")


@pytest.mark.parametrize("n,P", [(2000, 2), (4099, 4), (16384, 8)])
def test_logical_ranks_bit_equal_to_single_context(nbx, n, P):
    """T5: the block partition + all-gather scheme gives the SAME BITS as one context, provided the
    global j order is the same (same j_split over the same n_alloc)."""
    import ctypes
    import sharded
    hip = _hip()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ic = nbx.initial_conditions(n)
    steps = 12
    block, _, _, n_alloc = sharded.block_partition(n, P, 0)
    shape = dict(j_split=4, bodies_per_lane=2, n_alloc=n_alloc)
    with nbx.Context(n, **shape) as one:
        one.upload(ic)
        ke_one = one.step_trace(steps)
        ref = one.download()
    ranks = []
    for r in range(P):
        _, ib, ic_, na = sharded.block_partition(n, P, r)
        c = nbx.Context(n, i_begin=ib, i_count=ic_, **shape)
        c.upload(ic)
        ranks.append(c)
    ke = []
    for _ in range(steps):
        for c in ranks:
            c.step_local()
        bufs = [c.exchange_buffer() for c in ranks]
        for c in ranks:
            c.sync()
        for r, (ptr_r, tot, off, own) in enumerate(bufs):  # "all-gather": everyone receives r's block
            for q, (ptr_q, _, _, _) in enumerate(bufs):
                if q != r and own:
                    assert hip.hipMemcpy(ptr_q + off, ptr_r + off, own, 3) == 0
        for c in ranks:
            c.commit()
        ke.append(0.5 * sum(c.kenergy_partial() for c in ranks))
    got = {f: np.zeros(n, dtype=np.float32) for f in ref}
    for c in ranks:
        d = c.download()
        st = c.stats()
        sl = slice(st["i_begin"], st["i_begin"] + st["i_count"])
        for f in ("vel_x", "vel_y", "vel_z"):
            got[f][sl] = d[f][sl]
        for f in ("pos_x", "pos_y", "pos_z"):
            assert np.array_equal(d[f], ref[f]), (f, st["i_begin"])
        c.close()
    for f in ("vel_x", "vel_y", "vel_z"):
        assert np.array_equal(got[f], ref[f]), f
    assert rel_err(ke, ke_one).max() < 1e-12  # partial sums are regrouped across ranks, nothing else


def test_sharded_simulation_single_rank_matches_context(nbx):
    import sharded
    n = 5000
    ic = nbx.initial_conditions(n)
    sim = sharded.ShardedSimulation(n, 32, dist=None, j_split=4, bodies_per_lane=2)
    sim.upload(ic)
    sim.step(10)
    ke = sim.kenergy()
    with nbx.Context(n, j_split=4, bodies_per_lane=2) as c:
        c.upload(ic)
        assert c.step(10) == ke
    sim.close()


# ---- full-size, size-independent properties (n = 262144, where the oracle needs minutes) ---------
@pytest.fixture(scope="module")
def big(nbx):
    n = 262144
    ic = nbx.initial_conditions(n)
    # tree order: these fixtures are compared with fp64 "truth"; the reference order (default at this size) carries the
    # reference's own ~1e-5 summation noise by design (see the summation-order tests below)
    with nbx.Context(n, summation_order=2) as c:
        c.upload(ic)
        acc = c.accel()
    return n, ic, acc


def test_fullsize_newton_third_law(big):
    """sum_i m_i a_i = 0 for pairwise forces (antisymmetric pair terms), to fp32 rounding."""
    n, ic, (ax, ay, az) = big
    m = ic["mass"].astype(np.float64)
    for a in (ax, ay, az):
        f = m * a.astype(np.float64)
        assert abs(f.sum()) / np.abs(f).sum() < 2e-6


def test_fullsize_mass_scaling_is_exact(nbx, big):
    """a is linear in the masses; scaling every mass by 2 (a power of two) must double every bit pattern."""
    n, ic, (ax, ay, az) = big
    ic2 = dict(ic)
    ic2["mass"] = ic["mass"] * np.float32(2)
    with nbx.Context(n, summation_order=nbx.ORDER_TREE) as c:
        c.upload(ic2)
        bx, by, bz = c.accel()
    assert np.array_equal(bx, ax * np.float32(2)) and np.array_equal(by, ay * np.float32(2)) and np.array_equal(bz, az * np.float32(2))


def test_fullsize_sampled_bodies_vs_fp64_direct_sum(big):
    """64 sampled bodies against a float64 numpy direct sum over all 262144 sources."""
    n, ic, (ax, ay, az) = big
    x, y, z = (ic[k].astype(np.float64) for k in ("pos_x", "pos_y", "pos_z"))
    gm = float(np.float32(6.67259e-11)) * ic["mass"].astype(np.float64)
    eps = float(np.float32(1e-3))
    rng = np.random.default_rng(1)
    scale = max(np.abs(ax).max(), np.abs(ay).max(), np.abs(az).max())
    for i in rng.integers(0, n, 64):
        dx, dy, dz = x - x[i], y - y[i], z - z[i]
        inv3 = (dx * dx + dy * dy + dz * dz + eps) ** -1.5 * gm
        assert abs((dx * inv3).sum() - ax[i]) / scale < 1e-5
        assert abs((dz * inv3).sum() - az[i]) / scale < 1e-5


def test_fullsize_1m_bodies_config3_properties(nbx):
    """BASELINE.json configs[3]'s body count on one GPU (the CPU reference needs ~4 min per step here): Newton's third
    law, 32 sampled bodies against an fp64 direct sum, and one time step's kinetic energy against the fp64 evaluation of
    the same Euler update from those sampled accelerations' full-array counterpart."""
    n = 1048576
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, summation_order=nbx.ORDER_TREE) as c:   # compared with fp64 truth: see the `big` fixture's note
        c.upload(ic)
        ax, ay, az = c.accel()
        ke1 = c.step(1)
    m = ic["mass"].astype(np.float64)
    for a in (ax, ay, az):
        f = m * a.astype(np.float64)
        assert abs(f.sum()) / np.abs(f).sum() < 2e-6
    x, y, z = (ic[k].astype(np.float64) for k in ("pos_x", "pos_y", "pos_z"))
    gm = float(np.float32(6.67259e-11)) * m
    eps = float(np.float32(1e-3))
    scale = max(np.abs(ax).max(), np.abs(ay).max(), np.abs(az).max())
    for i in np.random.default_rng(5).integers(0, n, 32):
        dx, dy, dz = x - x[i], y - y[i], z - z[i]
        inv3 = (dx * dx + dy * dy + dz * dz + eps) ** -1.5 * gm
        assert abs((dy * inv3).sum() - ay[i]) / scale < 1e-5
    dt = nbx.DT
    vx, vy, vz = (ic[k].astype(np.float64) + a.astype(np.float64) * dt for k, a in (("vel_x", ax), ("vel_y", ay), ("vel_z", az)))
    ke_ref = 0.5 * float((m * (vx * vx + vy * vy + vz * vz)).sum())
    assert abs(ke1 - ke_ref) / ke_ref < 1e-5


@pytest.mark.parametrize("order", ["reference", "tree"])
def test_beyond_the_largest_baseline_size_4m_bodies(nbx, order):
    """n = 4194304 = four times BASELINE's largest body count (configs[3]): 64-MiB record array, 16384 workgroups in reference order,
    indices and byte offsets past 2^26.  No reference run exists at this size (hours per step); what is checked is size-independent:
    Newton's third law over all bodies; sampled bodies against an fp64 direct sum; and, in reference order, two slices of 2048
    bodies (the first and the last) against NBX_KERNEL_EXACT -- the reference's arithmetic bit for bit -- run on those slices only.
    That last check is the one that matters there: ONE fp32 accumulator over 4194304 terms is 1-3e-3 of |a|inf away from the true
    sum (each term is ~2 ulp of the running sum; 8e-6 at n = 262144), and the fast kernel reproduces exactly that
    (6e-7 against exact mode over all 4194304 bodies, measured once; 2.7e-3 between exact mode and a 32 x 4-chain tree)."""
    n = 4194304
    ic = nbx.initial_conditions(n)
    o = nbx.ORDER_REFERENCE if order == "reference" else nbx.ORDER_TREE
    with nbx.Context(n, summation_order=o) as c:
        c.upload(ic)
        ax, ay, az = c.accel()
        st = c.stats()
    assert st["n_alloc"] == n and st["summation_order"] == o
    m = ic["mass"].astype(np.float64)
    for a in (ax, ay, az):
        f = m * a.astype(np.float64)
        assert abs(f.sum()) / np.abs(f).sum() < (2e-5 if order == "reference" else 2e-6)
    x, y, z = (ic[k].astype(np.float64) for k in ("pos_x", "pos_y", "pos_z"))
    gm = float(np.float32(6.67259e-11)) * m
    eps = float(np.float32(1e-3))
    scale = max(np.abs(ax).max(), np.abs(ay).max(), np.abs(az).max())
    for i in np.concatenate([np.random.default_rng(11).integers(0, n, 10), [0, n - 1]]):
        dx, dy, dz = x - x[i], y - y[i], z - z[i]
        inv3 = (dx * dx + dy * dy + dz * dz + eps) ** -1.5 * gm
        for d, a in ((dx, ax), (dy, ay), (dz, az)):
            # tree order at this size = four chains of 1048576 terms per body (one j range per workgroup, the four waves' quarters):
            # 6e-5 measured -- 30x closer to the true sum than the single chain, not the 1e-6 of the 32 x 4 chains of small n
            assert abs((d * inv3).sum() - a[i]) / scale < (5e-3 if order == "reference" else 2e-4), (i, order)
    if order == "reference":
        for i0 in (0, n - 2048):
            with nbx.Context(n, kernel_variant=nbx.KERNEL_EXACT, i_begin=i0, i_count=2048, n_alloc=n) as c:
                c.upload(ic)
                ex, ey, ez = c.accel()
            sl = slice(i0, i0 + 2048)
            for a, e in ((ax, ex), (ay, ey), (az, ez)):
                assert np.abs(a[sl] - e[sl]).max() / scale < 3e-6, i0


def test_fullsize_tree_sums_are_closer_to_the_true_sum_than_the_reference_arithmetic(nbx, big):
    """At n = 262144 the reference adds 262144 fp32 terms per body one after the other; that sum carries ~1e-5 of
    rounding error by itself (NBX_KERNEL_EXACT reproduces it bit for bit, the reference-order fast kernel to ~1e-6).
    The tree of partial sums (summation_order = TREE) is MORE accurate: measured against an fp64 direct sum on 48 bodies.
    Which of the two a run should use is a parity question, not an accuracy one: see DESIGN.md "Summation order"."""
    n, ic, _ = big
    with nbx.Context(n, summation_order=nbx.ORDER_TREE) as c:
        c.upload(ic)
        ax, ay, az = c.accel()
        st = c.stats()  # on request at this size (AUTO takes reference order): 8 j-splits x 4 wave chains per body
        assert st["summation_order"] == nbx.ORDER_TREE and st["j_split"] == 8 and st["kernel_variant"] == nbx.KERNEL_SGPRW
    with nbx.Context(n, kernel_variant=nbx.KERNEL_EXACT) as c:
        c.upload(ic)
        ex, ey, ez = c.accel()
    with nbx.Context(n, summation_order=nbx.ORDER_REFERENCE) as c:   # the default at this size
        c.upload(ic)
        rx, ry, rz = c.accel()
        assert c.stats()["summation_order"] == nbx.ORDER_REFERENCE and c.stats()["j_split"] == 1
    # reference-order fast kernel: same summation order as the reference => same rounding noise, to ~1e-6 of |a|inf
    sc = max(np.abs(ex).max(), np.abs(ey).max(), np.abs(ez).max())
    assert max(np.abs(rx - ex).max(), np.abs(ry - ey).max(), np.abs(rz - ez).max()) / sc < 3e-6
    x, y, z = (ic[k].astype(np.float64) for k in ("pos_x", "pos_y", "pos_z"))
    gm = float(np.float32(6.67259e-11)) * ic["mass"].astype(np.float64)
    eps = float(np.float32(1e-3))
    e_fast, e_exact = [], []
    for i in np.random.default_rng(3).integers(0, n, 48):
        dx, dy, dz = x - x[i], y - y[i], z - z[i]
        inv3 = (dx * dx + dy * dy + dz * dz + eps) ** -1.5 * gm
        t = np.array([(dx * inv3).sum(), (dy * inv3).sum(), (dz * inv3).sum()])
        nt = np.abs(t).max()
        e_fast.append(np.abs(np.array([ax[i], ay[i], az[i]], dtype=np.float64) - t).max() / nt)
        e_exact.append(np.abs(np.array([ex[i], ey[i], ez[i]], dtype=np.float64) - t).max() / nt)
    _dump("accuracy_vs_fp64_n262144.json", {"fast_median": float(np.median(e_fast)), "fast_max": float(np.max(e_fast)),
                                            "reference_arithmetic_median": float(np.median(e_exact)),
                                            "reference_arithmetic_max": float(np.max(e_exact))})
    assert np.median(e_fast) < np.median(e_exact)
    assert np.max(e_fast) < 2e-5


def test_fullsize_padding_bodies_are_inert(nbx):
    """n = 262144 - 37 (ragged tail tile): appending zero-mass bodies must not change anything."""
    n = 262144 - 37
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, j_split=8, bodies_per_lane=8) as c:
        c.upload(ic)
        a1 = c.accel()
    with nbx.Context(n, j_split=8, bodies_per_lane=8, n_alloc=262144 + 2048) as c:
        c.upload(ic)
        a2 = c.accel()
    # same split count but different split boundaries: agree to rounding, not bitwise
    scale = np.abs(a1[0]).max()
    assert np.abs(a1[0] - a2[0]).max() / scale < 1e-5


# ---- the product engine under torch.distributed (rehearsals possible on a 1-GPU box) ------------
def _run_ranks(tmp_path, n, steps, world, backend, weights=None):
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    out = str(tmp_path / "res")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    if weights:
        env["NBX_TEST_WEIGHTS"] = weights
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", port,
           os.path.join(ROOT, "tests", "_dist_gpu_worker.py"), str(n), str(steps), out, backend]
    p = subprocess.run(cmd, env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return [json.load(open("%s.%d" % (out, r))) for r in range(world)]


@pytest.mark.parametrize("world,backend", [(2, "gloo"), (3, "gloo"), (1, "nccl")])
def test_product_engine_under_torch_distributed(nbx, tmp_path, world, backend):
    """NbxEngine + ShardedSimulation end to end: device buffer aliased as a torch tensor, context on torch's
    stream, in-place all-gather, energy all-reduce.  gloo: `world` ranks share cuda:0 (exchange staged through the
    host); nccl: a 1-rank RCCL group with the collectives forced on.  Must be bit-equal to a single context."""
    import sharded
    n, steps = 3001, 8
    res = _run_ranks(tmp_path, n, steps, world, backend)
    n_alloc = sharded.block_partition(n, world, 0)[3]
    with nbx.Context(n, j_split=4, bodies_per_lane=2, n_alloc=n_alloc) as c:
        c.upload(nbx.initial_conditions(n))
        ke = c.step_trace(steps)
        px = c.download()["pos_x"]
    for r in res:
        assert r["world"] == world and r["n_alloc"] == n_alloc
        assert r["pos_x"] == px.tolist()[:64] + px.tolist()[-64:]
        assert rel_err(r["ke"], ke).max() < 1e-12
    assert sum(r["i_count"] for r in res) == n


def test_product_engine_with_unequal_shares_under_torch_distributed(nbx, tmp_path):
    """ShardedSimulation(weights=[1, 2, 1]) with the product engine: three ranks sharing cuda:0 over gloo, shares 768 / 1536 / 697 bodies,
    one broadcast per owner and step -- bit-equal to one context in reference order."""
    n, steps = 3001, 8
    res = _run_ranks(tmp_path, n, steps, 3, "gloo", weights="1,2,1")
    with nbx.Context(n, summation_order=nbx.ORDER_REFERENCE) as c:
        c.upload(nbx.initial_conditions(n))
        ke = c.step_trace(steps)
        px = c.download()["pos_x"]
    assert [r["i_count"] for r in res] == [768, 1536, 697] and all(r["n_alloc"] == 3072 for r in res)
    for r in res:
        assert r["pos_x"] == px.tolist()[:64] + px.tolist()[-64:]
        assert rel_err(r["ke"], ke).max() < 1e-12


# ---- T6: the drop-in executables -----------------------------------------------------------------
def _run_cli(exe, *args, env=None):
    import subprocess
    path = os.path.join(ROOT, "nbody-demo-2023_amd", "host", exe)
    p = subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout.splitlines(), p.stderr


def _rows(lines):
    import re
    out = []
    for ln in lines:
        m = re.match(r"^ (\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", ln)
        if m:
            out.append(m.groups())
    return out


def test_cli_default_run_prints_the_reference_table():
    """`./nbody.x` (no arguments) = the reference's default 2000 x 500: same frame, same 5-digit kenergy column
    as the unmodified ver7 binary prints, 0 exit status."""
    rc, lines, _ = _run_cli("nbody.x")
    assert rc == 0
    assert lines[0] == "=" * 31 and lines[1] == " Initialize Gravity Simulation"
    assert lines[2] == " nPart = 2000; nSteps = 500; dt = 0.1"
    assert lines[3] == "-" * 48 and lines[5] == "-" * 48
    assert lines[4] == " " + "s".ljust(8) + "dt".ljust(8) + "kenergy".ljust(12) + "time (s)".ljust(12) + "GFlops".ljust(12)
    rows = _rows(lines)
    assert [r[0] for r in rows] == [str(s) for s in range(50, 501, 50)]
    assert [r[1] for r in rows] == ["5", "10", "15", "20", "25", "30", "35", "40", "45", "50"]
    assert [r[2] for r in rows] == ["0.1432", "2.4341", "8.1256", "17.877", "32.966", "55.786", "91.132", "150.12", "264.78", "571.53"]
    assert all(len(ln) == 53 for ln in lines[6:16])              # 1 + 8 + 8 + 12 + 12 + 12, left aligned
    i = lines.index("", 16)
    assert lines[i + 1].startswith("# Number Threads     : ")
    assert lines[i + 2].startswith("# Total Time (s)     : ")
    assert lines[i + 3].startswith("# Average Perfomance : ") and " +- " in lines[i + 3]
    assert lines[i + 4] == "=" * 31
    assert lines[i + 5].startswith("# Device") and lines[i + 6].startswith("# Pair rate")


def test_cli_json_summary(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    out = str(tmp_path / "run.json")
    p = subprocess.run([exe, "2000", "200"], env=dict(os.environ, NBODY_JSON=out), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0
    d = json.load(open(out))
    assert d["n"] == 2000 and d["steps"] == 200 and d["precision"] == 32 and d["ranks"] == 1 and d["kernel"] == "jlane"
    assert abs(d["kenergy_last_printed"] - 17.877) < 1e-3 and d["pair_per_s_total"] > 1e9


def test_cli_argument_quirks_of_ver7_main():
    # one argument: particles only; three arguments: the step count is silently ignored (argc == 3 test, ver7/main.cpp:36)
    rc, lines, _ = _run_cli("nbody.x", 1000)
    assert rc == 0 and lines[2] == " nPart = 1000; nSteps = 500; dt = 0.1"
    rc, lines, _ = _run_cli("nbody.x", 1000, 100, "extra")
    assert rc == 0 and lines[2] == " nPart = 1000; nSteps = 500; dt = 0.1"
    rc, lines, _ = _run_cli("nbody.x", 1000, 120)
    rows = _rows(lines)
    assert rc == 0 and [r[0] for r in rows] == ["50", "100"]       # trailing 20 steps run, not printed
    assert any("nan" in ln for ln in lines if ln.startswith("# Average"))  # nf <= 2: the reference prints nan too
    g = load_golden("ver7_f32_n1000_s100.json")
    assert rows[1][2] == "%.5g" % np.float32(g["kenergy"][99])


def test_cli_fp64_and_ver5_front_end(tmp_path):
    import subprocess
    out = str(tmp_path / "fp64.json")
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody_fp64.x")
    p = subprocess.run([exe, "2000", "100"], env=dict(os.environ, NBODY_JSON=out), capture_output=True, text=True, timeout=300)
    rc, lines = p.returncode, p.stdout.splitlines()
    g = load_golden("ver7_f64_n2000_s500.json")
    rows = _rows(lines)
    assert rc == 0 and rows[1][2] == "%.5g" % g["kenergy"][99] and rows[0][2] == "%.5g" % g["kenergy"][49]
    # the fp64 drop-in steps with dt = (double)0.1f like the fixtures: its kenergy meets the fp64 gate, not
    # just the 5 printed digits (with the double literal 0.1 it would sit ~1e-8 away)
    d = json.load(open(out))
    assert d["precision"] == 64 and abs(d["kenergy_last_printed"] / g["kenergy"][99] - 1.0) < 1e-10
    rc, lines, err = _run_cli("nbody_v5.x", 2000, 100, "gpu", 0.5, 256, 2)
    assert rc == 0 and lines[0] == "gpu" and lines[1] == "=" * 31
    assert _rows(lines)[1][2] == "2.4341"
    assert any("bodies/lane 2" in ln for ln in lines)
    # the frame of the reference's HIP build, line for line up to the first row (hip/Compute.cpp:140 prints the block size
    # between the header and the table's first row)
    assert lines[:8] == ["gpu", "=" * 31, " Initialize Gravity Simulation", " nPart = 2000; nSteps = 100; dt = 0.1", "-" * 48,
                         " s       dt      kenergy     time (s)    GFlops      ", "-" * 48, "using block_size = 256"], lines[:8]
    assert lines[8].split()[0] == "50" and err == ""
    rc, lines, err = _run_cli("nbody_v5.x", 2000, 50, "gpu", 0.5, 1024, 2)
    assert rc == 0 and "using block_size = 256" in lines and "thread_dim0 = 1024 ignored" in err
    rc, lines, err = _run_cli("nbody.x", 2000, 50)  # the ver7 drop-in has no such line (ver7 never prints one)
    assert rc == 0 and not any("block_size" in ln for ln in lines)
    rc, lines, err = _run_cli("nbody_v5.x", 2000, 100, "cpu")
    assert rc == 1 and "no CPU engine" in err


def test_cli_cpu_plus_gpu_maps_onto_unequal_shares_and_the_tuner(tmp_path):
    """ver5_all's `cpu+gpu <cpu_ratio>` (ver5_all/main.cpp:40-54 -> opencl/Compute.cpp:154-162,241-255,317-321).  One GPU: nothing to
    split -- all bodies on the GPU, and the user is TOLD so where the results are (the `#` lines behind the footer, NBODY_JSON), not
    only on stderr; a cpu_ratio of 0.3 and of 0.9 give the same run and say so.  NBODY_GPUS=2 (logical ranks on the one device here):
    device 0 owns the share cpu_ratio, exactly the reference's arithmetic for two devices, in whole 256-record tiles; a negative
    ratio is the reference's tuning mode: its `cpu/gpu ratio = ...` line in front of every printed row, shares re-weighted from the
    measured force-kernel times.  Results do not depend on the shares (rows equal those of the plain run)."""
    rc, base, _ = _run_cli("nbody_v5.x", 16384, 100, "gpu")
    assert rc == 0
    j1 = str(tmp_path / "one.json")
    rc, lines, err = _run_cli("nbody_v5.x", 16384, 100, "cpu+gpu", 0.3, env={"NBODY_JSON": j1})
    assert rc == 0 and [r[2] for r in _rows(lines)] == [r[2] for r in _rows(base)]
    note = [ln for ln in lines if ln.startswith("# Device word")]
    assert len(note) == 1 and "all bodies on the GPU" in note[0] and "cpu_ratio ignored" in note[0] and "cpu_ratio ignored" in err
    assert lines.index(note[0]) > lines.index("=" * 31, 2)                      # behind the reference's footer
    assert "cpu_ratio ignored" in json.load(open(j1))["device_word_note"]
    j2 = str(tmp_path / "two.json")
    rc, lines, err = _run_cli("nbody_v5.x", 16384, 100, "cpu+gpu", 0.25, env={"NBODY_GPUS": "2", "NBODY_JSON": j2})
    assert rc == 0, err
    d = json.load(open(j2))
    assert d["shares"] == "4096 12288" and d["ranks"] == 2 and not d["tuned"]
    assert any(ln.startswith("# GPUs / shares") and "4096 12288" in ln and "fixed weights" in ln for ln in lines)
    assert [r[2][:5] for r in _rows(lines)] == [r[2][:5] for r in _rows(base)]   # tree order at this n: the same to the printed digits' noise
    rc, lines, err = _run_cli("nbody.x", 16384, 100, env={"NBODY_GPUS": "3", "NBODY_WEIGHTS": "1,2,1", "NBODY_JSON": j2})   # the same without the device word
    assert rc == 0 and json.load(open(j2))["shares"] == "4096 8192 4096", err
    rc, lines, err = _run_cli("nbody.x", 16384, 100, env={"NBODY_GPUS": "3", "NBODY_WEIGHTS": "1,2"})
    assert rc == 1 and "NBODY_WEIGHTS needs 3" in err
    rc, lines, err = _run_cli("nbody_v5.x", 16384, 150, "cpu+gpu", -1, env={"NBODY_GPUS": "2", "NBODY_JSON": j2})
    assert rc == 0, err
    d = json.load(open(j2))
    assert d["tuned"] and sum(int(x) for x in d["shares"].split()) == 16384
    ratio = [ln for ln in lines if ln.startswith("cpu/gpu ratio = ")]
    assert len(ratio) == 3 and ratio[0] == "cpu/gpu ratio = 0.500000"            # one per printed row, as in the reference's tuning mode
    assert all(lines[lines.index(r) + 1].split()[0] in ("50", "100", "150") for r in ratio)


# ---- T8: bench.py contract and performance floor -------------------------------------------------
def test_bench_line_schema_and_roofline_floor():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--cpu-baseline", "port", "--full"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "pair-interactions/s" and d["unit"] == "pair/s" and d["n_gpus"] == 1 and d["steps"] == 5
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and d["higher_is_better"] is True
    assert "workload" in d["config"] and d["config"]["n_bodies"] == 262144
    r = d["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(r)
    assert r["peak"] == 157.3 and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["launches_timed"] == 5
    # value (whole step, wall clock) and the HIP-event kernel time must tell the same story
    assert abs(d["value"] * 20e-12 / r["achieved"] - 1.0) < 0.05
    assert r["frac"] > 0.40, r["frac"]                       # north_star target at n = 262144
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 1e8 and c["unit"] == "pair/s"
    assert c["cores_on_box"] >= c["cores"]
    assert d["parity"]["max_rel_kenergy_err"] < 1e-4
    # the one-GPU slice proxies of every multi-GPU cell the table will have, not only of n = 1M
    px = d["multi_gpu_slice_proxy"]
    cells = {(c["n_bodies"], c["gpus"]): c for c in px["cells"]}
    assert sorted(cells) == [(nn, P) for nn in (262144, 524288, 1048576) for P in (2, 4, 8)]
    for (nn, P), c in cells.items():
        assert c["measured"] is False and c["bodies_owned"] == nn // P and c["ms_per_step"] > 0 and "not a %d-GPU measurement" % P in c["note"]
        assert abs(c["implied_%dgpu_speedup_before_communication" % P] * c["ms_per_step"] / c["one_gpu_ms_per_step"] - 1) < 1e-9
    assert cells[(262144, 4)]["bodies_per_lane"] == 1 and cells[(262144, 4)]["inner_loop"] == "asm"    # two j records per packed operation
    assert cells[(262144, 4)]["roofline_frac"] > 0.38 and cells[(262144, 8)]["roofline_frac"] > 0.19 and cells[(1048576, 8)]["roofline_frac"] > 0.50
    assert d["one_rank_of_8_at_1m"] is cells[(1048576, 8)] or d["one_rank_of_8_at_1m"] == cells[(1048576, 8)]
    # traffic is reported only for the launch shape the committed PMC profile was taken on
    assert (r["traffic"] is not None) == (r["traffic_profiled_shape"] == r["traffic_shape_ran"]) and r["traffic_note"]


def test_bench_plain_run_and_dumped_outputs(nbx, tmp_path):
    """Without --full the line carries the headline figure and nothing that takes runs of its own; --dump-outputs writes what the
    last timed step left: the state of one context stepping the same seed-42 system warmup + steps times."""
    import subprocess
    import sys
    steps, warmup = 3, 1
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "pair-interactions/s" and d["unit"] == "pair/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["roofline"]["launches_timed"] == steps
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / float(d["config"]["n_bodies"]) ** 2 - 1) < 1e-9
    for k in ("cpu_baseline", "parity", "other_summation_order", "multi_gpu_slice_proxy", "one_gpu_at_multi_gpu_n", "ranks"):
        assert k not in d, k
    _check_dumped_outputs(nbx, tmp_path, d, warmup + steps)


def _check_dumped_outputs(nbx, dump_dir, line, nsteps):
    """bench.py --dump-outputs against one context stepping the same seed-42 system nsteps times: every body's position and
    velocity at its own index (at N > 1 each rank's velocity slice must land at its offset) and the line's kinetic energy."""
    n = line["config"]["n_bodies"]
    with nbx.Context(n, 32) as c:
        c.upload(nbx.initial_conditions(n))
        ke = c.step(nsteps)
        ref = c.download()
    assert sorted(os.listdir(dump_dir)) == sorted(f + ".npy" for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "kenergy"))
    for f, want in ref.items():
        got = np.load(dump_dir / (f + ".npy"))
        assert got.dtype == np.float32 and got.shape == (n,), (f, got.dtype, got.shape)
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-6 * np.abs(want).max(), f
    k = np.load(dump_dir / "kenergy.npy")
    assert k.dtype == np.float64 and k.shape == (1,) and k[0] == line["kenergy_after_run"] and rel_err(k[0], ke) < 1e-6


def test_cli_snapshot_and_restart(nbx, tmp_path):
    """NBODY_SNAPSHOT / NBODY_RESTART: 100 + 100 steps through a snapshot file == 200 steps straight, bit for bit."""
    import subprocess
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    a, b, c = (str(tmp_path / x) for x in ("a.snap", "b.snap", "c.snap"))
    run = lambda args, env: subprocess.run([exe] + args, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert run(["3000", "100"], {"NBODY_SNAPSHOT": a}).returncode == 0
    p2 = run(["3000", "100"], {"NBODY_RESTART": a, "NBODY_SNAPSHOT": b})
    p3 = run(["3000", "200"], {"NBODY_SNAPSHOT": c})
    assert p2.returncode == 0 and p3.returncode == 0
    sb, nb_ = nbx.read_snapshot(b)
    sc, nc_ = nbx.read_snapshot(c)
    assert nb_ == nc_ == 200
    for f in sb:
        assert np.array_equal(sb[f], sc[f]), f
    assert _rows(p2.stdout.splitlines())[-1][2] == _rows(p3.stdout.splitlines())[-1][2]
    # the snapshot is what a context would download after the same steps
    with nbx.Context(3000) as ctx:
        ctx.upload(nbx.initial_conditions(3000))
        ctx.step(200, kenergy=False)
        d = ctx.download()
    for f in d:
        assert np.array_equal(d[f], sc[f]), f
    bad = run(["2999", "10"], {"NBODY_RESTART": a})
    assert bad.returncode == 1 and "snapshot holds 3000 bodies" in bad.stderr


# ---- nbx_group: the single-process multi-GPU driver behind `NBODY_GPUS=k ./nbody.x` --------------------
@pytest.mark.parametrize("n,P", [(2000, 2), (4099, 4), (16384, 8), (300, 8)])
def test_group_of_logical_ranks_bit_equal_to_single_context(nbx, n, P):
    """All ranks on device 0 (the only one here): the same partition / step_local / exchange / commit sequence
    the multi-GPU run performs, with the exchange as stream-ordered device-to-device copies."""
    import sharded
    ic = nbx.initial_conditions(n)
    steps = 15
    with nbx.Group(n, 32, n_ranks=P, devices=[0] * P, j_split=4, bodies_per_lane=2) as g:
        Peff, rccl, st0 = g.info(0)
        assert not rccl and 1 <= Peff <= P
        g.upload(ic)
        ke_g = [g.step(5), g.step(5), g.step(5)]
        dg = g.download()
        st0 = g.info(0)[2]
        stl = g.info(Peff - 1)[2]
    assert st0["i_begin"] == 0 and stl["i_begin"] + stl["i_count"] == n and st0["steps_done"] == steps
    if n == 300:
        assert Peff == 2            # 256-record blocks: ranks that would own nothing are dropped
    n_alloc = st0["n_alloc"]
    assert n_alloc == sharded.block_partition(n, Peff, 0)[3]
    with nbx.Context(n, j_split=4, bodies_per_lane=2, n_alloc=n_alloc) as c:
        c.upload(ic)
        ke_c = [c.step(5), c.step(5), c.step(5)]
        dc = c.download()
    for f in dc:
        assert np.array_equal(dg[f], dc[f]), f
    assert rel_err(ke_g, ke_c).max() < 1e-12


def test_cli_multi_gpu_env(nbx):
    import subprocess
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    one = subprocess.run([exe, "4099", "100"], capture_output=True, text=True, timeout=300)
    four = subprocess.run([exe, "4099", "100"], env=dict(os.environ, NBODY_GPUS="4"), capture_output=True, text=True, timeout=300)
    assert one.returncode == 0 and four.returncode == 0, four.stderr
    r1, r4 = _rows(one.stdout.splitlines()), _rows(four.stdout.splitlines())
    assert [r[2] for r in r1] == [r[2] for r in r4] and len(r4) == 2
    assert any(ln.startswith("# GPUs / ranks       : 4 x ") for ln in four.stdout.splitlines())


def test_group_rccl_binding_with_one_rank(nbx):
    """NBX_EXCHANGE=rccl with a single rank: librccl is dlopen'ed, ncclCommInitAll / grouped in-place ncclAllGather run
    on the context's stream (the multi-device form of this call cannot run on a 1-GPU box).  Through the CLI too, where
    the system RCCL -- not the copy PyTorch bundles -- is the one that gets loaded."""
    import subprocess
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    ref = subprocess.run([exe, "3000", "100"], capture_output=True, text=True, timeout=300)
    got = subprocess.run([exe, "3000", "100"], env=dict(os.environ, NBX_EXCHANGE="rccl", NBODY_GPUS="1"), capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stderr[-2000:]
    assert [r[2] for r in _rows(got.stdout.splitlines())] == [r[2] for r in _rows(ref.stdout.splitlines())]
    os.environ["NBX_EXCHANGE"] = "rccl"
    try:
        with nbx.Group(3000, 32, n_ranks=1, devices=[0]) as g:
            P, rccl, _ = g.info(0)
            assert P == 1 and rccl
            g.upload(nbx.initial_conditions(3000))
            ke = g.step(20)
        # the weighted form exchanges with one in-place ncclBroadcast per owner (blocks of unequal size): the same one-rank smoke test
        with nbx.Group(3000, 32, n_ranks=1, devices=[0], weighted=True) as g:
            P, rccl, _ = g.info(0)
            assert P == 1 and rccl and g.shares(timings=False)[1] == [3000]
            g.upload(nbx.initial_conditions(3000))
            kew = g.step(20)
            assert not g.retune()                    # one rank: nothing to move
            kew2 = g.step(5)
    finally:
        del os.environ["NBX_EXCHANGE"]
    with nbx.Context(3000, use_graph=2) as c:
        c.upload(nbx.initial_conditions(3000))
        assert c.step(20) == ke == kew
        assert c.step(5) == kew2


# ---- NBX_KERNEL_EXACT: the reference's arithmetic bit for bit ---------------------------------------------------------
def _crc(a):
    import zlib
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


@pytest.mark.parametrize("name", ["ver7_f32_n5_s20.json", "ver7_f32_n65_s20.json", "ver7_f32_n1000_s100.json",
                                  "ver7_f32_n2000_s500.json", "ver7_f32_n4099_s40.json", "ver7_f32_n16384_s500.json",
                                  "ver7_f32_n32768_s500.json",   # the chaotic regime: no rounding-different kernel follows it
                                  pytest.param("ver7_f32_n65536_s500.json", marks=pytest.mark.skipif(
                                      not os.path.exists(os.path.join(ROOT, "tests", "golden", "ver7_f32_n65536_s500.json")),
                                      reason="fixture (25 min of the reference's CPU binary) not generated")),
                                  "ver7_f32_n65536_s20.json", "ver7_f32_n262144_s7.json", "ver7_f64_n2000_s500.json",
                                  "ver7_f64_n4099_s40.json", "ver7_f64_n16384_s60.json", "ver7_f64_n262144_s3.json"])
def test_exact_mode_reproduces_the_reference_trajectory_bit_for_bit(nbx, name):
    """kernel_variant = NBX_KERNEL_EXACT: after ALL steps of the fixture, the CRC-32 of each whole position and velocity
    array equals the one the reference's own ver7 binary produced (fp32 and the fp64 variant).  The fast kernels differ
    from this only by rounding (rsqrt instruction, FMA, summation order), which is what the tolerance tests bound."""
    g = load_golden(name)
    prec = g["precision"]
    with nbx.Context(g["n"], prec, kernel_variant=nbx.KERNEL_EXACT) as c:
        c.upload(nbx.initial_conditions(g["n"], prec))
        ke = c.step_trace(g["nsteps"])
        d = c.download()
        assert c.stats()["kernel_variant"] == nbx.KERNEL_EXACT
    for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert _crc(d[f]) == g["final"][f]["crc32"], f
    # energies: same terms, fp64 sum here vs the reference's thread-ordered float (or double) reduction
    assert rel_err(ke, g["kenergy"]).max() < (EXACT_MODE_ENERGY_TOL_F32 if prec == 32 else 1e-13)


def test_chaotic_regime_only_the_exact_mode_follows_the_reference(nbx):
    """n = 32768 x 500 steps against the REAL reference (fixture generated by its own binary): the cloud bounces around step
    20 and relaxes violently; from there any rounding-level difference is amplified.  The fast kernel (either order) stays
    inside the 1e-4 gate only for the first printed steps and is percent-level off by step 500 -- while the exact mode
    (previous test) ends on the reference's very bits.  Documents DESIGN.md 4b; not a BASELINE config."""
    g = load_golden("ver7_f32_n32768_s500.json")
    ref = np.array(g["kenergy"])
    out = {}
    for name, order in (("tree", nbx.ORDER_TREE), ("reference_order", nbx.ORDER_REFERENCE)):
        with nbx.Context(g["n"], 32, summation_order=order) as c:
            c.upload(nbx.initial_conditions(g["n"]))
            out[name] = rel_err(c.step_trace(500), ref)
    for name, e in out.items():
        assert e[:10].max() < 1e-5, (name, e[:10].max())      # before the bounce everything agrees
        assert e.max() < 0.2, (name, e.max())                    # and it never becomes a different simulation
    _dump("parity_chaotic_n32768_s500.json", {k: {"printed_steps": {str(s): float(v[s - 1]) for s in range(50, 501, 50)}, "max": float(v.max())}
                                  for k, v in out.items()})


def test_exact_mode_accelerations_equal_oracle_on_arbitrary_states(nbx, oracle):
    rng = np.random.default_rng(11)
    for n in (1, 3, 257, 1500):
        s = oracle.State(n)
        st = {}
        for f in ("pos_x", "pos_y", "pos_z"):
            getattr(s, f)[:] = rng.random(n, dtype=np.float32) * 4 - 2
        for f in ("vel_x", "vel_y", "vel_z"):
            getattr(s, f)[:] = rng.standard_normal(n).astype(np.float32) * 1e-3
        s.mass[:] = rng.random(n, dtype=np.float32) * 1e3
        st = {f: getattr(s, f).copy() for f in nbx.FIELDS}
        with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_EXACT) as c:
            c.upload(st)
            ax, ay, az = c.accel()
            c.step(9, kenergy=False)
            d = c.download()
        t = s.copy()
        oracle.accel(t)
        assert np.array_equal(ax, t.acc_x) and np.array_equal(ay, t.acc_y) and np.array_equal(az, t.acc_z), n
        oracle.run(s, 9)
        for f in d:
            assert np.array_equal(d[f], getattr(s, f)), (n, f)


def test_fast_kernels_differ_from_exact_mode_only_by_rounding(nbx):
    """One force evaluation: default kernel vs exact mode, per body, relative to |a|inf -- the rounding budget."""
    n = 16384
    ic = nbx.initial_conditions(n)
    acc = {}
    for k in (nbx.KERNEL_EXACT, nbx.KERNEL_SGPRW, nbx.KERNEL_LDS):
        with nbx.Context(n, 32, kernel_variant=k) as c:
            c.upload(ic)
            acc[k] = c.accel()
    scale = max(np.abs(a).max() for a in acc[nbx.KERNEL_EXACT])
    for k in (nbx.KERNEL_SGPRW, nbx.KERNEL_LDS):
        worst = max(np.abs(a - b).max() for a, b in zip(acc[k], acc[nbx.KERNEL_EXACT])) / scale
        assert 0 < worst < 2e-5, (k, worst)


def test_throughput_floors_other_configs(nbx):
    """Regression floors (well under the measured round-1 figures in profiles/r01_sweep_*): config 1's n, a mid n, fp64."""
    import time
    floors = [(16384, 32, 0.30), (65536, 32, 0.45), (65536, 64, 0.35)]
    for n, prec, floor in floors:
        with nbx.Context(n, prec) as c:
            c.upload(nbx.initial_conditions(n, prec))
            c.step(5, kenergy=False)
            c.sync()
            steps = 200 if n == 16384 else 30
            t0 = time.perf_counter()
            c.step(steps, kenergy=False)
            c.sync()
            dt = time.perf_counter() - t0
        frac = 20.0 * float(n) * n * steps / dt / (157.3e12 if prec == 32 else 78.6e12)
        assert frac > floor, (n, prec, frac)


# ---- summation order: the parity gate at the large configurations --------------------------------------------------
@pytest.fixture(scope="module")
def config2_run(nbx):
    """configs[2] (n = 262144 x 200 steps) stepped once for the tests below: reference order (= the default context), tree order and
    exact mode side by side, every step's energy, and exact mode's final state (19 s of the validation kernel: run it once)."""
    n, steps = 262144, 200
    ctx = {"reference_order": nbx.Context(n, 32), "tree": nbx.Context(n, 32, summation_order=nbx.ORDER_TREE),
           "exact": nbx.Context(n, 32, kernel_variant=nbx.KERNEL_EXACT)}
    ic = nbx.initial_conditions(n)
    tr = {}
    for name, c in ctx.items():
        c.upload(ic)
        tr[name] = np.concatenate([c.step_trace(25) for _ in range(steps // 25)])
    st = {k: c.stats() for k, c in ctx.items()}
    final = ctx["exact"].download()
    for c in ctx.values():
        c.close()
    return tr, st, final


def test_config2_printed_steps_reference_order_vs_reference_arithmetic(nbx, config2_run):
    """BASELINE.json configs[2] (n = 262144, rows at s = 50, 100, 150, 200).  The CPU reference needs 3.6 h for this
    run, so NBX_KERNEL_EXACT (bit-identical to it on every fixture, incl. 7 steps at this n) stands in.  The default
    (reference summation order) must stay within the north-star gate of 1e-4 at EVERY step; the tree order does not --
    the reference's one-accumulator fp32 sum heats the system -- which is why it is not the default at this size."""
    tr, st, _ = config2_run
    e_ref = rel_err(tr["reference_order"], tr["exact"])
    e_tree = rel_err(tr["tree"], tr["exact"])
    _dump("parity_config2_n262144_s200.json", {"reference_order_vs_exact": [float(x) for x in e_ref],
                                              "tree_vs_exact": [float(x) for x in e_tree],
                                              "printed_reference_order": {s: float(e_ref[s - 1]) for s in (50, 100, 150, 200)},
                                              "printed_tree": {s: float(e_tree[s - 1]) for s in (50, 100, 150, 200)}})
    assert st["reference_order"]["summation_order"] == nbx.ORDER_REFERENCE and st["reference_order"]["j_split"] == 1
    assert e_ref.max() < 1e-4, e_ref.max()
    assert e_tree[49] > 2e-4 and e_tree[199] > 5e-4          # documents WHY: measured 4.5e-4 and 1.3e-3


_CONFIG2_FIXTURE = os.path.join(ROOT, "tests", "golden", "ver7_f32_n262144_s200.json")


@pytest.mark.skipif(not os.path.exists(_CONFIG2_FIXTURE), reason="fixture of the full configs[2] run (hours of the reference's CPU binary) not generated")
def test_config2_all_200_steps_against_the_real_reference(nbx, config2_run):
    """BASELINE.json configs[2] against the reference's OWN binary over the whole run (fixture: `oracle/gen_golden.py --only
    f32:262144:200`, hours of CPU): the default kernel stays within the 1e-4 gate at every step, the printed rows
    (s = 50, 100, 150, 200) included, and NBX_KERNEL_EXACT ends on the reference's very bits."""
    g = load_golden("ver7_f32_n262144_s200.json")
    ref = np.array(g["kenergy"])
    tr, st, d = config2_run
    assert st["reference_order"]["summation_order"] == nbx.ORDER_REFERENCE   # the default context
    e = rel_err(tr["reference_order"], ref)
    ke = tr["exact"]
    _dump("parity_config2_vs_real_reference.json", {"max": float(e.max()), "printed": {str(s): float(e[s - 1]) for s in (50, 100, 150, 200)},
                                                    "all_steps": [float(x) for x in e]})
    assert e.max() < 1e-4, e.max()
    for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert _crc(d[f]) == g["final"][f]["crc32"], f
    # same velocities, different sum: the reference reduces m*v^2 in float over its OpenMP threads, here an fp64 tree
    assert rel_err(ke, ref).max() < EXACT_MODE_ENERGY_TOL_F32



_CONFIG3_FIXTURES = [f for f in ("ver7_f32_n1048576_s3.json", "ver7_f32_n1048576_s10.json") if os.path.exists(os.path.join(ROOT, "tests", "golden", f))]


@pytest.mark.skipif(not _CONFIG3_FIXTURES, reason="fixtures of configs[3]'s first steps (12-15 min of the reference's CPU binary per step) not generated")
@pytest.mark.parametrize("name", _CONFIG3_FIXTURES or ["none"])
def test_config3_first_steps_against_the_real_reference(nbx, name):
    """BASELINE.json configs[3]'s size (n = 1048576) against the reference's own binary for its first 3 (and, second fixture,
    10) steps -- 12-15 min of CPU per step here: one context, 8 logical ranks of 131072 bodies (the 8-GPU partition) and
    the exact mode."""
    g = load_golden(name)
    n, k = g["n"], g["nsteps"]
    ref = np.array(g["kenergy"])
    ic = nbx.initial_conditions(n)
    with nbx.Context(n) as c:
        c.upload(ic)
        e1 = rel_err(c.step_trace(k), ref)
        assert c.stats()["summation_order"] == nbx.ORDER_REFERENCE
    with nbx.Group(n, 32, n_ranks=8) as grp:
        grp.upload(ic)
        e8 = abs(grp.step(k) - ref[-1]) / ref[-1]
    with nbx.Context(n, kernel_variant=nbx.KERNEL_EXACT) as c:
        c.upload(ic)
        ke = c.step_trace(k)
        d = c.download()
    _dump("parity_config3_vs_real_reference_s%d.json" % k, {"one_context": [float(x) for x in e1], "eight_logical_ranks_last_step": float(e8),
                                                            "exact_mode_kenergy": [float(x) for x in rel_err(ke, ref)]})
    assert e1.max() < 1e-5 and e8 < 1e-5, (e1, e8)
    for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert _crc(d[f]) == g["final"][f]["crc32"], f
    # the stored exact-mode trace of all 100 steps (tools/gen_exact_fixture.py, used by the 100-step test below) starts on these very numbers
    stored = os.path.join(ROOT, "tests", "golden", "nbx_exact_f32_n1048576_s100.json")
    if os.path.exists(stored):
        assert np.array_equal(np.array(json.load(open(stored))["kenergy"][:k]), ke), "exact mode no longer reproduces its stored trace"


_CONFIG4_FIXTURE = os.path.join(ROOT, "tests", "golden", "ver7_f64_n262144_s50.json")


@pytest.mark.skipif(not os.path.exists(_CONFIG4_FIXTURE), reason="fixture of 50 fp64 steps at n = 262144 (over an hour of the reference's CPU binary) not generated")
def test_config4_fp64_first_printed_row_against_the_real_reference(nbx):
    """BASELINE.json configs[4] (n = 262144, fp64 variant, tolerance 1e-10) up to the first printed row (s = 50) against the
    reference's own source built as the fp64 variant; exact mode CRC-identical after the 50 steps."""
    g = load_golden("ver7_f64_n262144_s50.json")
    ref = np.array(g["kenergy"])
    with nbx.Context(262144, 64) as c:
        c.upload(nbx.initial_conditions(262144, 64))
        e = rel_err(c.step_trace(50), ref)
    _dump("parity_config4_vs_real_reference.json", {"max": float(e.max()), "step50": float(e[49]), "all_steps": [float(x) for x in e]})
    assert e.max() < 1e-10, e.max()
    with nbx.Context(262144, 64, kernel_variant=nbx.KERNEL_EXACT) as c:
        c.upload(nbx.initial_conditions(262144, 64))
        ke = c.step_trace(50)
        d = c.download()
    for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert _crc(d[f]) == g["final"][f]["crc32"], f
    assert rel_err(ke, ref).max() < 1e-13


_CONFIG3_EXACT_FIXTURE = os.path.join(ROOT, "tests", "golden", "nbx_exact_f32_n1048576_s100.json")


@pytest.mark.skipif(not os.path.exists(_CONFIG3_EXACT_FIXTURE), reason="tools/gen_exact_fixture.py has not been run (120 s of GPU)")
def test_config3_all_100_steps_printed_rows_vs_reference_arithmetic(nbx):
    """BASELINE.json configs[3] (n = 1048576, 100 steps, rows printed at s = 50 and s = 100: ver7/GSimulation.cpp:203-212) over
    the WHOLE run.  The reference's CPU binary needs ~12 min per step at this size (its first 10 steps are the anchor:
    test_config3_first_steps_against_the_real_reference, CRC-identical to NBX_KERNEL_EXACT), so exact mode -- the reference's
    arithmetic bit for bit -- carries the comparison from there to step 100.  Its trace is a committed fixture since round 4
    (tools/gen_exact_fixture.py; 120 s of the validation kernel per run bought nothing: the trace is an fp64 fixed-order sum of a
    bit-reproducible trajectory) whose first 10 entries are re-derived live, bit for bit, by the first-steps test on every run and
    the whole of it with NBX_TEST_FULL=1.  Gated: the default context at every step, and both it and the 8-rank partition of the
    8-GPU run (8 logical ranks, the same kernels and slices) at the two printed rows, within 1e-5 of exact mode (10x inside the
    1e-4 gate; measured ~5e-7).  Tree order is shown NOT to qualify at this size (why reference order is the default here)."""
    n, steps = 1048576, 100
    gx = load_golden("nbx_exact_f32_n1048576_s100.json")
    assert gx["n"] == n and gx["nsteps"] == steps
    exact = np.array(gx["kenergy"])
    g10 = load_golden("ver7_f32_n1048576_s10.json")        # the stored trace starts on the reference's own numbers
    assert rel_err(exact[:10], np.array(g10["kenergy"])).max() < EXACT_MODE_ENERGY_TOL_F32
    ic = nbx.initial_conditions(n)
    if os.environ.get("NBX_TEST_FULL"):
        with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_EXACT) as c:
            c.upload(ic)
            live = np.concatenate([c.step_trace(25) for _ in range(steps // 25)])
            d = c.download()
        assert np.array_equal(live, exact)
        for f in d:
            assert _crc(d[f]) == gx["final"][f]["crc32"], f
    with nbx.Context(n, 32) as c:
        c.upload(ic)
        st = c.stats()
        assert st["summation_order"] == nbx.ORDER_REFERENCE and st["j_split"] == 1
        default = np.concatenate([c.step_trace(25) for _ in range(steps // 25)])
    with nbx.Context(n, 32, summation_order=nbx.ORDER_TREE) as c:
        c.upload(ic)
        tree6 = c.step_trace(6)
    with nbx.Group(n, 32, n_ranks=8) as grp:
        grp.upload(ic)
        P, _, st8 = grp.info(0)
        ke8 = {s: grp.step(50) for s in (50, 100)}
    assert P == 8 and st8["i_count"] == n // 8 and st8["summation_order"] == nbx.ORDER_REFERENCE
    e = rel_err(default, exact)
    e8 = {s: abs(ke8[s] - exact[s - 1]) / exact[s - 1] for s in (50, 100)}
    _dump("parity_config3_n1048576_s100.json", {
        "what": "kenergy per step, n = 1048576 x 100 steps (BASELINE.json configs[3]): relative difference to NBX_KERNEL_EXACT (= the reference's arithmetic, CRC-pinned on its first 10 steps; trace from tests/golden/nbx_exact_f32_n1048576_s100.json)",
        "default_context_vs_exact_all_steps": [float(x) for x in e], "default_context_max": float(e.max()),
        "printed_rows": {str(s): {"exact_kenergy": float(exact[s - 1]), "default_context": float(e[s - 1]), "eight_ranks": float(e8[s])} for s in (50, 100)},
        "tree_order_first_6_steps": [float(x) for x in rel_err(tree6, exact[:6])]})
    assert e.max() < 1e-5, (int(e.argmax()) + 1, e.max())
    assert e[49] < 1e-5 and e[99] < 1e-5 and e8[50] < 1e-5 and e8[100] < 1e-5, (e[49], e[99], e8)
    assert rel_err(tree6, exact[:6]).max() > 2e-4                  # measured 8.5e-4 from step 1 on


@pytest.mark.parametrize("prec", [32, 64])
def test_reference_order_is_partition_independent_bit_for_bit(nbx, prec):
    """One accumulator per body over all j in ascending order: the result for a body cannot depend on who owns it, on the
    j source, on bodies per lane or on graph replay -- single context, 3 logical ranks and every plain shape agree bitwise."""
    n, steps = 5001, 12
    ic = nbx.initial_conditions(n, prec)
    with nbx.Context(n, prec, summation_order=nbx.ORDER_REFERENCE) as c:
        c.upload(ic)
        st = c.stats()
        assert st["summation_order"] == nbx.ORDER_REFERENCE and st["j_split"] == 1 and st["fused_epilogue"] == 1
        ke = c.step(steps)
        ref = c.download()
    for opts in (dict(kernel_variant=nbx.KERNEL_LDS, bodies_per_lane=1), dict(kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=4),
                 dict(kernel_variant=nbx.KERNEL_LDS, bodies_per_lane=4, fused_epilogue=2), dict(use_graph=1),
                 dict(kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=1),                      # fp32: two j records per packed operation
                 dict(kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=1, use_graph=1, fused_epilogue=2)):
        with nbx.Context(n, prec, summation_order=nbx.ORDER_REFERENCE, **opts) as c:
            c.upload(ic)
            c.step(steps, kenergy=False)
            d = c.download()
        for f in ref:
            assert np.array_equal(d[f], ref[f]), (opts, f)
    with nbx.Group(n, prec, n_ranks=3, devices=[0, 0, 0], summation_order=nbx.ORDER_REFERENCE) as g:
        g.upload(ic)
        keg = g.step(steps)
        dg = g.download()
        assert g.info(1)[2]["summation_order"] == nbx.ORDER_REFERENCE
    for f in ref:
        assert np.array_equal(dg[f], ref[f]), f
    assert abs(keg / ke - 1.0) < 1e-13


def test_eight_ranks_of_config2_with_the_two_records_per_operation_loop_against_the_real_reference(nbx):
    """n = 262144 on 8 ranks = 32768 bodies per rank: half a wave per SIMD with two bodies per lane, so every rank takes one body per
    lane and the two-j-records-per-operation loop (sgpr_loop_asm_jpair).  All 200 steps of BASELINE configs[2] as 8 logical ranks
    against the trace of the reference's own binary (tests/golden/ver7_f32_n262144_s200.json, gate 1e-4), and the final state bit
    for bit against the one-context run (two bodies per lane, time-sliced loop): reference order is partition independent."""
    if not os.path.exists(_CONFIG2_FIXTURE):
        pytest.skip("fixture of the full configs[2] run not generated")
    g = load_golden("ver7_f32_n262144_s200.json")
    n, steps = g["n"], g["nsteps"]
    assert n == 262144 and steps == 200
    ref = np.array(g["kenergy"])
    ic = nbx.initial_conditions(n)
    with nbx.Group(n, 32, n_ranks=8) as grp:
        grp.upload(ic)
        P, _, st = grp.info(3)
        assert P == 8 and st["i_count"] == 32768 and st["bodies_per_lane"] == 1 and st["inner_loop"] == nbx.LOOP_ASM
        assert st["kernel_variant"] == nbx.KERNEL_SGPR and st["summation_order"] == nbx.ORDER_REFERENCE and st["force_grid_x"] == 128
        ke = np.array([grp.step(1) for _ in range(steps)])
        d8 = grp.download()
    e = rel_err(ke, ref)
    assert e.max() < 1e-4, (int(e.argmax()) + 1, e.max())          # measured 4.9e-5, as the one-context run
    with nbx.Context(n, 32) as c:
        c.upload(ic)
        assert c.stats()["bodies_per_lane"] == 2
        ke1 = c.step(steps)
        d1 = c.download()
    for f in d1:
        assert np.array_equal(d8[f], d1[f]), f
    assert abs(ke[-1] / ke1 - 1.0) < 1e-13


def test_weighted_shares_and_retuning_change_no_bit_in_reference_order(nbx):
    """nbx_group_create_weighted / nbx_group_retune (the reference's cpu_ratio split and its tuner, with GPUs as the devices): shares
    of whole 256-record tiles in proportion 1:2:1, moved in mid-run by the tuner (synthetic per-rank times: rank 1 eight times slower)
    -- and the trajectory stays that of one context bit for bit, because reference summation order gives every body the same chain
    whoever owns it and a retune copies values, never recomputes them."""
    n, steps = 5001, 6
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, summation_order=nbx.ORDER_REFERENCE) as c:
        c.upload(ic)
        ke_ref = [c.step(steps) for _ in range(2)]
        ref = c.download()
    with nbx.Group(n, 32, n_ranks=3, devices=[0, 0, 0], weights=[1, 2, 1], summation_order=nbx.ORDER_REFERENCE) as g:
        g.upload(ic)
        b, cnt, _ = g.shares(timings=False)
        assert cnt == [1280, 2560, 1161] and b == [0, 1280, 3840] and g.info(0)[0] == 3
        ke = [g.step(steps)]
        _, _, ms = g.shares()
        assert all(x > 0 for x in ms)                                   # every rank timed its force launches
        # at this size every share is less than one workgroup per CU: a launch takes the same time whatever the share, the library's cost
        # model knows it, and the tuner does not move bodies for nothing
        assert not g.retune([1.0, 8.0, 1.0]) and g.shares(timings=False)[1] == cnt
        ke.append(g.step(steps))
        got = g.download()
    for f in ref:
        assert np.array_equal(got[f], ref[f]), f
    assert all(abs(a / b - 1.0) < 1e-13 for a, b in zip(ke, ke_ref))
    # configs[2]'s size, weights 1:2:1 over three logical ranks: 65536 / 131072 / 65536 bodies = the two-records-per-operation loop on
    # ranks 0 and 2, two bodies per lane with the L2 prefetch on rank 1 -- against one context (two bodies per lane, time-sliced); then
    # a retune that does pay by the model (rank 1 eight times slower per launch) moves the shares in mid-run: still the same bits
    n = 262144
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32) as c:
        c.upload(ic)
        k1 = [c.step(3), c.step(2)]
        ref = c.download()
    with nbx.Group(n, 32, n_ranks=3, devices=[0, 0, 0], weights=[1, 2, 1]) as g:
        g.upload(ic)
        assert g.shares(timings=False)[1] == [65536, 131072, 65536]
        assert [g.info(r)[2]["bodies_per_lane"] for r in range(3)] == [1, 2, 1] and g.info(1)[2]["inner_loop"] == nbx.LOOP_ASM_PF
        k3 = [g.step(3)]
        assert g.retune([1.0, 8.0, 1.0])
        cnt2 = g.shares(timings=False)[1]
        assert sum(cnt2) == n and cnt2[1] < 65536 and all(x % 256 == 0 for x in g.shares(timings=False)[0])
        k3.append(g.step(2))
        g.retune()                                                       # from its own measurements: may or may not move a tile
        assert sum(g.shares(timings=False)[1]) == n
        got = g.download()
    for f in ref:
        assert np.array_equal(got[f], ref[f]), f
    assert all(abs(a / b - 1.0) < 1e-13 for a, b in zip(k3, k1))
    with pytest.raises(nbx.NbxError):                                    # retuning needs the weighted form
        with nbx.Group(5001, 32, n_ranks=2, devices=[0, 0]) as g:
            g.upload(nbx.initial_conditions(5001))
            g.retune()


def test_the_tuner_predicts_before_it_moves_and_takes_back_what_made_the_step_slower(nbx):
    """A rank's time is a step function of its share in reference order (a launch lasts as long as its fullest SIMD: 131072 bodies of 1M
    take 30 ms, 131073 take 58).  nbx_group_retune therefore (1) predicts each rank's time under the new shares with the library's own
    cost table and does not make a move the model expects to slow the slowest rank down, and (2) judges every move it did make by the
    window after it: slower than before (by more than 1 %) -> the previous shares come back and stay."""
    # (1) four ranks of 65536 bodies at n = 262144 sit exactly at one workgroup per CU: any rank that grows gets a second round.  Rank 0
    # measured 9 % faster (noise, or a faster clock): a proportional move would cost +100 % -- refused
    n = 262144
    with nbx.Group(n, 32, n_ranks=4, devices=[0, 0, 0, 0], weighted=True) as g:
        g.upload(nbx.initial_conditions(n))
        g.step(1, kenergy=False)
        assert g.shares(timings=False)[1] == [65536] * 4
        assert not g.retune([4.30, 4.70, 4.70, 4.70])
        assert g.shares(timings=False)[1] == [65536] * 4
    # (2) tree order (time close to proportional to the share): a move is made, the next window is reported slower, it is taken back
    n = 20000
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32) as c:
        c.upload(ic)
        ke_ref = c.step(9)
    with nbx.Group(n, 32, n_ranks=2, devices=[0, 0], weighted=True) as g:
        g.upload(ic)
        first = g.shares(timings=False)[1]
        g.step(3, kenergy=False)
        assert g.retune([1.0, 2.0])                               # slowest rank 2.0: bodies move to rank 0
        moved = g.shares(timings=False)[1]
        assert moved[0] > first[0]
        g.step(3, kenergy=False)
        assert g.retune([3.0, 0.5])                               # the window after the move: slowest rank 3.0 > 2.0 -> taken back
        assert g.shares(timings=False)[1] == first
        assert not g.retune([1.0, 2.0])                           # and the shares are left alone from then on
        assert g.shares(timings=False)[1] == first
        ke = g.step(3)
    assert abs(ke / ke_ref - 1.0) < 2e-6
    with nbx.Group(n, 32, n_ranks=2, devices=[0, 0], weighted=True) as g:
        g.upload(ic)
        g.step(2, kenergy=False)
        assert g.retune([1.0, 2.0])
        after = g.shares(timings=False)[1]
        assert not g.retune([1.3, 1.3])                            # both ranks now take the same time, less than before: kept, fixed point
        assert g.shares(timings=False)[1] == after


def test_recorded_retune_scenarios_on_the_device(nbx):
    """tests/golden/group_shares.json, `retune`: what nbx_group_retune decided before the share planner moved to csrc/nbx_shares.hpp
    (tools/record_group_shares.py; one scenario per branch of the decision).  Logical ranks on device 0, the recorded force_ms, nothing
    stepped: the same `changed` flag and the same shares after every call.  tests/test_shares_cpu.py replays them without a device."""
    d = load_golden("group_shares.json")
    assert len(d["retune"]) >= 10
    for s in d["retune"]:
        with nbx.Group(s["n"], s["precision"], n_ranks=s["ranks"], devices=[0] * s["ranks"], weights=s["weights"], weighted=True, **s["opts"]) as g:
            g.upload(nbx.initial_conditions(s["n"], s["precision"]))
            assert g.info(0)[2]["cu_count"] == d["cu_count"]
            assert g.shares(timings=False)[:2] == (s["begin"], s["count"]), s["name"]
            for c in s["calls"]:
                changed = g.retune(c["force_ms"])
                assert (int(changed),) + g.shares(timings=False)[:2] == (c["changed"], c["begin"], c["count"]), (s["name"], c)


@pytest.mark.parametrize("prec,tol", [(32, 2e-6), (64, 1e-12)])
def test_weighted_shares_in_tree_order_and_fp64_stay_inside_the_rounding_band(nbx, prec, tol):
    """Tree order: the summation tree of a body depends on the launch shape of whoever owns it, so shares and retunes move results
    by rounding only -- energies of a weighted, retuned group against one context (fp32 2e-6 after 30 steps, fp64 1e-12), every body
    stepped exactly once per step (positions close to the single context's everywhere)."""
    n, steps = 20000, 10
    ic = nbx.initial_conditions(n, prec)
    with nbx.Context(n, prec) as c:
        c.upload(ic)
        assert c.stats()["summation_order"] == nbx.ORDER_TREE
        ke_ref = [c.step(steps) for _ in range(3)]
        ref = c.download()
    with nbx.Group(n, prec, n_ranks=2, devices=[0, 0], weights=[1, 3]) as g:
        g.upload(ic)
        assert g.shares(timings=False)[1] == [5120, 14880]
        ke = [g.step(steps)]
        assert g.retune([1.0, 9.0])                                     # rank 0: 5120 bodies per unit, rank 1: 14880 in 9 -- rank 0 is the fast one
        assert g.shares(timings=False)[1][0] > 3 * 5120 - 512
        ke.append(g.step(steps))
        g.retune()
        ke.append(g.step(steps))
        got = g.download()
    assert max(abs(a / b - 1.0) for a, b in zip(ke, ke_ref)) < tol, (ke, ke_ref)
    for f in ref:
        assert np.allclose(got[f], ref[f], rtol=1e-4 if prec == 32 else 1e-10, atol=1e-5 if prec == 32 else 1e-12), f


def test_auto_order_threshold(nbx):
    for n, want in ((131072, nbx.ORDER_TREE), (131073, nbx.ORDER_REFERENCE), (262144, nbx.ORDER_REFERENCE)):
        with nbx.Context(n) as c:
            assert c.stats()["summation_order"] == want, n
    # the decision follows n, the length of the sums, not the slice a rank owns: every rank of a sharded run agrees
    with nbx.Context(262144, i_begin=65536, i_count=32768, n_alloc=262144) as c:
        st = c.stats()
        assert st["summation_order"] == nbx.ORDER_REFERENCE and st["j_split"] == 1 and st["bodies_per_lane"] == 1
        assert st["inner_loop"] == nbx.LOOP_ASM and st["kernel_variant"] == nbx.KERNEL_SGPR  # two j records per packed operation
    for own, B in ((65536, 1), (65537, 2), (49152, 1), (131072, 2)):   # one body per lane up to one workgroup per CU, two from there
        with nbx.Context(1048576, i_begin=0, i_count=own, n_alloc=1048576) as c:
            assert c.stats()["bodies_per_lane"] == B, own
    with nbx.Context(131072, i_begin=0, i_count=16384, n_alloc=131072) as c:
        assert c.stats()["summation_order"] == nbx.ORDER_TREE
    with nbx.Context(1048576, i_begin=0, i_count=131072, n_alloc=1048576) as c:      # one rank of the 8-GPU configuration
        st = c.stats()
        assert st["summation_order"] == nbx.ORDER_REFERENCE and st["j_split"] == 1 and st["bodies_per_lane"] == 2
    with nbx.Context(262144, j_split=8) as c:                                        # an explicit split means tree
        assert c.stats()["summation_order"] == nbx.ORDER_TREE
    with nbx.Context(262144, 64) as c:                                               # fp64: noise 1e-13, tree is fine
        assert c.stats()["summation_order"] == nbx.ORDER_TREE


def test_randomized_shapes_orders_and_sizes_against_exact_mode(nbx, oracle):
    """80 pseudo-random (n, precision, kernel, bodies/lane, j-split, order, epilogue, slice) combinations, fixed seed: every one
    must agree with the bit-exact reference arithmetic on the accelerations (2e-5 of |a|inf) and on a 3-step state.  The un-sliced
    ones also take the zero-velocity probe of tests/test_step_probe_gpu.py: every body of the step kernel against a
    high-precision direct sum, under the gate of tests/force_ref.py (the atol below lets a 1 % error of one body pass)."""
    import force_ref
    from test_step_probe_gpu import reference_of, state_of
    rng = np.random.default_rng(20261004)
    tried = 0
    for _ in range(80):
        n = int(rng.choice([1, 2, 7, 63, 64, 65, 255, 256, 257, 511, 1000, 1023, 1025, 2047, 3000, 4099, 6001]))
        prec = int(rng.choice([32, 32, 32, 64]))
        opts = dict(kernel_variant=int(rng.choice([0, 1, 2, 3])), bodies_per_lane=int(rng.choice([0, 1, 2, 4, 8])),
                    j_split=int(rng.choice([0, 0, 1, 2, 3, 5, 16, 64])), summation_order=int(rng.choice([0, 1, 2])),
                    fused_epilogue=int(rng.choice([0, 1, 2])), use_graph=int(rng.choice([0, 1, 2])))
        sl = {}
        if n > 300 and rng.random() < 0.3:      # a slice of a larger padded array, as one rank of a sharded run has
            ib = int(rng.integers(0, n // 2))
            sl = dict(i_begin=ib, i_count=int(rng.integers(1, n - ib + 1)), n_alloc=int(-(-n // 256) * 256 + 256 * rng.integers(0, 3)))
        ic = nbx.initial_conditions(n, prec)
        try:
            c = nbx.Context(n, prec, **opts, **sl)
        except nbx.NbxError as e:
            assert e.code == nbx.NBX_ERR_ARG, (opts, sl, str(e))
            continue
        with c, nbx.Context(n, prec, kernel_variant=nbx.KERNEL_EXACT, **sl) as x:
            c.upload(ic)
            x.upload(ic)
            a, b = c.accel(), x.accel()
            st = c.stats()
            lo, hi = st["i_begin"], st["i_begin"] + st["i_count"]
            scale = max(max(float(np.abs(v[lo:hi]).max()) for v in b), 1e-300)   # float(): a float32 zero would swallow 1e-300
            err = max(float(np.abs(u[lo:hi].astype(np.float64) - v[lo:hi]).max()) for u, v in zip(a, b)) / scale
            assert err < (2e-5 if prec == 32 else 1e-12), (n, prec, opts, sl, err)
            if not sl:
                k1, k2 = c.step(3), x.step(3)
                assert abs(k1 - k2) <= 2e-5 * abs(k2) + 1e-300, (n, prec, opts, k1, k2)
                d1, d2 = c.download(), x.download()
                for f in d1:
                    assert np.allclose(d1[f], d2[f], rtol=1e-4 if prec == 32 else 1e-11, atol=1e-6 if prec == 32 else 1e-14), (n, opts, f)
                tr, k_ref = reference_of(oracle, "seed42", n, prec)
                c.upload(state_of(oracle, "seed42", n, prec))
                c.step(1)
                d1 = c.download()
                K = force_ref.k_metric(force_ref.accel_from_v1(np.stack([d1["vel_x"], d1["vel_y"], d1["vel_z"]], axis=1), prec), tr, prec)
                bad = np.flatnonzero(~(K <= force_ref.gate(k_ref.max())))
                assert bad.size == 0, (n, prec, opts, "bodies over the gate %.1f" % force_ref.gate(k_ref.max()), [(int(i), float(K[i])) for i in bad[:10]])
            else:
                c.step_local()
                c.commit()
                x.step_local()
                x.commit()
                p1, p2 = c.kenergy_partial(), x.kenergy_partial()
                assert abs(p1 - p2) <= 2e-5 * abs(p2) + 1e-300, (n, prec, opts, sl)
        tried += 1
    assert tried >= 60


# ---- the hand-scheduled j loop (nbx_sgpr_loop.inc) against the compiler-scheduled one ------------------------------
@pytest.mark.parametrize("n,own,steps", [(2000, 2000, 40), (4099, 4099, 25), (16384, 16384, 12), (65536, 65536, 4), (300, 300, 30),
                                          (262144, 32768, 2)])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_hand_scheduled_loop_is_bit_equal_to_the_compiled_loop(nbx, n, own, steps, B):
    """inner_loop = NBX_LOOP_ASM runs the same operations in the same order as the C++ loop: accelerations, trajectories
    and energies must agree bit for bit, for the row epilogue (reference order), for slabs (j-splits) and on a slice.
    This is also the hazard check of the asm stream: a consumer issued too close to its producer would change bits.
    B = 1 is the two-j-records-per-packed-operation loop (round 4): records j and j + 1 of ONE body in the two halves of each
    packed instruction, out of the pair-interleaved copy of the records, the two terms added in ascending j -- against the
    compiled one-body-per-lane loop with its plain (unpacked) instructions."""
    ic = nbx.initial_conditions(n)
    for shape in (dict(j_split=1), dict(j_split=1, fused_epilogue=2), dict(j_split=3), dict(j_split=16)):
        res = []
        for loop in (nbx.LOOP_ASM, nbx.LOOP_CXX):
            with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=B, inner_loop=loop, use_graph=2,
                             i_begin=0, i_count=own, n_alloc=n, **shape) as c:
                c.upload(ic)
                acc = c.accel()
                for _ in range(steps):
                    c.step_local()
                    c.commit()
                part = c.kenergy_partial()
                st = c.stats()
                assert st["inner_loop"] == loop and st["bodies_per_lane"] == B and st["kernel_variant"] == nbx.KERNEL_SGPR
                res.append((acc, c.download(), part))
        for k in range(3):
            assert np.array_equal(res[0][0][k], res[1][0][k]), (shape, "acc", k)
        for f in res[0][1]:
            assert np.array_equal(res[0][1][f], res[1][1][f]), (shape, f)
        assert res[0][2] == res[1][2], shape


@pytest.mark.parametrize("n,S,steps", [(16384, 32, 10), (16384, 8, 6), (65536, 32, 3), (4096, 16, 20)])
@pytest.mark.parametrize("B", [2, 4])
def test_hand_scheduled_loop_in_the_wave_split_kernel_is_bit_equal_too(nbx, n, S, steps, B):
    """SGPRW (tree order: the four waves of a workgroup split each j range) takes the same generated loop whenever a wave's
    quarter of a split is a whole number of trips (j_per_split a multiple of 256): same bits as the compiled loop."""
    ic = nbx.initial_conditions(n)
    res = []
    for loop in (nbx.LOOP_ASM, nbx.LOOP_CXX):
        with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_SGPRW, bodies_per_lane=B, j_split=S, inner_loop=loop, use_graph=2) as c:
            c.upload(ic)
            acc = c.accel()
            ke = c.step_trace(steps)
            st = c.stats()
            assert st["inner_loop"] == loop and st["kernel_variant"] == nbx.KERNEL_SGPRW and st["j_split"] == S
            res.append((acc, ke, c.download()))
    for k in range(3):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    assert np.array_equal(res[0][1], res[1][1])
    for f in res[0][2]:
        assert np.array_equal(res[0][2][f], res[1][2][f]), f
    with pytest.raises(nbx.NbxError):  # j_per_split = 96: a wave's quarter is not a whole trip
        nbx.Context(n, 32, kernel_variant=nbx.KERNEL_SGPRW, bodies_per_lane=B, j_split=n // 96, inner_loop=nbx.LOOP_ASM)


def test_hand_scheduled_loop_bit_equal_on_adversarial_states(nbx):
    """Not only the seed-42 cloud: clustered bodies (many pairs at r^2 = softening), coincident bodies, masses spanning twelve
    decades, zero masses, masses so small that G m / r^3 is a denormal number, a far-away outlier -- whatever the operands, the two
    loops must produce the same bits.  One body per lane compares PACKED instructions (two j records per operation) with the compiled
    loop's plain ones: the denormal terms are where the two instruction families could have differed."""
    rng = np.random.default_rng(7)
    n = 8192
    st8 = {f: np.zeros(n, dtype=np.float32) for f in nbx.FIELDS}
    centres = rng.random((16, 3), dtype=np.float32)
    k = rng.integers(0, 16, n)
    spread = np.float32(10.0) ** rng.uniform(-7, -1, n).astype(np.float32)
    for a, f in enumerate(("pos_x", "pos_y", "pos_z")):
        st8[f] = (centres[k, a] + spread * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    st8["pos_x"][1::97] = st8["pos_x"][0]; st8["pos_y"][1::97] = st8["pos_y"][0]; st8["pos_z"][1::97] = st8["pos_z"][0]  # coincident
    st8["pos_x"][5] = np.float32(3.0e3)                                                                                     # outlier
    for f in ("vel_x", "vel_y", "vel_z"):
        st8[f] = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    st8["mass"] = (np.float32(10.0) ** rng.uniform(-6, 6, n).astype(np.float32)).astype(np.float32)
    st8["mass"][::13] = 0.0
    st8["mass"][3::29] = np.float32(1e-22)   # G m = 6.7e-33: times 1 / r^3 of the outlier (3.7e-11) far below the smallest normal float
    st8["mass"][4::31] = np.float32(3e-26)
    for variant, shapes in ((nbx.KERNEL_SGPR, (dict(j_split=1), dict(j_split=4))), (nbx.KERNEL_SGPRW, (dict(j_split=8),))):
        for B in ((1, 2, 4) if variant == nbx.KERNEL_SGPR else (2, 4)):
            for shape in shapes:
                res = []
                for loop in (nbx.LOOP_ASM, nbx.LOOP_CXX):
                    with nbx.Context(n, 32, kernel_variant=variant, bodies_per_lane=B, inner_loop=loop, use_graph=2, **shape) as c:
                        c.upload(st8)
                        acc = c.accel()
                        ke = c.step_trace(6)
                        assert c.stats()["inner_loop"] == loop
                        res.append((acc, ke, c.download()))
                assert all(np.isfinite(x).all() for x in res[0][0])
                for q in range(3):
                    assert np.array_equal(res[0][0][q], res[1][0][q]), (variant, B, shape, q)
                assert np.array_equal(res[0][1], res[1][1]), (variant, B, shape)
                for f in res[0][2]:
                    assert np.array_equal(res[0][2][f], res[1][2][f]), (variant, B, shape, f)


def test_hand_scheduled_loop_bit_equal_over_random_sizes_slices_and_splits(nbx):
    """80 seeded random combinations of n (ragged), owned slice, bodies per lane, kernel, j-split: wherever an asm instance
    exists for the shape it must agree with the compiled loop bit for bit (accelerations and two steps)."""
    rng = np.random.default_rng(2024)
    checked = 0
    for _ in range(80):
        n = int(rng.integers(300, 40000))
        blk = -(-n // 256) * 256
        i_begin = int(rng.integers(0, max(1, n // 2)))
        i_count = int(rng.integers(1, n - i_begin + 1))
        B = int(rng.choice([2, 4]))
        variant = int(rng.choice([nbx.KERNEL_SGPR, nbx.KERNEL_SGPRW]))
        S = int(rng.choice([1, 2, 3, 5, 8, 16])) if variant == nbx.KERNEL_SGPR else int(rng.choice([1, 2, 4, 8]))
        opts = dict(kernel_variant=variant, bodies_per_lane=B, j_split=S, i_begin=i_begin, i_count=i_count, n_alloc=blk, use_graph=2)
        try:
            ca = nbx.Context(n, 32, inner_loop=nbx.LOOP_ASM, **opts)
        except nbx.NbxError:
            continue  # no instance for this shape (a wave's quarter of a split is not a whole trip)
        ic = nbx.initial_conditions(n)
        with ca, nbx.Context(n, 32, inner_loop=nbx.LOOP_CXX, **opts) as cc:
            out = []
            for c in (ca, cc):
                c.upload(ic)
                acc = c.accel()
                for _k in range(2):
                    c.step_local()
                    c.commit()
                out.append((acc, c.download(), c.kenergy_partial()))
            assert ca.stats()["inner_loop"] == nbx.LOOP_ASM and cc.stats()["inner_loop"] == nbx.LOOP_CXX
        for q in range(3):
            assert np.array_equal(out[0][0][q], out[1][0][q]), (n, opts, q)
        for f in out[0][1]:
            assert np.array_equal(out[0][1][f], out[1][1][f]), (n, opts, f)
        assert out[0][2] == out[1][2], (n, opts)
        checked += 1
    assert checked >= 40, checked


def test_two_records_per_operation_loop_bit_equal_over_random_sizes_slices_and_splits(nbx):
    """The same for ONE body per lane (round 4): 50 seeded random combinations of ragged n, owned slice and j-split on the plain SGPR kernel
    -- the loop that packs records j and j + 1 of the pair-interleaved copy into every packed instruction against the compiled loop of plain
    instructions on the records themselves: accelerations and two steps, bit for bit (odd slice offsets, padding records, splits that begin
    and end inside the array)."""
    rng = np.random.default_rng(4242)
    for _ in range(50):
        n = int(rng.integers(300, 60000))
        blk = -(-n // 256) * 256 + 256 * int(rng.integers(0, 3))
        i_begin = int(rng.integers(0, max(1, n // 2)))
        i_count = int(rng.integers(1, n - i_begin + 1))
        S = int(rng.choice([1, 1, 2, 3, 5, 8]))
        opts = dict(kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=1, j_split=S, i_begin=i_begin, i_count=i_count, n_alloc=blk, use_graph=int(rng.choice([1, 2])))
        ic = nbx.initial_conditions(n)
        with nbx.Context(n, 32, inner_loop=nbx.LOOP_ASM, **opts) as ca, nbx.Context(n, 32, inner_loop=nbx.LOOP_CXX, **opts) as cc:
            out = []
            for c in (ca, cc):
                c.upload(ic)
                acc = c.accel()
                for _k in range(2):
                    c.step_local()
                    c.commit()
                out.append((acc, c.download(), c.kenergy_partial()))
            assert ca.stats()["inner_loop"] == nbx.LOOP_ASM and cc.stats()["inner_loop"] == nbx.LOOP_CXX and ca.stats()["bodies_per_lane"] == 1
        for q in range(3):
            assert np.array_equal(out[0][0][q], out[1][0][q]), (n, opts, q)
        for f in out[0][1]:
            assert np.array_equal(out[0][1][f], out[1][1][f]), (n, opts, f)
        assert out[0][2] == out[1][2], (n, opts)


@pytest.mark.parametrize("n,own,steps,B", [(262144, 262144, 2, 2), (262144, 262144, 1, 4), (131072, 131072, 3, 2), (16384, 16384, 12, 2),
                                            (4099, 4099, 25, 4), (524288, 65536, 1, 2)])
def test_time_sliced_wave_priority_changes_no_bit(nbx, n, own, steps, B):
    """NBX_LOOP_ASM_TS = the hand-scheduled loop plus, once per trip, an s_setprio decided by the clock and the wave's slot
    on its SIMD.  Priority only changes WHEN a wave issues, never what it computes: accelerations, trajectories and energies
    equal those of the plain asm loop and of the compiled loop bit for bit -- with two waves per SIMD (n = 262144, B = 2: 512
    workgroups), with one (262144 x B4, 131072 x B2: 256 workgroups), on small grids and on a slice of a larger system."""
    ic = nbx.initial_conditions(n)
    res = []
    for loop in (nbx.LOOP_ASM_TS, nbx.LOOP_ASM, nbx.LOOP_CXX, nbx.LOOP_ASM_PF):  # ASM_PF (round 4): the plain loop + one L2-prefetch load per trip
        with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=B, inner_loop=loop, use_graph=2, j_split=1,
                         i_begin=0, i_count=own, n_alloc=n) as c:
            c.upload(ic)
            acc = c.accel()
            for _ in range(steps):
                c.step_local()
                c.commit()
            part = c.kenergy_partial()
            st = c.stats()
            assert st["inner_loop"] == loop and st["bodies_per_lane"] == B and st["force_grid_y"] == 1
            res.append((acc, c.download(), part))
    for other in (1, 2, 3):
        for k in range(3):
            assert np.array_equal(res[0][0][k], res[other][0][k]), (other, "acc", k)
        for f in res[0][1]:
            assert np.array_equal(res[0][1][f], res[other][1][f]), (other, f)
        assert res[0][2] == res[other][2], other


def test_time_sliced_priority_with_every_slice_length(nbx, monkeypatch):
    """NBX_SLICE_BIT picks the clock bit of the slices (experiments); from 160 ns to 10 s per slice the bits stay the same."""
    n = 65536
    ic = nbx.initial_conditions(n)
    ref = None
    for k in (None, 4, 10, 20, 30):
        if k is None:
            monkeypatch.delenv("NBX_SLICE_BIT", raising=False)
        else:
            monkeypatch.setenv("NBX_SLICE_BIT", str(k))
        with nbx.Context(n, 32, kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=2, inner_loop=nbx.LOOP_ASM_TS, j_split=1) as c:
            c.upload(ic)
            ke = c.step_trace(3)
            got = c.download()
        if ref is None:
            ref = (ke, got)
        else:
            assert np.array_equal(ke, ref[0])
            for f in got:
                assert np.array_equal(got[f], ref[1][f]), (k, f)


def test_hand_scheduled_loop_is_the_default_where_it_exists(nbx):
    with nbx.Context(262144, 32) as c:  # configs[2]: reference order, SGPR kernel, packed math, two waves per SIMD
        st = c.stats()
        assert st["summation_order"] == nbx.ORDER_REFERENCE and st["inner_loop"] == nbx.LOOP_ASM_TS
    with nbx.Context(1048576, 32, i_begin=0, i_count=131072, n_alloc=1048576) as c:  # one rank of eight: one wave per SIMD
        st = c.stats()
        assert st["summation_order"] == nbx.ORDER_REFERENCE and st["inner_loop"] == nbx.LOOP_ASM_PF  # with the L2 prefetch
    with nbx.Context(1048576, 32) as c:  # four waves per SIMD: the plain loop
        assert c.stats()["inner_loop"] == nbx.LOOP_ASM
    with pytest.raises(nbx.NbxError):
        nbx.Context(65536, 32, kernel_variant=nbx.KERNEL_SGPRW, inner_loop=nbx.LOOP_ASM_TS)  # single-row SGPR kernel only
    with pytest.raises(nbx.NbxError):
        nbx.Context(65536, 32, kernel_variant=nbx.KERNEL_SGPRW, inner_loop=nbx.LOOP_ASM_PF)
    with nbx.Context(65536, 32) as c:  # tree order, wave-split kernel: 2048 records per split
        st = c.stats()
        assert st["kernel_variant"] == nbx.KERNEL_SGPRW and st["inner_loop"] == nbx.LOOP_ASM
    with nbx.Context(4099, 32, kernel_variant=nbx.KERNEL_LDS) as c:
        assert c.stats()["inner_loop"] == nbx.LOOP_CXX
    with pytest.raises(nbx.NbxError):
        nbx.Context(4099, 64, inner_loop=nbx.LOOP_ASM)  # no fp64 instance


# ---- one process per GPU (nbx_group_create_rank): the only form a 1-GPU box can run is a world of one ------------------
def test_rank_group_world_of_one_matches_a_plain_context(nbx):
    """ncclGetUniqueId -> ncclCommInitRank(1 rank) -> per-step in-place ncclAllGather, kenergy all-gather, velocity
    all-gather at download: every collective of the multi-process mode runs (with one participant) and the results are
    those of a plain context, bit for bit."""
    n, steps = 4099, 30
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, use_graph=2) as c:
        c.upload(ic)
        ke_ref = c.step(steps)
        ref = c.download()
    with nbx.Group(n, 32, n_ranks=1, rank=0, unique_id=nbx.unique_id(), device=0) as g:
        g.upload(ic)
        ke = g.step(steps)
        got = g.download()
        P, rccl, st = g.info(0)
        b, cnt, ms = g.shares()                       # a rank group knows the whole partition and its own timing (none: not profiled)
        assert b == [0] and cnt == [n] and ms == [0.0]
        with pytest.raises(nbx.NbxError):             # unequal shares exist for the single-process form only
            g.retune()
    assert P == 1 and rccl and st["i_count"] == n
    assert ke == ke_ref
    for f in ref:
        assert np.array_equal(got[f], ref[f]), f


def test_cli_one_process_per_gpu_mode_with_a_world_of_one(tmp_path):
    """NBODY_WORLD=1: nbody.x takes the multi-process path (rendezvous skipped for a single rank, RCCL communicator of one
    rank, collective energy and download) and prints what the single-process run prints."""
    import subprocess
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    out = str(tmp_path / "w1.json")
    p = subprocess.run([exe, "2000", "150"], env=dict(os.environ, NBODY_WORLD="1", NBODY_RANK="0", NBODY_JSON=out), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert [r[2] for r in _rows(lines)] == ["0.1432", "2.4341", "8.1256"]
    assert any("one process per rank" in ln and "RCCL" in ln for ln in lines)
    assert json.load(open(out))["exchange"] == "none"  # a single rank: nothing to exchange with


def test_rank_whose_peer_left_after_the_rendezvous_ends_with_status_75(tmp_path):
    """VERDICT r2 item 3 on the GPU: nbody.x as rank 0 of a world of two; "rank 1" is the rendezvous test driver, which says
    its hello, receives the RCCL token and exits -- a rank that died right after the rendezvous.  Rank 0 then sits alone in
    ncclCommInitRank (no kernel is in flight at that point).  The reference's MPI mode would wait for ever; here libnbx's
    watchdog ends the process with NBX_EXIT_COLLECTIVE_TIMEOUT and names the call."""
    import socket
    import subprocess
    import time
    host = os.path.join(ROOT, "nbody-demo-2023_amd", "host")
    drv = str(tmp_path / "rendezvous_driver.x")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I", host, os.path.join(ROOT, "tests", "rendezvous_driver.cpp"), "-o", drv, "-lpthread"])
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ, NBODY_WORLD="2", NBODY_RANK="0", NBODY_MASTER_PORT=port, NBODY_COLLECTIVE_TIMEOUT="2", NBODY_RENDEZVOUS_TIMEOUT="60",
               NBX_RCCL_INIT_ALLOWANCE="2")  # default 30 s on top of the timeout for RCCL's own set-up: 4 s in all here
    t0 = time.time()
    p0 = subprocess.Popen([os.path.join(host, "nbody.x"), "3000", "100"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    p1 = subprocess.run([drv, "1", "2", port, "3000", "60"], capture_output=True, text=True, timeout=120)  # signature (3000, 100, 32)
    assert p1.returncode == 0 and p1.stdout.startswith("ok "), (p1.stdout, p1.stderr)
    out, err = p0.communicate(timeout=120)
    assert p0.returncode == nbx_exit_collective_timeout(), (p0.returncode, err[-2000:])
    assert "rank 0 of 2 has been inside ncclCommInitRank" in err and "a peer rank is gone or never arrived" in err
    assert 3.5 < time.time() - t0 < 60  # the 2 s asked for + the allowance every ncclCommInitRank gets for RCCL's own set-up (2 s here)


def test_two_real_ranks_on_the_one_gpu_get_through_rendezvous_and_rccl_bootstrap(tmp_path):
    """The farthest two REAL nbody.x processes can go on a 1-GPU box: both draw the particles, rank 0 makes the RCCL token, the
    TCP rendezvous delivers it, both enter ncclCommInitRank and RCCL's own bootstrap connects them -- and then RCCL refuses the
    communicator because both ranks sit on device 0 (it has no notion of two ranks sharing a GPU).  What must hold: both processes
    end promptly with status 1 and RCCL's message (not a hang, not a crash, not the watchdog), and only rank 0 has printed."""
    import socket
    import subprocess
    import time
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ, NBODY_WORLD="2", NBODY_MASTER_PORT=port, NBODY_DEVICE="0", NBODY_COLLECTIVE_TIMEOUT="60", NBODY_RENDEZVOUS_TIMEOUT="60")
    t0 = time.time()
    ps = [subprocess.Popen([exe, "3000", "100"], env=dict(env, NBODY_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in (0, 1)]
    res = [p.communicate(timeout=150) + (p.returncode,) for p in ps]
    assert time.time() - t0 < 100
    for r, (out, err, rc) in enumerate(res):
        assert rc == 1, (r, rc, err[-1500:])
        assert "nbx_group_create_rank failed" in err and "ncclCommInitRank" in err, (r, err[-1500:])
        assert ("Initialize Gravity Simulation" in out) == (r == 0)


def test_watchdog_does_not_mistake_a_long_window_for_a_dead_peer(tmp_path):
    """The bound is on the collective, not on the work queued in front of it: with a 1 s timeout, print windows of ~2.3 s
    (n = 1048576, 10 steps of ~235 ms) must run to the end -- the deadline is the timeout plus the window's expected duration
    (a conservative rate before the first window has been timed, four times the measured step time afterwards; ncclCommInitRank
    has its own allowance for RCCL's set-up)."""
    import subprocess
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    out = str(tmp_path / "w.json")
    p = subprocess.run([exe, "1048576", "20"], env=dict(os.environ, NBODY_WORLD="1", NBODY_RANK="0", NBODY_COLLECTIVE_TIMEOUT="1", NBODY_SFREQ="10",
                                                        NBODY_JSON=out), capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, (p.returncode, p.stderr[-1500:])
    w = json.load(open(out))["windows"]
    assert [x["step"] for x in w] == [10, 20] and all(x["seconds"] > 1.5 for x in w)  # each window outlasts the bare timeout


def nbx_exit_collective_timeout():
    return 75  # NBX_EXIT_COLLECTIVE_TIMEOUT (include/nbx.h; tests/test_watchdog.py checks the header)


# ---- bench.py's N > 1 path, rehearsed on the one GPU: same launcher line as the driver's ----------------------------------
def _bench_under_torchrun(nproc, extra_env, args, port):
    import subprocess
    import sys
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + args
    p = subprocess.run(cmd, env=dict(os.environ, **extra_env), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # the contract: ONE JSON line on stdout, whatever the native libraries print
    return json.loads(lines[0])


def test_bench_n_gt_1_path_with_two_ranks_sharing_the_gpu(nbx, tmp_path):
    """Two ranks under torch.distributed.run, gloo for the exchange because RCCL refuses two ranks on one device: partition,
    per-step all-gather, max-over-ranks timing and the energy all-reduce of bench.py's multi-GPU branch, checked against a
    single context stepping the same system (same summation order for every rank count: bit-equal kenergy)."""
    n, steps, warmup = 16384, 4, 2
    line = _bench_under_torchrun(2, {"NBX_BENCH_BACKEND": "gloo"}, ["--bodies", str(n), "--steps", str(steps), "--warmup", str(warmup),
                                                                     "--cpu-baseline", "none", "--full",
                                                                     "--dump-outputs", str(tmp_path)], 29531)
    assert line["n_gpus"] == 2 and line["steps"] == steps and line["scaling"] == "strong" and line["value"] > 0
    assert line["config"]["n_bodies"] == n and line["config"]["bodies_per_gpu"] == n // 2
    with nbx.Context(n, 32) as c:
        c.upload(nbx.initial_conditions(n))
        ke = c.step(steps + warmup)
    assert rel_err(line["kenergy_after_run"], ke) < 1e-6, (line["kenergy_after_run"], ke)
    _check_dumped_outputs(nbx, tmp_path, line, steps + warmup)  # rank 1's velocities gathered to rank 0 at their offset
    # an N > 1 line validates itself -- parity of this very multi-rank form against the reference's trace ...
    par = line["parity"]
    assert par["fixture"] == "ver7_f32_n16384_s500.json" and par["steps"] == 10 and par["ranks"] == 2
    assert par["pass"] and par["max_rel_kenergy_err"] < 1e-4 and len(par["rel_kenergy_err_per_step"]) == 10
    # ... and says what every rank did
    rk = line["ranks"]
    assert rk["world_seen"] == 2 and rk["backend"].startswith("gloo") and [r["rank"] for r in rk["per_rank"]] == [0, 1]
    assert [r["bodies_owned"] for r in rk["per_rank"]] == [n // 2, n // 2] and all(r["device"] == 0 for r in rk["per_rank"])
    assert rk["bytes_gathered_per_step"] == (n // 2) * 16 == rk["bytes_sent_per_step"]
    f, g = rk["force_kernel_ms"], rk["allgather_ms_per_step"]
    assert 0 < f["min"] <= f["mean"] <= f["max"] and 0 < g["min"] <= g["mean"] <= g["max"] <= rk["allgather_ms_worst_step"]
    assert rk["skew_ms"] == pytest.approx(f["max"] - f["min"]) and 0 < rk["allgather_share_of_step"] < 1
    assert "skipped" in line["native_rank_group"]  # RCCL cannot form a communicator of two ranks on one device
    assert "skipped" in line["native_single_process"] and line["value_native_single_process"] is None
    assert line["one_gpu_at_multi_gpu_n"]["n_bodies"] == n and line["speedup_vs_one_gpu_same_n"] > 0
    assert line["roofline"]["traffic"] is None and line["roofline"]["traffic_note"]


def test_bench_n_gt_1_path_over_rccl_with_a_world_of_one(nbx, tmp_path):
    """The same branch over the real backend ("nccl" = RCCL), which a 1-GPU box can only run with one rank:
    init_process_group(device_id), in-place all_gather_into_tensor on the device buffer, all_reduce of the timing and energy."""
    n, steps, warmup = 16384, 4, 2
    line = _bench_under_torchrun(1, {"NBX_BENCH_FORCE_DIST": "1"}, ["--bodies", str(n), "--steps", str(steps), "--warmup", str(warmup),
                                                                     "--cpu-baseline", "none", "--full",
                                                                     "--dump-outputs", str(tmp_path)], 29533)
    assert line["n_gpus"] == 1 and line["value"] > 0
    with nbx.Context(n, 32) as c:
        c.upload(nbx.initial_conditions(n))
        ke = c.step(steps + warmup)
        c.upload(nbx.initial_conditions(n))
        ke10 = c.step(10)
    assert rel_err(line["kenergy_after_run"], ke) < 1e-6, (line["kenergy_after_run"], ke)
    _check_dumped_outputs(nbx, tmp_path, line, steps + warmup)  # the velocity gather over RCCL
    rk = line["ranks"]
    assert rk["world_seen"] == 1 and rk["backend"].startswith("nccl") and rk["bytes_gathered_per_step"] == 0
    assert rk["allgather_ms_per_step"]["mean"] > 0 and rk["force_kernel_ms"]["mean"] > 0 and rk["skew_ms"] == 0
    assert line["parity"]["pass"] and line["parity"]["ranks"] == 1
    # the drop-in's own multi-process path (nbody.x: nbx_group_create_rank + in-place ncclAllGather inside libnbx) ran as a
    # child on the same GPU and agrees with the torch.distributed path of the line
    nat = line["native_rank_group"]
    assert nat["returncodes"] == [0] and nat["uses_rccl"] and nat["one_process_per_rank"] and nat["ms_per_step"] > 0, nat
    assert nat["kenergy_equal_to_torch_path"] and nat["rel_diff_vs_torch_path"] < 1e-12
    assert rel_err(nat["kenergy_step10"], ke10) < 1e-12
    assert nat["rel_kenergy_err_vs_reference_step10"] < 1e-4
    # the product's single-process form (nbody.x with NBODY_GPUS = the job's GPUs: nbx_group_create -> ncclCommInitAll ->
    # grouped in-place ncclAllGather per step) is a timed leg of the N > 1 line too, beside the rank-group leg and the torch figure, and
    # the line carries its own one-GPU denominator
    one = line["native_single_process"]
    assert one["returncode"] == 0 and one["uses_rccl"] and not one["one_process_per_rank"] and one["gpus"] == 1 and one["ms_per_step"] > 0, one
    assert one["kenergy_equal_to_torch_path"] and rel_err(one["kenergy_step10"], ke10) < 1e-12 and one["rel_kenergy_err_vs_reference_step10"] < 1e-4
    assert line["value_native_single_process"] == one["pair_per_s"] > 0 and line["value_native_rank_group"] == nat["pair_per_s"] > 0
    assert line["value_torch_distributed"] == line["value"]
    same = line["one_gpu_at_multi_gpu_n"]
    assert same["n_bodies"] == n and same["ms_per_step"] > 0 and abs(line["speedup_vs_one_gpu_same_n"] * line["ms_per_step"] / same["ms_per_step"] - 1) < 1e-9
