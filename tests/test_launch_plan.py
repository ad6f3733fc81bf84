"""The launch plan of nbx_create -- kernel variant, summation order, bodies per lane, j-splits, epilogue, inner loop, grid,
graph replay -- against tests/golden/launch_plans.json, which was recorded on an MI355X (256 CUs) from nbx_ctx itself.

On the device: every row of n <= 1M through nbx.Context, compared on what nbx_stats shows.  On the CPU: the host-only planner
(csrc/nbx_plan.hpp) through a small g++ driver, compared on every field, the error texts and the tuner's cost model; the
driver also walks the whole cross product of the nbx_opts shape fields and checks that every plan it can produce names a
kernel instance that is compiled."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

FIXTURE = "launch_plans.json"
CSRC = os.path.join(ROOT, "nbody-demo-2023_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "plan_driver.cpp")
# internal LOOP_* of the plan -> the NBX_LOOP_* nbx_stats reports
STATS_LOOP = {0: 1, 1: 2, 2: 3, 3: 4}


def _opts(d, row):
    return dict(zip(d["inputs"][2:], row[2:13]))


@pytest.mark.gpu
def test_recorded_launch_plans_on_the_device(nbx):
    d = load_golden(FIXTURE)
    plan = d["plan"]
    bad, checked = [], 0
    for row in d["rows"]:
        n, prec, want = row[0], row[1], row[13]
        if n > 1 << 20:
            continue
        checked += 1
        try:
            with nbx.Context(n, prec, **_opts(d, row)) as c:
                st = c.stats()
        except nbx.NbxError as e:
            got = ("error", e.code, str(e))
        else:
            assert st["cu_count"] == d["cu_count"], st["cu_count"]
            got = (st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"], st["fused_epilogue"],
                   st["inner_loop"], st["force_grid_x"], st["force_grid_y"], st["use_graph"])
        if len(want) == 2:
            exp = ("error", want[0], "nbx_create failed (%d): %s" % (want[0], d["messages"][want[1]]))
        else:
            p = dict(zip(plan, want))
            exp = (p["variant"], p["order"], p["B"], p["S"], p["epi"], STATS_LOOP[p["loop"]], p["grid_x"], p["grid_y"], p["use_graph"])
        if got != exp:
            bad.append((row[:13], exp, got))
    assert checked > 1000, checked
    assert not bad, (len(bad), bad[:5])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The planner alone: g++ compiles csrc/nbx_plan.hpp without ROCm."""
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def declared_instances(exe):
    """kInstances of nbx_plan.hpp as (kind, precision, B, jsrc, epi, math, ws, loop) tuples."""
    out = subprocess.run([exe, "instances"], capture_output=True, text=True, check=True).stdout
    return [tuple(map(int, line.split())) for line in out.splitlines()]


def test_planner_reproduces_every_recorded_plan(driver):
    """Every row of the fixture, every plan field (j records per split, math, the pair-interleaved copy included), every error text,
    and the tuner's cost model at each recorded `own`."""
    d = load_golden(FIXTURE)
    costs = {row: values for row, values in d["costs"]}
    rows = "".join(" ".join(map(str, r[:13])) + " %d\n" % (i in costs) for i, r in enumerate(d["rows"]))
    out = subprocess.run([driver, "rows", str(d["cu_count"])], input=rows, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(d["rows"])
    for i, (row, line) in enumerate(zip(d["rows"], out)):
        want = row[13]
        if len(want) == 2:
            assert line == "E %d %s" % (want[0], d["messages"][want[1]]), (row[:13], line)
            continue
        kind, *vals = line.split()
        assert kind == "P" and dict(zip(d["plan"], map(int, vals[:12]))) == dict(zip(d["plan"], want)), (row[:13], line)
        if i in costs:
            assert [float(x) for x in vals[12:]] == costs[i], (row[:13], vals[12:])
        else:
            assert len(vals) == 12


def test_every_plan_of_every_option_names_a_compiled_instance(driver):
    """The whole cross product of the nbx_opts shape fields, out-of-range values included, at sizes and slices on both sides of the
    thresholds and for both precisions: the step kernel and nbx_accel's form of every plan are in the declared instance set, so
    nbx_create never hands a context to a launch that does not exist."""
    r = subprocess.run([driver, "cross", "256"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    plans = int(r.stdout.split()[0])
    assert plans > 1000000, r.stdout


def test_declared_instances_are_distinct(driver):
    inst = declared_instances(driver)
    assert len(inst) == len(set(inst)) == 60, len(inst)
