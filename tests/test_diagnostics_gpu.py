"""Physics diagnostics on the MI355X (include/nbx_diag.h): values against the fp64 numpy restatement (energy_ref.py), the j != i
rule, determinism and independence of the launch shape, no effect on the trajectory, energy conservation, groups, the CLI
knob NBODY_ENERGY and the cost of one call."""
import json
import os
import subprocess
import time
import zlib

import numpy as np
import pytest

import energy_ref
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

SCALARS = ("mass", "kenergy", "potential", "etotal")


def _crc(state):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(state[f]).tobytes()) for f in sorted(state)]


def _with_mass(state, ic):
    s = dict(state)
    s["mass"] = ic["mass"]
    return s


def _check_against_ref(d, ref, pscale, pot_tol):
    assert rel_err(d["potential"], ref["potential"]) < pot_tol, (d["potential"], ref["potential"])
    for k in ("mass", "kenergy"):
        assert rel_err(d[k], ref[k]) < 1e-12, (k, d[k], ref[k])
    assert np.abs(np.subtract(d["momentum"], ref["momentum"])).max() < 1e-12 * pscale
    assert rel_err(d["mass_moment"], ref["mass_moment"]).max() < 1e-12
    assert d["etotal"] == d["kenergy"] + d["potential"]


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 1000, 4099, 16384])
def test_initial_state_matches_numpy(nbx, n, precision):
    ic = nbx.initial_conditions(n, precision)
    with nbx.Context(n, precision, device=0) as c:
        c.upload(ic)
        d = c.diagnostics()
    ref = energy_ref.diagnostics(ic)
    _check_against_ref(d, ref, energy_ref.momentum_scale(ic), 1e-5 if precision == 32 else 1e-12)
    assert d["i_count"] == n and d["steps_done"] == 0


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("n,i_begin,i_count", [(1000, 100, 700), (4099, 1000, 3099), (5000, 300, 1)])
def test_unaligned_slice_partials_match_numpy(nbx, n, i_begin, i_count, precision):
    """A context owning a slice that does not start on a 256-record tile: its workgroups straddle B + 1 masked tiles and
    index posm / velm with an offset."""
    ic = nbx.initial_conditions(n, precision)
    with nbx.Context(n, precision, device=0, i_begin=i_begin, i_count=i_count) as c:
        c.upload(ic)
        d = c.diagnostics()
    ref = energy_ref.diagnostics(ic, i_begin, i_count)
    _check_against_ref(d, ref, energy_ref.momentum_scale(ic), 1e-5 if precision == 32 else 1e-12)
    assert d["i_count"] == i_count


@pytest.mark.parametrize("precision", [32, 64])
def test_hand_placed_bodies_match_the_closed_form(nbx, precision):
    """Two bodies one unit apart, plus two DISTINCT bodies at one position (included, softened) -- and no self term."""
    dt = np.float32 if precision == 32 else np.float64
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]])
    m = np.array([2.0, 3.0, 1.0, 4.0], dtype=dt)
    vel = np.array([[1.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 0.5], [0.25, 0.0, 0.0]])
    st = {"pos_x": pos[:, 0].astype(dt), "pos_y": pos[:, 1].astype(dt), "pos_z": pos[:, 2].astype(dt),
          "vel_x": vel[:, 0].astype(dt), "vel_y": vel[:, 1].astype(dt), "vel_z": vel[:, 2].astype(dt), "mass": m}
    gm = energy_ref.gm_as_uploaded(m)
    eps2 = energy_ref.EPS2
    u = 0.0
    for i in range(4):
        for j in range(4):
            if i != j:
                r2 = float(((pos[i] - pos[j]) ** 2).sum())
                u += -0.5 * float(m[i]) * gm[j] / np.sqrt(r2 + eps2)
    with nbx.Context(4, precision, device=0) as c:
        c.upload(st)
        d = c.diagnostics()
    assert rel_err(d["potential"], u) < (1e-6 if precision == 32 else 1e-14), (d["potential"], u)
    assert d["mass"] == 10.0
    assert rel_err(d["kenergy"], 0.5 * (2 * 1 + 3 * 4 + 1 * 0.25 + 4 * 0.0625)) < 1e-15
    assert np.allclose(d["momentum"], [2.0 + 1.0, -6.0, 0.5], rtol=0, atol=1e-15)
    assert np.allclose(d["mass_moment"], [3.0 + 2.5, 2.5, 2.5], rtol=0, atol=1e-15)


def test_large_n_fp32_potential_matches_fp64(nbx):
    n = 262144
    vals = {}
    for precision in (32, 64):
        with nbx.Context(n, precision, device=0) as c:
            c.upload(nbx.initial_conditions(n, precision))
            vals[precision] = c.diagnostics()
    assert rel_err(vals[32]["potential"], vals[64]["potential"]) < 1e-5, (vals[32]["potential"], vals[64]["potential"])


def test_result_is_independent_of_the_force_options_and_repeatable(nbx):
    n = 4099
    ic = nbx.initial_conditions(n)
    shapes = [dict(kernel_variant=k, summation_order=o)
              for k in (nbx.KERNEL_LDS, nbx.KERNEL_SGPR, nbx.KERNEL_SGPRW, nbx.KERNEL_JLANE, nbx.KERNEL_EXACT)
              for o in (nbx.ORDER_REFERENCE, nbx.ORDER_TREE)]
    shapes += [dict(kernel_variant=nbx.KERNEL_SGPR, bodies_per_lane=1), dict(kernel_variant=nbx.KERNEL_LDS, j_split=4, bodies_per_lane=4)]
    got, made = [], []
    for opts in shapes:
        try:
            c = nbx.Context(n, 32, device=0, **opts)
        except nbx.NbxError:  # a combination the force kernels do not offer (e.g. jlane in reference order)
            continue
        with c:
            c.upload(ic)
            d = [c.diagnostics() for _ in range(3)]
        assert d[0] == d[1] == d[2], opts  # repeated calls: the same bits
        got.append(d[0])
        made.append(opts)
    assert len(made) >= 8, made
    assert {o["kernel_variant"] for o in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR, nbx.KERNEL_SGPRW, nbx.KERNEL_JLANE, nbx.KERNEL_EXACT}
    assert {o.get("summation_order") for o in made} >= {nbx.ORDER_REFERENCE, nbx.ORDER_TREE}
    for d, opts in zip(got, made):
        assert d == got[0], opts


def test_state_errors(nbx):
    with nbx.Context(1000, 32, device=0) as c:
        with pytest.raises(nbx.NbxError) as e:
            c.diagnostics()
        assert e.value.code == nbx.NBX_ERR_STATE
    n, blk = 1000, 512
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, device=0, i_begin=0, i_count=blk, n_alloc=2 * blk) as c:
        c.upload(ic)
        c.step_local()
        with pytest.raises(nbx.NbxError) as e:
            c.diagnostics()
        assert e.value.code == nbx.NBX_ERR_STATE
        c.commit()
        d = c.diagnostics()  # the owned slice's partials after the commit
        assert d["i_count"] == blk and d["steps_done"] == 1
    with nbx.Group(n, 32, n_ranks=2, devices=[0, 0]) as g:
        with pytest.raises(nbx.NbxError) as e:
            g.diagnostics()
        assert e.value.code == nbx.NBX_ERR_STATE


def test_diagnostics_do_not_change_the_trajectory(nbx):
    n = 2000
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, device=0) as c:
        c.upload(ic)
        c.step(50)
        c.diagnostics()
        c.step(50)
        a = c.download()
    with nbx.Context(n, 32, device=0) as c:
        c.upload(ic)
        c.step(100)
        b = c.download()
    assert _crc(a) == _crc(b)


@pytest.mark.parametrize("precision", [32, 64])
def test_after_stepping_matches_numpy_and_the_step_energy(nbx, precision):
    n, steps = 2000, 100
    ic = nbx.initial_conditions(n, precision)
    with nbx.Context(n, precision, device=0) as c:
        c.upload(ic)
        ke = c.step(steps)
        d = c.diagnostics()
        state = _with_mass(c.download(), ic)
    assert d["steps_done"] == steps
    assert rel_err(d["kenergy"], ke) < 1e-12, (d["kenergy"], ke)
    _check_against_ref(d, energy_ref.diagnostics(state), energy_ref.momentum_scale(state), 1e-5 if precision == 32 else 1e-12)


def test_energy_is_conserved_over_100_steps(nbx):
    n = 2000
    with nbx.Context(n, 32, device=0) as c:
        c.upload(nbx.initial_conditions(n))
        e0 = c.diagnostics()["etotal"]
        c.step(100)
        e1 = c.diagnostics()["etotal"]
    drift = abs(e1 - e0) / abs(e0)
    print("n = 2000 fp32: E(0) = %.7f, E(100) = %.7f, drift %.2e" % (e0, e1, drift))
    assert drift <= 1e-3


def _close(a, b, tol=1e-12):
    for k in SCALARS:
        assert rel_err(a[k], b[k]) < tol, (k, a[k], b[k])
    for k in ("momentum", "mass_moment"):
        assert rel_err(a[k], b[k]).max() < tol or np.abs(np.subtract(a[k], b[k])).max() < tol * max(1.0, np.abs(b[k]).max()), k


@pytest.mark.parametrize("form", ["equal", "weighted"])
def test_logical_rank_groups_total_the_single_context(nbx, form):
    # reference summation order: the trajectory is the same bit for bit whoever owns a body, so only the sums of the
    # partials can differ (in the last bits of fp64)
    n, steps = 4099, 20
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, device=0, summation_order=nbx.ORDER_REFERENCE) as c:
        c.upload(ic)
        c.step(steps)
        ref = c.diagnostics()
    kw = dict(weights=[1, 2, 1]) if form == "weighted" else {}
    with nbx.Group(n, 32, n_ranks=3, devices=[0, 0, 0], summation_order=nbx.ORDER_REFERENCE, **kw) as g:
        g.upload(ic)
        g.step(steps)
        d = g.diagnostics()
        assert g.diagnostics() == d
        P = g.info(0)[0]
    assert P == 3
    assert d["i_count"] == n and d["steps_done"] == steps
    _close(d, ref)


def test_rank_group_of_one_gives_the_single_context_value(nbx):
    n, steps = 4099, 30
    ic = nbx.initial_conditions(n)
    with nbx.Context(n, 32, use_graph=2) as c:
        c.upload(ic)
        c.step(steps)
        ref = c.diagnostics()
    with nbx.Group(n, 32, n_ranks=1, rank=0, unique_id=nbx.unique_id(), device=0) as g:
        g.upload(ic)
        g.step(steps)
        d = g.diagnostics()
    assert d["i_count"] == n and d["steps_done"] == steps
    _close(d, ref)


def _table_rows(stdout):
    import re
    return [m.groups() for m in (re.match(r"^ (\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s*$", ln) for ln in stdout.splitlines()) if m]


def test_cli_energy_knob(nbx, tmp_path):
    exe = os.path.join(ROOT, "nbody-demo-2023_amd", "host", "nbody.x")
    plain_json, energy_json = str(tmp_path / "plain.json"), str(tmp_path / "energy.json")
    env = {k: v for k, v in os.environ.items() if k != "NBODY_ENERGY"}
    p0 = subprocess.run([exe, "2000", "100"], env=dict(env, NBODY_JSON=plain_json), capture_output=True, text=True, timeout=300)
    p1 = subprocess.run([exe, "2000", "100"], env=dict(env, NBODY_JSON=energy_json, NBODY_ENERGY="1"), capture_output=True, text=True,
                        timeout=300)
    assert p0.returncode == 0 and p1.returncode == 0, (p0.stderr, p1.stderr)
    r0, r1 = _table_rows(p0.stdout), _table_rows(p1.stdout)
    assert len(r0) == 2 and [r[:3] for r in r0] == [r[:3] for r in r1]  # s, dt, kenergy columns unchanged
    assert "# Energy" not in p0.stdout
    last = p1.stdout.splitlines()[-1]
    assert last.startswith("# Energy             : E(0) = ") and "drift" in last and "sqrt(2 M K)" in last
    j0, j1 = json.load(open(plain_json)), json.load(open(energy_json))
    assert "energy_initial" not in j0 and all("potential" not in w for w in j0["windows"])
    w = j1["windows"][0]
    assert set(w) >= {"potential", "etotal", "momentum"} and len(w["momentum"]) == 3
    assert w["etotal"] == w["kenergy"] + w["potential"]
    with nbx.Context(2000, 32, device=0) as c:
        c.upload(nbx.initial_conditions(2000))
        e0 = c.diagnostics()["etotal"]
        c.step(w["step"])
        d = c.diagnostics()
    assert w["potential"] == d["potential"] and w["momentum"] == d["momentum"]
    assert j1["energy_initial"] == e0


def test_cost_of_one_call_at_n_262144(nbx):
    """Deliberately loose gate on a shared pool: one diagnostics call under three default force steps (tools/diag_cost.py
    prints the measured ratio)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import diag_cost
    r = diag_cost.measure(nbx, 262144, steps=6, calls=4)
    print("n = 262144 fp32: step %.3f ms, diagnostics %.3f ms, ratio %.3f" % (r["step_ms"], r["diag_ms"], r["ratio"]))
    assert r["ratio"] < 3.0
