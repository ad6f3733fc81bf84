"""Per-member diagnostics of an ensemble on the device (include/nbx_ensemble_diag.h).  The contract needs no tolerance: the
entry of a member is, field for field and bit for bit, what nbx_diagnostics returns for an nbx_ctx of n bodies holding that
member's state.  Member states are those of test_ensemble_gpu.member_states -- slices of a large seed-42 system, with the
seed-42 system of n bodies as the LAST member so that a wrong stride cannot pass.  Beyond bit equality: the values against the
fp64 numpy restatement and a closed form, ranges, repeatability, independence of the member's place, no effect on the
trajectory, stream order, the error paths, energy conservation and the cost against one call per context."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

import energy_ref
from conftest import ROOT, rel_err
from test_diagnostics_gpu import _check_against_ref
from test_ensemble_gpu import ARRAYS, member_states

pytestmark = pytest.mark.gpu

F32_CASES = [(5, 3, 20), (65, 7, 20), (2000, 16, 60), (2048, 64, 20), (4099, 9, 40), (16383, 2, 4)]
F64_CASES = [(5, 3, 20), (2000, 8, 40), (12288, 2, 4)]


def _member_state(nbx, down, m, state):
    """Member m of an Ensemble.download() as a state dict, with the masses it was uploaded with."""
    s = {f: down[f][m].copy() for f in ARRAYS}
    s["mass"] = state["mass"]
    return s


def _without_steps(d):
    return {k: v for k, v in d.items() if k != "steps_done"}


def assert_members_equal_contexts(nbx, n, S, steps, precision):
    states = member_states(nbx, n, S, precision)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        st = e.stats()
        d0 = e.diagnostics()
        e.step(steps, kenergy=False)
        d1 = e.diagnostics()
        down = e.download()
    assert len(d0) == len(d1) == S
    NB, loop = st["bodies_per_lane"], st["inner_loop"]
    for m in range(S):
        with nbx.Context(n, precision, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
            c.upload(states[m])
            c0 = c.diagnostics()
            c.step(steps, kenergy=False)
            c1 = c.diagnostics()
            cst = c.stats()
        assert cst["bodies_per_lane"] == NB and cst["inner_loop"] == loop and cst["force_grid_x"] == st["grid_x"]
        assert c0["i_count"] == n and c0["steps_done"] == 0 and c1["steps_done"] == steps
        assert d0[m] == c0, (n, S, m, "step 0", d0[m], c0)
        assert d1[m] == c1, (n, S, m, "step %d" % steps, d1[m], c1)
        # a default context that never stepped, holding the member's downloaded state: the same bits, whatever its force options
        with nbx.Context(n, precision) as c:
            c.upload(_member_state(nbx, down, m, states[m]))
            cd = c.diagnostics()
        assert cd["steps_done"] == 0
        assert _without_steps(d1[m]) == _without_steps(cd), (n, S, m, "downloaded", d1[m], cd)


@pytest.mark.parametrize("n,S,steps", F32_CASES)
def test_every_member_is_bit_equal_to_the_diagnostics_of_a_context_fp32(nbx, n, S, steps):
    assert_members_equal_contexts(nbx, n, S, steps, 32)


@pytest.mark.parametrize("n,S,steps", F64_CASES)
def test_every_member_is_bit_equal_to_the_diagnostics_of_a_context_fp64(nbx, n, S, steps):
    assert_members_equal_contexts(nbx, n, S, steps, 64)


@pytest.mark.parametrize("precision,n,S,steps", [(32, 2000, 5, 60), (64, 2000, 4, 40)])
def test_after_stepping_matches_numpy_and_the_step_energy(nbx, precision, n, S, steps):
    """The gates of test_diagnostics_gpu._check_against_ref (potential 1e-5 fp32 / 1e-12 fp64, the other fields 1e-12) for every
    member, and the gate of test_after_stepping_matches_numpy_and_the_step_energy between kenergy and the step's own."""
    states = member_states(nbx, n, S, precision)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        ke = e.step(steps)
        d = e.diagnostics()
        down = e.download()
    for m in range(S):
        assert d[m]["steps_done"] == steps and d[m]["i_count"] == n
        assert rel_err(d[m]["kenergy"], ke[m]) < 1e-12, (m, d[m]["kenergy"], ke[m])
        state = _member_state(nbx, down, m, states[m])
        _check_against_ref(d[m], energy_ref.diagnostics(state), energy_ref.momentum_scale(state), 1e-5 if precision == 32 else 1e-12)


@pytest.mark.parametrize("precision", [32, 64])
def test_hand_placed_member_matches_the_closed_form(nbx, precision):
    """The 4-body system of test_hand_placed_bodies_match_the_closed_form as member 1 of 3: two bodies one unit apart, plus two
    DISTINCT bodies at one position (included, softened) -- and no self term.  That test's tolerances."""
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
    states = member_states(nbx, 4, 3, precision)
    states[1] = st
    with nbx.Ensemble(4, 3, precision) as e:
        e.upload(states)
        d = e.diagnostics()[1]
    assert rel_err(d["potential"], u) < (1e-6 if precision == 32 else 1e-14), (d["potential"], u)
    assert d["mass"] == 10.0
    assert rel_err(d["kenergy"], 0.5 * (2 * 1 + 3 * 4 + 1 * 0.25 + 4 * 0.0625)) < 1e-15
    assert np.allclose(d["momentum"], [2.0 + 1.0, -6.0, 0.5], rtol=0, atol=1e-15)
    assert np.allclose(d["mass_moment"], [3.0 + 2.5, 2.5, 2.5], rtol=0, atol=1e-15)
    assert d["i_count"] == 4 and d["steps_done"] == 0


@pytest.mark.parametrize("precision,n,S,steps", [(32, 2000, 16, 30), (32, 65, 7, 20), (64, 2000, 8, 20)])
def test_ranges_repeats_and_member_order(nbx, precision, n, S, steps):
    states = member_states(nbx, n, S, precision)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        e.step(steps, kenergy=False)
        full = e.diagnostics()
        assert e.diagnostics() == full and e.diagnostics() == full  # repeated calls: the same bits
        for a, c in ((0, 1), (1, 2), (S - 1, 1), (S // 2, S - S // 2), (3, 0), (S, 0)):
            assert e.diagnostics(first=a, count=c) == full[a:a + c], (a, c)
        assert e.diagnostics(first=2) == full[2:]
        assert e.diagnostics() == full  # a partial call leaves nothing behind that a full one sees
    with nbx.Ensemble(n, S, precision) as e:  # system k at member S - 1 - k
        e.upload(states[::-1])
        e.step(steps, kenergy=False)
        assert e.diagnostics() == full[::-1]


def _crc(down):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(down[f]).tobytes()) for f in ARRAYS]


def test_diagnostics_do_not_change_the_trajectory(nbx):
    n, S = 2000, 6
    states = member_states(nbx, n, S, 32)
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(states)
        ke_a = [e.step(50)]
        e.diagnostics()
        e.diagnostics(first=2, count=3)
        ke_a.append(e.step(50))
        a = e.download()
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(states)
        ke_b = [e.step(50), e.step(50)]
        b = e.download()
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(states)
        ke_c = e.step(100)
        c = e.download()
    assert _crc(a) == _crc(b) == _crc(c)
    assert np.array_equal(ke_a, ke_b) and np.array_equal(ke_a[1], ke_c)


def test_the_call_is_ordered_on_the_ensembles_stream(nbx):
    n, S = 2048, 8
    states = member_states(nbx, n, S, 32)
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(states)
        d0 = e.diagnostics()
        assert e.step(10, kenergy=False) is None  # asynchronous
        d = e.diagnostics()
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(states)
        e.step(10)  # synchronises
        e.sync()
        ref = e.diagnostics()
    assert all(x["steps_done"] == 10 for x in d)
    assert d == ref
    assert all(x["potential"] != y["potential"] and x["kenergy"] != y["kenergy"] for x, y in zip(d, d0))


def test_state_and_argument_errors(nbx):
    n, S = 300, 4
    L = nbx.load()
    states = member_states(nbx, n, S, 32)
    with nbx.Ensemble(n, S, 32) as e:
        with pytest.raises(nbx.NbxError) as err:
            e.diagnostics()
        assert err.value.code == nbx.NBX_ERR_STATE and "member 0" in str(err.value)
        e.upload(states[:3])
        with pytest.raises(nbx.NbxError) as err:
            e.diagnostics()
        assert err.value.code == nbx.NBX_ERR_STATE and "member 3" in str(err.value)
        with pytest.raises(nbx.NbxError) as err:
            e.diagnostics(first=2, count=2)
        assert err.value.code == nbx.NBX_ERR_STATE
        part = e.diagnostics(first=0, count=3)  # the uploaded members can be asked before the others arrive
        assert len(part) == 3 and all(d["i_count"] == n and d["steps_done"] == 0 for d in part)
        for first, count in ((-1, 1), (0, S + 1), (S, 1), (2, 3), (0, -1), (S + 1, 0)):
            with pytest.raises(nbx.NbxError) as err:
                e.diagnostics(first=first, count=count)
            assert err.value.code == nbx.NBX_ERR_ARG, (first, count, str(err.value))
        one = nbx.Diag()  # first + count beyond 31 bits: the range check does not wrap
        assert L.nbx_ensemble_diagnostics(e._h, 2 ** 31 - 1, 2 ** 31 - 1, ctypes.byref(one)) == nbx.NBX_ERR_ARG
        e.upload(states[3:], first=3)
        assert e.diagnostics(first=0, count=3) == part
        # count == 0: OK, nothing written
        d = (nbx.Diag * 3)()
        d[0].mass = -7.0
        assert L.nbx_ensemble_diagnostics(e._h, 1, 0, d) == nbx.NBX_OK
        assert d[0].mass == -7.0 and d[0].struct_size == 0
        assert e.diagnostics(first=S, count=0) == []
        # a wrong struct_size in out[1]: NBX_ERR_ARG, nothing written
        d[1].struct_size = ctypes.sizeof(nbx.Diag) - 8
        assert L.nbx_ensemble_diagnostics(e._h, 0, 3, d) == nbx.NBX_ERR_ARG
        assert b"struct_size" in L.nbx_last_error() and d[0].mass == -7.0 and d[2].i_count == 0
        # struct_size 0 is "this version"; it is set on return
        d[1].struct_size = 0
        assert L.nbx_ensemble_diagnostics(e._h, 0, 3, d) == nbx.NBX_OK
        assert [d[k].struct_size for k in range(3)] == [ctypes.sizeof(nbx.Diag)] * 3
        assert [d[k].asdict() for k in range(3)] == part


def test_energy_is_conserved_over_100_steps(nbx):
    """The last member is the seed-42 system of 2000 bodies, the run test_energy_is_conserved_over_100_steps gates: its drift is
    gated at that test's 1e-3.  The other members' drifts have not been measured before: printed, not gated."""
    n, S = 2000, 6
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(member_states(nbx, n, S, 32))
        e0 = [d["etotal"] for d in e.diagnostics()]
        e.step(100, kenergy=False)
        e1 = [d["etotal"] for d in e.diagnostics()]
    drift = [abs(b - a) / abs(a) for a, b in zip(e0, e1)]
    for m in range(S):
        print("n = 2000 fp32 member %d: E(0) = %.7f, E(100) = %.7f, drift %.2e" % (m, e0[m], e1[m], drift[m]))
    assert drift[-1] <= 1e-3, drift[-1]


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """64 x 2048 fp32: one nbx_ensemble_diagnostics over all members against 64 nbx_diagnostics calls on 64 contexts that were
    created and uploaded beforehand, in this process, rounds alternated (tools/ensemble_diag_cost.py).  The contexts are not
    charged for download, create or upload, so the gate has no further margin: ratio <= 1.0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ensemble_diag_cost
    r = ensemble_diag_cost.measure(nbx, 2048, 64)
    print("64 x 2048 fp32: ensemble %.1f us, 64 contexts %.1f us, ratio %.3f" % (r["ensemble_us"], r["contexts_us"], r["ratio"]))
    ensemble_diag_cost.write(ensemble_diag_cost.OUT, gate=r)
    assert r["same_values_from_both_arms"]
    assert r["ratio"] <= 1.0, r
