"""Ensembles on the device (include/nbx_ensemble.h): every member of an ensemble must come out bit for bit as a single nbx_ctx
of the same shape does -- positions, velocities and the kinetic energy of every step -- and the reference's own seed-42
system, placed as the LAST member so that a wrong stride cannot pass, must meet the reference's fixtures within the
project's existing gates for the one-launch kernel."""
import numpy as np
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

ARRAYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z")


def member_states(nbx, n, S, precision):
    """Member m = bodies [m n, (m + 1) n) of the seed-42 system of S n bodies; the last member is the seed-42 system of n bodies."""
    big = nbx.initial_conditions(S * n, precision)
    states = [{f: big[f][m * n:(m + 1) * n].copy() for f in nbx.FIELDS} for m in range(S)]
    states[-1] = nbx.initial_conditions(n, precision)
    return states


def run_ensemble(nbx, n, S, steps, precision, states, **opts):
    with nbx.Ensemble(n, S, precision, **opts) as e:
        e.upload(states)
        st = e.stats()
        ke = e.step_trace(steps)
        out = e.download()
        assert e.stats()["steps_done"] == steps
    assert ke.shape == (steps, S) and all(out[f].shape == (S, n) for f in ARRAYS)
    assert st["n"] == n and st["members"] == S and st["grid_y"] == S and st["block"] == 256 and st["n_alloc"] == -(-n // 256) * 256
    assert st["grid_x"] == -(-(-(-n // st["bodies_per_lane"])) // 4)
    return st, ke, out


def run_context(nbx, n, steps, precision, state, NB, loop):
    with nbx.Context(n, precision, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
        c.upload(state)
        ke = c.step_trace(steps)
        out = c.download()
        st = c.stats()
    assert st["kernel_variant"] == nbx.KERNEL_JLANE and st["bodies_per_lane"] == NB and st["inner_loop"] == loop
    return st, ke, out


def assert_members_equal_single_contexts(nbx, n, S, steps, precision, **opts):
    states = member_states(nbx, n, S, precision)
    st, ke, out = run_ensemble(nbx, n, S, steps, precision, states, **opts)
    NB, loop = st["bodies_per_lane"], st["inner_loop"]
    assert loop in (nbx.LOOP_CXX, nbx.LOOP_ASM)
    for m in range(S):
        cst, cke, cout = run_context(nbx, n, steps, precision, states[m], NB, loop)
        assert cst["force_grid_x"] == st["grid_x"] and cst["force_grid_y"] == 1
        for f in ARRAYS:
            assert np.array_equal(out[f][m], cout[f]), (n, S, m, f, NB, loop)
        assert np.array_equal(ke[:, m], cke), (n, S, m, NB, loop, float(np.abs(ke[:, m] / cke - 1).max()))
    return st


F32_CASES = [(5, 3, 20), (65, 7, 20), (1000, 5, 100), (2000, 16, 60), (2048, 64, 20), (4099, 9, 40), (8192, 4, 10), (16383, 2, 4)]
F64_CASES = [(5, 3, 20), (2000, 8, 40), (4099, 3, 20), (12288, 2, 4)]


@pytest.mark.parametrize("n,S,steps", F32_CASES)
def test_every_member_is_bit_equal_to_a_single_context_fp32(nbx, n, S, steps):
    assert_members_equal_single_contexts(nbx, n, S, steps, 32)


@pytest.mark.parametrize("n,S,steps", F64_CASES)
def test_every_member_is_bit_equal_to_a_single_context_fp64(nbx, n, S, steps):
    assert_members_equal_single_contexts(nbx, n, S, steps, 64)


@pytest.mark.parametrize("precision,n,S,steps,NB", [(32, 2000, 16, 60, NB) for NB in (2, 4, 8, 16)] + [(64, 2000, 8, 40, NB) for NB in (2, 4, 8)])
def test_every_member_is_bit_equal_with_explicit_bodies_per_wave(nbx, precision, n, S, steps, NB):
    st = assert_members_equal_single_contexts(nbx, n, S, steps, precision, bodies_per_lane=NB)
    assert st["bodies_per_lane"] == NB


@pytest.mark.parametrize("NB", [2, 4, 8])
@pytest.mark.parametrize("loop", ["LOOP_CXX", "LOOP_ASM"])
def test_every_member_is_bit_equal_with_explicit_inner_loop(nbx, NB, loop):
    """Both loops of every fp32 shape that has two (the planner's own choice covers only one of them per shape)."""
    st = assert_members_equal_single_contexts(nbx, 2000, 5, 30, 32, bodies_per_lane=NB, inner_loop=getattr(nbx, loop))
    assert st["inner_loop"] == getattr(nbx, loop)


@pytest.mark.parametrize("precision,n,S,steps", [(32, 2000, 16, 60), (64, 2000, 8, 40)])
def test_step_returns_the_last_row_of_the_trace(nbx, precision, n, S, steps):
    states = member_states(nbx, n, S, precision)
    _, ke, out = run_ensemble(nbx, n, S, steps, precision, states)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        assert e.step(steps // 2, kenergy=False) is None  # asynchronous
        last = e.step(steps - steps // 2)
        again = e.step(0)                                  # nsteps == 0: the energies the last step left, as nbx_step
        fin = e.download()
    assert np.array_equal(last, ke[-1]) and np.array_equal(again, ke[-1])
    for f in ARRAYS:
        assert np.array_equal(fin[f], out[f]), f


@pytest.mark.parametrize("precision,n,S,steps", [(32, 2000, 16, 60), (32, 65, 7, 20), (64, 2000, 8, 40)])
def test_a_member_does_not_depend_on_its_neighbours_or_on_how_it_was_uploaded(nbx, precision, n, S, steps):
    """The same systems in reversed member order, uploaded in two calls (the upper half first, one of them as a dict of 2-D
    arrays): system k then sits at member S - 1 - k, and its trajectory is the same bits."""
    states = member_states(nbx, n, S, precision)
    _, ke, out = run_ensemble(nbx, n, S, steps, precision, states)
    rev = states[::-1]
    h = S // 2
    with nbx.Ensemble(n, S, precision) as e:
        e.upload({f: np.stack([s[f] for s in rev[h:]]) for f in nbx.FIELDS}, first=h)
        with pytest.raises(nbx.NbxError) as err:
            e.step(1)
        assert err.value.code == nbx.NBX_ERR_STATE
        e.upload(rev[:h])
        ke2 = e.step_trace(steps)
        part = e.download(first=1, count=2)
        out2 = e.download()
    assert np.array_equal(ke2, ke[:, ::-1])
    for f in ARRAYS:
        assert np.array_equal(out2[f], out[f][::-1]), f
        assert np.array_equal(part[f], out2[f][1:3]), f


def _last_member_trace(nbx, n, steps, precision, S=6):
    states = member_states(nbx, n, S, precision)
    _, ke, _ = run_ensemble(nbx, n, S, steps, precision, states)
    return ke[:, -1]


@pytest.mark.parametrize("n,steps", [(2000, 500), (1000, 100), (4099, 40), (65, 20), (5, 20)])
def test_last_member_against_the_reference_fp32(nbx, n, steps):
    """The gate of test_jlane_sizes_against_the_reference_binary: relative kinetic-energy error < 1e-4 at every printed row
    (steps that are multiples of 50; runs shorter than 50 steps: the last step)."""
    g = load_golden("ver7_f32_n%d_s%d.json" % (n, steps))
    assert g["n"] == n and g["nsteps"] == steps
    e = rel_err(_last_member_trace(nbx, n, steps, 32), g["kenergy"])
    rows = list(range(50, steps + 1, 50)) or [steps]
    print("ensemble last member vs reference fp32 n=%d: " % n + ", ".join("step %d: %.3e" % (k, e[k - 1]) for k in rows))
    for k in rows:
        assert e[k - 1] < 1e-4, (k, e[k - 1])


@pytest.mark.parametrize("n,steps", [(2000, 500), (4099, 40), (5, 20)])
def test_last_member_against_the_reference_fp64(nbx, n, steps):
    """The bound of test_jlane_fp64_traces_against_the_reference_fp64_build: < 1e-10 at every step."""
    g = load_golden("ver7_f64_n%d_s%d.json" % (n, steps))
    assert g["n"] == n and g["nsteps"] == steps and g["precision"] == 64
    e = rel_err(_last_member_trace(nbx, n, steps, 64), g["kenergy"])
    print("ensemble last member vs reference fp64 n=%d: max %.3e" % (n, e.max()))
    assert e.max() < 1e-10, e.max()


def test_state_and_range_errors(nbx):
    n, S = 300, 4
    states = member_states(nbx, n, S, 32)
    with nbx.Ensemble(n, S, 32) as e:
        with pytest.raises(nbx.NbxError) as err:
            e.step(1)
        assert err.value.code == nbx.NBX_ERR_STATE
        e.upload(states[:3])
        for call in (lambda: e.step(1), lambda: e.step_trace(2), lambda: e.download()):
            with pytest.raises(nbx.NbxError) as err:
                call()
            assert err.value.code == nbx.NBX_ERR_STATE, str(err.value)
        assert all(e.download(first=0, count=3)[f].shape == (3, n) for f in ARRAYS)
        for first, states_ in ((3, states[:2]), (4, states[:1]), (-1, states[:1])):
            with pytest.raises(nbx.NbxError) as err:
                e.upload(states_, first=first)
            assert err.value.code == nbx.NBX_ERR_ARG
        with pytest.raises(nbx.NbxError) as err:
            e.download(first=2, count=3)
        assert err.value.code == nbx.NBX_ERR_ARG
        e.upload(states[3:], first=3)
        with pytest.raises(nbx.NbxError) as err:
            e.step(-1)
        assert err.value.code == nbx.NBX_ERR_ARG
        assert np.array_equal(e.step(0), np.zeros(S))  # no step yet: zeros, as nbx_step
        ke = e.step(3)
        assert ke.shape == (S,) and (ke > 0).all()


def test_profile_times_one_launch_per_step(nbx):
    n, S = 2048, 8
    with nbx.Ensemble(n, S, 32) as e:
        e.upload(member_states(nbx, n, S, 32))
        e.profile(True)
        e.step(25, kenergy=False)
        e.step(5)
        st = e.stats()
        e.profile(False)
    assert st["launches_timed"] == 30 and st["steps_done"] == 30 and st["step_ms_total"] > 0.0
    assert st["cu_count"] > 0


def test_an_ensemble_and_a_context_do_not_disturb_each_other(nbx):
    n, S, steps, m = 2000, 12, 40, 1500
    ic = nbx.initial_conditions(m)
    with nbx.Context(m, 32) as c:
        c.upload(ic)
        alone_ke = c.step_trace(steps)
        alone = c.download()
    states = member_states(nbx, n, S, 32)
    _, ke, out = run_ensemble(nbx, n, S, steps, 32, states)
    with nbx.Ensemble(n, S, 32) as e, nbx.Context(m, 32) as c:
        e.upload(states)
        c.upload(ic)
        ke2, cke = [], []
        for _ in range(steps // 4):  # interleaved: asynchronous steps of both in flight at once
            e.step(3, kenergy=False)
            c.step(3, kenergy=False)
            ke2.append(e.step(1))
            cke.append(c.step(1))
        both, cboth = e.download(), c.download()
    assert np.array_equal(np.array(ke2), ke[3::4]) and np.array_equal(np.array(cke), alone_ke[3::4])
    for f in ARRAYS:
        assert np.array_equal(both[f], out[f]) and np.array_equal(cboth[f], alone[f]), f
