"""Ragged ensembles on the device (include/nbx_ragged.h): every member of a launch over members of different size must come out
bit for bit as a single nbx_ctx of the same shape does -- positions, velocities and the kinetic energy of every step --
whatever its neighbours are and wherever the work list puts its workgroups; a launch over equal members must be an
nbx_ensemble; the reference's own seed-42 system, placed as the LAST member, must meet the reference's fixtures within the
project's existing gates for the one-launch kernel; and one ragged step must cost no more than stepping the members as
contexts."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu

ARRAYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z")


def member_states(nbx, sizes, precision):
    """As member_states of test_ensemble_gpu.py: member k = the next sizes[k] bodies of the seed-42 system of sum(sizes) bodies; the
    last member is the seed-42 system of its own size."""
    big = nbx.initial_conditions(sum(sizes), precision)
    at = np.concatenate([[0], np.cumsum(sizes)])
    states = [{f: big[f][at[k]:at[k + 1]].copy() for f in nbx.FIELDS} for k in range(len(sizes))]
    states[-1] = nbx.initial_conditions(sizes[-1], precision)
    return states


def run_ragged(nbx, sizes, steps, precision, states, **opts):
    with nbx.Ragged(sizes, precision, **opts) as r:
        r.upload(states)
        st = r.stats()
        ke = r.step_trace(steps)
        out = r.download()
        assert r.stats()["steps_done"] == steps
    assert ke.shape == (steps, len(sizes)) and [o[f].shape for o in out for f in ARRAYS] == [(n,) for n in sizes for _ in ARRAYS]
    NB = st["bodies_per_lane"]
    assert st["members"] == len(sizes) and st["block"] == 256 and st["n_min"] == min(sizes) and st["n_max"] == max(sizes)
    assert st["bodies_total"] == sum(sizes) and st["pairs_per_step"] == float(sum(n * n for n in sizes))
    assert st["grid_x"] == sum(-(-(-(-n // NB)) // 4) for n in sizes)
    assert st["inner_loop"] in (nbx.LOOP_CXX, nbx.LOOP_ASM)
    return st, ke, out


def run_context(nbx, n, steps, precision, state, NB, loop):
    with nbx.Context(n, precision, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
        c.upload(state)
        ke = c.step_trace(steps)
        out = c.download()
        st = c.stats()
    assert st["kernel_variant"] == nbx.KERNEL_JLANE and st["bodies_per_lane"] == NB and st["inner_loop"] == loop
    assert st["force_grid_x"] == -(-(-(-n // NB)) // 4) and st["force_grid_y"] == 1
    return ke, out


def assert_members_equal_single_contexts(nbx, sizes, steps, precision, **opts):
    states = member_states(nbx, sizes, precision)
    st, ke, out = run_ragged(nbx, sizes, steps, precision, states, **opts)
    NB, loop = st["bodies_per_lane"], st["inner_loop"]
    for m, n in enumerate(sizes):
        cke, cout = run_context(nbx, n, steps, precision, states[m], NB, loop)
        for f in ARRAYS:
            assert np.array_equal(out[m][f], cout[f]), (sizes, m, f, NB, loop)
        assert np.array_equal(ke[:, m], cke), (sizes, m, NB, loop, float(np.abs(ke[:, m] / cke - 1).max()))
    return st


# the smallest shapes that reach every branch of the body: a member smaller than a wave, K = 4 with zero trips of the generated
# loop, ragged last waves; trip remainders 0 and 4; the largest members the kernel takes
F32_POPULATIONS = [((5, 65, 1000, 256, 257, 2000, 63), 20), ((512, 700, 2048, 300), 20), ((16383, 5, 8192), 4)]
F64_POPULATIONS = [((5, 2000, 300, 4099), 20), ((12288, 7), 4)]
MIXED = (5, 65, 1000, 257, 2000)


@pytest.mark.parametrize("sizes,steps", F32_POPULATIONS)
def test_every_member_is_bit_equal_to_a_single_context_fp32(nbx, sizes, steps):
    assert_members_equal_single_contexts(nbx, sizes, steps, 32)


@pytest.mark.parametrize("sizes,steps", F64_POPULATIONS)
def test_every_member_is_bit_equal_to_a_single_context_fp64(nbx, sizes, steps):
    assert_members_equal_single_contexts(nbx, sizes, steps, 64)


@pytest.mark.parametrize("precision,NB", [(32, NB) for NB in (2, 4, 8, 16)] + [(64, NB) for NB in (2, 4, 8)])
def test_every_member_is_bit_equal_with_explicit_bodies_per_wave(nbx, precision, NB):
    st = assert_members_equal_single_contexts(nbx, MIXED, 20, precision, bodies_per_lane=NB)
    assert st["bodies_per_lane"] == NB


@pytest.mark.parametrize("NB", [2, 4, 8])
@pytest.mark.parametrize("loop", ["LOOP_CXX", "LOOP_ASM"])
def test_every_member_is_bit_equal_with_explicit_inner_loop(nbx, NB, loop):
    """Both loops of every fp32 shape that has two (the planner's own choice covers only one of them per shape)."""
    st = assert_members_equal_single_contexts(nbx, MIXED, 20, 32, bodies_per_lane=NB, inner_loop=getattr(nbx, loop))
    assert st["inner_loop"] == getattr(nbx, loop)


@pytest.mark.parametrize("precision", [32, 64])
def test_equal_members_are_an_ensemble(nbx, precision):
    """Ragged([2000] * 8) against Ensemble(2000, 8): the planner's choice, the arrays and the whole energy trace."""
    n, S, steps = 2000, 8, 40
    states = member_states(nbx, [n] * S, precision)
    st, ke, out = run_ragged(nbx, [n] * S, steps, precision, states)
    with nbx.Ensemble(n, S, precision) as e:
        e.upload(states)
        est = e.stats()
        eke = e.step_trace(steps)
        eout = e.download()
    assert (st["bodies_per_lane"], st["inner_loop"]) == (est["bodies_per_lane"], est["inner_loop"])
    assert st["grid_x"] == est["grid_x"] * est["grid_y"]
    assert np.array_equal(ke, eke)
    for f in ARRAYS:
        assert np.array_equal(np.stack([o[f] for o in out]), eout[f]), f


@pytest.mark.parametrize("precision,sizes,steps", [(32, (5, 65, 1000, 256, 257, 2000, 63), 20), (64, (5, 2000, 300, 4099), 20)])
def test_a_member_does_not_depend_on_its_neighbours_or_on_how_it_was_uploaded(nbx, precision, sizes, steps):
    """The same systems in reversed member order, uploaded in two calls (the upper half first): system k then sits at member
    S - 1 - k -- behind other neighbours, at other offsets and at another place of the work list -- and its trajectory is the same bits."""
    S = len(sizes)
    states = member_states(nbx, sizes, precision)
    st, ke, out = run_ragged(nbx, sizes, steps, precision, states)
    rev, rsizes = states[::-1], sizes[::-1]
    h = S // 2
    with nbx.Ragged(rsizes, precision) as r:
        r.upload(rev[h:], first=h)
        with pytest.raises(nbx.NbxError) as err:
            r.step(1)
        assert err.value.code == nbx.NBX_ERR_STATE
        r.upload(rev[:h])
        st2 = r.stats()
        ke2 = r.step_trace(steps)
        part = r.download(first=1, count=2)
        out2 = r.download()
    assert (st2["bodies_per_lane"], st2["inner_loop"], st2["grid_x"]) == (st["bodies_per_lane"], st["inner_loop"], st["grid_x"])
    assert np.array_equal(ke2, ke[:, ::-1])
    for k in range(S):
        for f in ARRAYS:
            assert np.array_equal(out2[S - 1 - k][f], out[k][f]), (k, f)
    assert len(part) == 2
    for f in ARRAYS:
        assert np.array_equal(part[0][f], out2[1][f]) and np.array_equal(part[1][f], out2[2][f]), f


@pytest.mark.parametrize("precision,sizes,steps", [(32, (5, 65, 1000, 256, 257, 2000, 63), 20), (64, (5, 2000, 300, 4099), 20)])
def test_step_returns_the_last_row_of_the_trace(nbx, precision, sizes, steps):
    states = member_states(nbx, sizes, precision)
    _, ke, out = run_ragged(nbx, sizes, steps, precision, states)
    with nbx.Ragged(sizes, precision) as r:
        r.upload(states)
        assert np.array_equal(r.step(0), np.zeros(len(sizes)))  # no step yet: zeros, as nbx_step
        assert r.step(steps // 2, kenergy=False) is None         # asynchronous
        last = r.step(steps - steps // 2)
        again = r.step(0)                                        # nsteps == 0: the energies the last step left
        fin = r.download()
    assert np.array_equal(last, ke[-1]) and np.array_equal(again, ke[-1])
    for m in range(len(sizes)):
        for f in ARRAYS:
            assert np.array_equal(fin[m][f], out[m][f]), (m, f)


def test_a_member_uploaded_again_starts_over(nbx):
    sizes, steps = (300, 1000, 65), 10
    states = member_states(nbx, sizes, 32)
    _, ke, out = run_ragged(nbx, sizes, steps, 32, states)
    with nbx.Ragged(sizes, 32) as r:
        r.upload(states)
        r.step(7, kenergy=False)
        r.upload(states)
        ke2 = r.step_trace(steps)
        out2 = r.download()
    assert np.array_equal(ke2, ke)
    assert all(np.array_equal(out2[m][f], out[m][f]) for m in range(len(sizes)) for f in ARRAYS)


REFERENCE_POPULATION = (65, 4099, 1000, 2000)  # the seed-42 system of 2000 bodies last, behind members of other sizes


def _last_member_trace(nbx, precision):
    states = member_states(nbx, REFERENCE_POPULATION, precision)
    _, ke, _ = run_ragged(nbx, REFERENCE_POPULATION, 500, precision, states)
    return ke[:, -1]


def test_last_member_against_the_reference_fp32(nbx):
    """The gate of test_jlane_sizes_against_the_reference_binary: relative kinetic-energy error < 1e-4 at every printed row
    (steps that are multiples of 50)."""
    g = load_golden("ver7_f32_n2000_s500.json")
    assert g["n"] == 2000 and g["nsteps"] == 500
    e = rel_err(_last_member_trace(nbx, 32), g["kenergy"])
    rows = list(range(50, 501, 50))
    print("ragged last member vs reference fp32 n=2000: " + ", ".join("step %d: %.3e" % (k, e[k - 1]) for k in rows))
    for k in rows:
        assert e[k - 1] < 1e-4, (k, e[k - 1])


def test_last_member_against_the_reference_fp64(nbx):
    """The bound of test_jlane_fp64_traces_against_the_reference_fp64_build: < 1e-10 at every step."""
    g = load_golden("ver7_f64_n2000_s500.json")
    assert g["n"] == 2000 and g["nsteps"] == 500 and g["precision"] == 64
    e = rel_err(_last_member_trace(nbx, 64), g["kenergy"])
    print("ragged last member vs reference fp64 n=2000: max %.3e, at the multiples of 50: %s" % (e.max(), ", ".join("%.2e" % e[k - 1] for k in range(50, 501, 50))))
    assert e.max() < 1e-10, e.max()


def test_state_and_range_errors(nbx):
    sizes = (300, 5, 1000, 64)
    states = member_states(nbx, sizes, 32)
    with nbx.Ragged(sizes, 32) as r:
        r.upload(states[:3])
        for call in (lambda: r.step(1), lambda: r.step_trace(2), lambda: r.download()):
            with pytest.raises(nbx.NbxError) as err:
                call()
            assert err.value.code == nbx.NBX_ERR_STATE, str(err.value)
        assert [o["pos_x"].shape for o in r.download(first=0, count=3)] == [(300,), (5,), (1000,)]
        for first, states_ in ((3, states[:2]), (4, states[:1]), (-1, states[:1])):
            with pytest.raises(nbx.NbxError) as err:
                r.upload(states_, first=first)
            assert err.value.code == nbx.NBX_ERR_ARG
        with pytest.raises(nbx.NbxError) as err:
            r.upload(states[:1], first=1)  # a state of 300 bodies for a member of 5
        assert err.value.code == nbx.NBX_ERR_ARG
        with pytest.raises(nbx.NbxError) as err:
            r.download(first=2, count=3)
        assert err.value.code == nbx.NBX_ERR_ARG
        r.upload(states[3:], first=3)
        with pytest.raises(nbx.NbxError) as err:
            r.step(-1)
        assert err.value.code == nbx.NBX_ERR_ARG
        ke = r.step(3)
        assert ke.shape == (4,) and (ke > 0).all()


def test_profile_times_one_launch_per_step(nbx):
    sizes = (2048, 300, 1000, 700)
    with nbx.Ragged(sizes, 32) as r:
        r.upload(member_states(nbx, sizes, 32))
        r.profile(True)
        r.step(25, kenergy=False)
        r.step(5)
        st = r.stats()
        r.profile(False)
    assert st["launches_timed"] == 30 and st["steps_done"] == 30 and st["step_ms_total"] > 0.0 and st["cu_count"] > 0


def test_one_ragged_step_costs_no_more_than_the_members_as_contexts(nbx):
    """Uniform 64 x 2048 fp32, the method of the ensemble sweep (scripts/ragged_sweep.py: warm-up, legs alternated, medians, one
    process): one ragged step of all members against the 64 contexts on their own streams with graph replay, taken the way that
    is better for them.  The uniform ensemble measured 1.72 x at this shape (profiles/ensemble_sweep.json), so a bound of 1.0
    leaves the descriptor fetch ample room, and a planner or work-list mistake that serialises members trips it."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import ragged_sweep
    g = ragged_sweep.measure_gate(nbx)
    print("64 x 2048 fp32: ragged %.1f us per step, 64 contexts %.1f (one after the other) / %.1f (round-robin), ratio %.3f" % (
        g["ragged_us"], g["contexts_sequential_us"], g["contexts_round_robin_us"], g["ratio_ragged_over_contexts"]))
    ragged_sweep.write(ragged_sweep.OUT, gate=g)
    assert g["ratio_ragged_over_contexts"] <= 1.0, g
