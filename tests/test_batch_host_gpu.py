"""The host paths both batch objects share (csrc/nbx_batch.hpp) that the modules of each kind do not reach: a raw C-ABI
download through a single array, the growth of the energy-trace buffer and the splitting of a run over several calls, the
partials a re-upload drops, and the profiling counters across enable / disable.  Every comparison is bit for bit, against the
same library doing the same work another way.

The smallest objects that have more than one member, members smaller and larger than a workgroup, and (ragged) padding
between members: an ensemble of 3 members of 65 bodies and a ragged ensemble of sizes (5, 65, 257)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z")
KINDS = {"ensemble": (65, 65, 65), "ragged": (5, 65, 257)}
CASES = [(kind, precision) for kind in KINDS for precision in (32, 64)]


def make(nbx, kind, precision):
    return nbx.Ensemble(65, 3, precision) if kind == "ensemble" else nbx.Ragged(KINDS[kind], precision)


def member_states(nbx, kind, precision):
    """member k = the next sizes[k] bodies of the seed-42 system of sum(sizes) bodies"""
    sizes = KINDS[kind]
    big = nbx.initial_conditions(sum(sizes), precision)
    at = np.concatenate([[0], np.cumsum(sizes)])
    return [{f: big[f][at[k]:at[k + 1]].copy() for f in nbx.FIELDS} for k in range(len(sizes))]


def members(kind, out):
    """a download of either kind as a list of dicts, one per member"""
    if kind == "ragged":
        return out
    return [{f: out[f][k] for f in ARRAYS} for k in range(out[ARRAYS[0]].shape[0])]


def assert_same_download(kind, a, b):
    a, b = members(kind, a), members(kind, b)
    assert len(a) == len(b)
    for k in range(len(a)):
        for f in ARRAYS:
            assert np.array_equal(a[k][f], b[k][f]), (k, f)


@pytest.mark.parametrize("kind,precision", CASES)
def test_raw_download_through_one_array_at_a_time(nbx, kind, precision):
    """Members [1, 3) with exactly one of the six arrays non-NULL: each equals the matching array of a full download, and the
    call writes exactly the elements of those members (the elements behind them keep their marker)."""
    sizes = KINDS[kind]
    L = nbx.load()
    fn = L.nbx_ensemble_download if kind == "ensemble" else L.nbx_ragged_download
    total, guard = sizes[1] + sizes[2], 8
    with make(nbx, kind, precision) as o:
        o.upload(member_states(nbx, kind, precision))
        o.step(3, kenergy=False)
        full = members(kind, o.download())
        for i, f in enumerate(ARRAYS):
            buf = np.full(total + guard, -7.0, dtype=o.dtype)
            ptrs = [None] * 6
            ptrs[i] = buf.ctypes.data_as(ctypes.c_void_p)
            rc = fn(o._h, 1, 2, *ptrs)
            assert rc == nbx.NBX_OK, L.nbx_last_error()
            assert np.array_equal(buf[:total], np.concatenate([full[1][f], full[2][f]])), f
            assert (buf[total:] == -7.0).all(), f


@pytest.mark.parametrize("kind,precision", CASES)
def test_trace_buffer_growth_and_a_run_split_over_calls(nbx, kind, precision):
    """step_trace(2), step_trace(40), step(3), step(0) on one object against one step_trace(45) on another: the trace buffer
    grows between the first two calls, step() reduces into slot 0 of it, and step(0) reduces the partials again."""
    states = member_states(nbx, kind, precision)
    with make(nbx, kind, precision) as a, make(nbx, kind, precision) as b:
        a.upload(states)
        b.upload(states)
        t2, t40, last, again = a.step_trace(2), a.step_trace(40), a.step(3), a.step(0)
        ref = b.step_trace(45)
        assert ref.shape == (45, 3) and (ref > 0).all()
        assert t2.shape == (2, 3) and t40.shape == (40, 3)
        assert np.array_equal(np.concatenate([t2, t40]), ref[:42])
        assert np.array_equal(last, ref[44]) and np.array_equal(again, ref[44])
        assert a.stats()["steps_done"] == 45 and b.stats()["steps_done"] == 45
        assert_same_download(kind, a.download(), b.download())


@pytest.mark.parametrize("kind,precision", CASES)
def test_an_upload_drops_the_partials_of_the_previous_trajectories(nbx, kind, precision):
    states = member_states(nbx, kind, precision)
    with make(nbx, kind, precision) as a, make(nbx, kind, precision) as fresh:
        a.upload(states)
        assert (a.step(4) > 0).all()
        now = members(kind, a.download())
        a.upload([states[1]], first=1)
        assert np.array_equal(a.step(0), np.zeros(3))  # all members: the flag belongs to the object
        ke = a.step(1)
        # a fresh object brought to the same state: members 0 and 2 as they were after four steps, member 1 as uploaded
        same = [dict(now[k], mass=states[k]["mass"]) for k in range(3)]
        same[1] = states[1]
        fresh.upload(same)
        assert np.array_equal(fresh.step(1), ke) and (ke > 0).all()
        assert_same_download(kind, a.download(), fresh.download())


@pytest.mark.parametrize("kind,precision", CASES)
def test_profiling_counts_across_stats_disable_and_enable(nbx, kind, precision):
    with make(nbx, kind, precision) as o:
        o.upload(member_states(nbx, kind, precision))
        o.profile(True)
        o.step(5, kenergy=False)
        assert o.stats()["launches_timed"] == 5  # stats drains the pending events
        o.step(5)
        o.profile(False)
        st = o.stats()
        assert st["launches_timed"] == 10 and st["step_ms_total"] > 0.0 and st["steps_done"] == 10
        o.profile(True)
        st = o.stats()
        assert st["launches_timed"] == 0 and st["step_ms_total"] == 0.0
