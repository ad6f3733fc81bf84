"""The host paths of the context (csrc/nbx_api.hip) that the parity modules do not reach: the growth of the energy-trace
buffer and the splitting of a run over several calls (through plain launches, graph replay and the separate integrate kernel),
the partials a re-upload drops, the profiling counters across enable / disable, a raw C-ABI download of a slice through a single
array, and a context on a stream the caller lent it.  Every comparison is bit for bit, against the same library doing the same
work another way."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z")
# the one-launch kernel (energy partials from the step kernel itself), and the wave-split kernel with four j splits (partials
# from the separate integrate kernel)
KERNEL_SGPRW = 3  # nbx.KERNEL_SGPRW
SHAPES = {"one-launch": (257, {}), "slab": (2304, dict(kernel_variant=KERNEL_SGPRW, j_split=4))}
CASES = [(shape, precision) for shape in SHAPES for precision in (32, 64)]


def assert_same_download(a, b):
    for f in ARRAYS:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("shape,precision", CASES)
def test_trace_buffer_growth_and_a_run_split_over_calls(nbx, shape, precision):
    """step_trace(2), step_trace(70), step(8), step(3), step(0) on one context against one step_trace(83) on another: the trace
    buffer (64 slots at create) grows for the second call, step(8) replays a captured graph and reduces into slot 0, step(3)
    launches plainly, and step(0) reduces the partials again."""
    n, opts = SHAPES[shape]
    assert KERNEL_SGPRW == nbx.KERNEL_SGPRW
    state = nbx.initial_conditions(n, precision)
    with nbx.Context(n, precision, **opts) as a, nbx.Context(n, precision, **opts) as b:
        a.upload(state)
        b.upload(state)
        t2, t70, k8, k3, again = a.step_trace(2), a.step_trace(70), a.step(8), a.step(3), a.step(0)
        ref = b.step_trace(83)
        assert ref.shape == (83,) and (ref > 0).all()
        assert t2.shape == (2,) and t70.shape == (70,)
        assert np.array_equal(np.concatenate([t2, t70]), ref[:72])
        assert k8 == ref[79] and k3 == ref[82] and again == ref[82]
        sa, sb = a.stats(), b.stats()
        assert sa["graph_replays"] > 0 and sb["graph_replays"] == 0
        assert sa["steps_done"] == 83 and sb["steps_done"] == 83
        assert sa["fused_epilogue"] == (0 if shape == "slab" else 1) and sa["j_split"] == (4 if shape == "slab" else 1)
        assert_same_download(a.download(), b.download())


@pytest.mark.parametrize("shape,precision", CASES)
def test_an_upload_drops_the_partials_of_the_previous_trajectory(nbx, shape, precision):
    n, opts = SHAPES[shape]
    state = nbx.initial_conditions(n, precision)
    with nbx.Context(n, precision, **opts) as a, nbx.Context(n, precision, **opts) as fresh:
        a.upload(state)
        assert a.step(4) > 0
        a.upload(state)
        assert a.step(0) == 0.0 and a.kenergy_partial() == 0.0
        ke = a.step(1)
        fresh.upload(state)
        assert fresh.step(1) == ke and ke > 0
        assert a.step(0) == ke
        assert_same_download(a.download(), fresh.download())


@pytest.mark.parametrize("precision", (32, 64))
def test_profiling_counts_across_stats_disable_and_enable(nbx, precision):
    with nbx.Context(257, precision) as c:
        c.upload(nbx.initial_conditions(257, precision))
        c.profile(True)
        c.step(5, kenergy=False)
        assert c.stats()["force_launches_timed"] == 5  # stats drains the pending events
        c.step(5)
        c.profile(False)
        st = c.stats()
        assert st["force_launches_timed"] == 10 and st["force_ms_total"] > 0.0 and st["steps_done"] == 10
        assert st["graph_replays"] == 0  # a profiled step is launched plainly
        c.profile(True)
        st = c.stats()
        assert st["force_launches_timed"] == 0 and st["force_ms_total"] == 0.0


@pytest.mark.parametrize("precision", (32, 64))
def test_the_validation_kernel_is_not_timed(nbx, precision):
    with nbx.Context(257, precision, kernel_variant=nbx.KERNEL_EXACT) as c:
        c.upload(nbx.initial_conditions(257, precision))
        c.profile(True)
        assert c.step(5) > 0
        st = c.stats()
        assert st["force_launches_timed"] == 0 and st["force_ms_total"] == 0.0 and st["steps_done"] == 5
        c.profile(False)
        assert c.stats()["force_launches_timed"] == 0


@pytest.mark.parametrize("precision", (32, 64))
def test_raw_download_of_a_slice_through_one_array_at_a_time(nbx, precision):
    """A context that owns bodies [256, 300) of 300, with exactly one of the six arrays non-NULL: a position array receives all
    300 elements, a velocity array those of the owned bodies only; everything else keeps its marker."""
    n, i_begin, i_count, guard = 300, 256, 44, 8
    L = nbx.load()
    with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count) as c:
        c.upload(nbx.initial_conditions(n, precision))
        c.step_local()
        c.commit()
        full = c.download()
        for i, f in enumerate(ARRAYS):
            buf = np.full(n + guard, -7.0, dtype=c.dtype)
            ptrs = [None] * 6
            ptrs[i] = buf.ctypes.data_as(ctypes.c_void_p)
            rc = L.nbx_download(c._h, *ptrs)
            assert rc == nbx.NBX_OK, L.nbx_last_error()
            lo, hi = (0, n) if f.startswith("pos") else (i_begin, i_begin + i_count)
            assert np.array_equal(buf[lo:hi], full[f][lo:hi]) and (buf[lo:hi] != -7.0).all(), f
            assert (buf[:lo] == -7.0).all() and (buf[hi:] == -7.0).all(), f


def test_a_context_on_the_default_stream_the_caller_lent_it(nbx):
    """external_stream = 1 with stream = NULL is the caller's default stream: the context works on it, its destroy synchronises
    it and leaves it alone, and a second such context in the same process gives what a context with its own stream gives."""
    n = 257
    state = nbx.initial_conditions(n, 32)
    with nbx.Context(n, 32, external_stream=1, stream=None) as first:
        first.upload(state)
        ke_first = first.step(4)
        assert first.stats()["use_graph"] == 0  # a lent stream is not captured
    with nbx.Context(n, 32, external_stream=1, stream=None) as lent, nbx.Context(n, 32) as own:
        lent.upload(state)
        own.upload(state)
        ke_lent, ke_own = lent.step(4), own.step(4)
        assert ke_lent == ke_own and ke_lent == ke_first and ke_own > 0
        assert lent.stats()["graph_replays"] == 0 and own.stats()["graph_replays"] > 0
        lent.sync()
        assert_same_download(lent.download(), own.download())
