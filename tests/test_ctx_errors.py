"""The argument and state errors of the context (include/nbx.h, nbx_diag.h; csrc/nbx_api.hip, nbx_diag.hip) as the exact text
nbx_last_error() gives for each, with its return code, through raw C-ABI calls.  The texts are literal: they are part of what a
caller sees, and the host layer under the context may be reorganised only if every one of them comes out byte for byte.

The first part needs no GPU (every case returns before the first HIP call); the second creates the smallest contexts, 65
bodies in fp32, and launches a few steps at most."""
import ctypes

import pytest

N = 65


def _call(nbx, name, *args):
    """(return code, nbx_last_error() text) of one raw C-ABI call"""
    L = nbx.load()
    rc = getattr(L, name)(*args)
    return rc, L.nbx_last_error().decode()


def _opts(nbx, **kw):
    o = nbx.Opts()
    o.struct_size = ctypes.sizeof(nbx.Opts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _create(nbx, n, precision, **kw):
    """nbx_create with a handle that is set beforehand: (rc, text, handle value afterwards)"""
    h = ctypes.c_void_p(1)
    o = _opts(nbx, **kw)
    rc, text = _call(nbx, "nbx_create", ctypes.byref(h), n, precision, ctypes.byref(o))
    return rc, text, h.value


# ---------------------------------------------------------------------------------------------------------------------------
# no GPU: everything here is refused before the first HIP call
# ---------------------------------------------------------------------------------------------------------------------------
def test_null_handle_texts(nbx):
    null = ctypes.c_void_p()
    d = ctypes.c_double()
    trace = (ctypes.c_double * 4)()
    cases = [
        ("nbx_upload", (null,) * 8, "nbx_upload"), ("nbx_step", (null, 0.1, 1, None), "nbx_step"),
        ("nbx_step", (null, 0.1, 1, ctypes.byref(d)), "nbx_step"), ("nbx_step_local", (null, 0.1), "nbx_step_local"),
        ("nbx_commit", (null,), "nbx_commit"), ("nbx_accel", (null,) * 4, "nbx_accel"), ("nbx_sync", (null,), "nbx_sync"),
        ("nbx_download", (null,) * 7, "nbx_download"), ("nbx_profile", (null, 0), "nbx_profile"), ("nbx_profile", (null, 1), "nbx_profile"),
        # a trace request shares nbx_step's checks and names them so
        ("nbx_step_trace", (null, 0.1, 1, trace), "nbx_step"),
    ]
    for fn, args, where in cases:
        rc, text = _call(nbx, fn, *args)
        assert rc == nbx.NBX_ERR_ARG, (fn, rc, text)
        assert text == where + ": ctx is NULL", (fn, text)


def test_null_argument_texts(nbx):
    null = ctypes.c_void_p()
    p, d, st, dg = ctypes.c_void_p(), ctypes.c_double(), nbx.Stats(), nbx.Diag()
    cases = [
        ("nbx_exchange_buffer", (null, ctypes.byref(p), None, None, None)), ("nbx_exchange_buffer", (null, None, None, None, None)),
        ("nbx_kenergy_partial", (null, ctypes.byref(d))), ("nbx_kenergy_partial", (null, None)),
        ("nbx_stats", (null, ctypes.byref(st))), ("nbx_stats", (null, None)),
        ("nbx_diagnostics", (null, ctypes.byref(dg))), ("nbx_diagnostics", (null, None)),
    ]
    for fn, args in cases:
        rc, text = _call(nbx, fn, *args)
        assert rc == nbx.NBX_ERR_ARG and text == fn + ": NULL argument", (fn, rc, text)


def test_null_ke_trace_is_reported_before_the_handle_is_looked_at(nbx):
    rc, text = _call(nbx, "nbx_step_trace", ctypes.c_void_p(), 0.1, 1, None)
    assert rc == nbx.NBX_ERR_ARG and text == "nbx_step_trace: ke_trace is NULL", text


def test_create_argument_texts(nbx):
    rc, text = _call(nbx, "nbx_create", None, N, 32, None)
    assert rc == nbx.NBX_ERR_ARG and text == "nbx_create: out is NULL", text
    rc, text = _call(nbx, "nbx_create", None, 0, 7, None)  # before anything else is looked at
    assert rc == nbx.NBX_ERR_ARG and text == "nbx_create: out is NULL", text
    slice_text = "nbx_create: slice [i_begin, i_begin+i_count) is outside [0, n)"
    cases = [
        ((0, 32, {}), "nbx_create: n must be > 0"), ((-3, 32, {}), "nbx_create: n must be > 0"),
        ((N, 16, {}), "nbx_create: precision must be 32 or 64"), ((N, 0, {}), "nbx_create: precision must be 32 or 64"),
        ((N, 32, dict(struct_size=ctypes.sizeof(nbx.Opts) + 4)), "nbx_create: nbx_opts.struct_size does not match this library"),
        ((N, 32, dict(i_begin=-1)), slice_text), ((N, 32, dict(i_count=-1)), slice_text), ((N, 32, dict(i_begin=N)), slice_text),
        ((N, 32, dict(i_begin=1, i_count=N)), slice_text), ((N, 32, dict(i_begin=2**31 - 1, i_count=2**31 - 1)), slice_text),
        ((N, 32, dict(n_alloc=N - 1)), "nbx_create: n_alloc < n"),
    ]
    for (n, precision, kw), want in cases:
        rc, text, h = _create(nbx, n, precision, **kw)
        assert rc == nbx.NBX_ERR_ARG and text == want, (n, precision, kw, rc, text)
        assert not h, (kw, h)  # *out is cleared before anything else is looked at


def test_create_errors_are_reported_in_a_fixed_order(nbx):
    """n, precision, nbx_opts.struct_size, the slice, n_alloc: the first of them that is wrong is the one reported."""
    foreign = ctypes.sizeof(nbx.Opts) + 4
    cases = [
        ((0, 32, dict(struct_size=foreign)), "nbx_create: n must be > 0"),
        ((N, 16, dict(i_begin=N)), "nbx_create: precision must be 32 or 64"),
        ((0, 16, {}), "nbx_create: n must be > 0"),
        ((N, 16, dict(struct_size=foreign)), "nbx_create: precision must be 32 or 64"),
        ((N, 32, dict(struct_size=foreign, i_begin=N, n_alloc=1)), "nbx_create: nbx_opts.struct_size does not match this library"),
        ((N, 32, dict(i_begin=N, n_alloc=1)), "nbx_create: slice [i_begin, i_begin+i_count) is outside [0, n)"),
    ]
    for (n, precision, kw), want in cases:
        rc, text, h = _create(nbx, n, precision, **kw)
        assert rc == nbx.NBX_ERR_ARG and text == want, (n, precision, kw, rc, text)
        assert not h


# ---------------------------------------------------------------------------------------------------------------------------
# on the device: state errors of live contexts; one step at most is launched
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_create_on_a_device_that_is_not_there(nbx):
    rc, text, h = _create(nbx, N, 32, device=9999)
    assert rc == nbx.NBX_ERR_ARG and text == "nbx_create: device ordinal out of range", text
    assert not h


@pytest.mark.gpu
def test_state_errors_of_a_live_context(nbx):
    null = ctypes.c_void_p()
    ke = (ctypes.c_double * 4)()
    buf = (ctypes.c_float * N)()
    dg = nbx.Diag()
    dg.struct_size = ctypes.sizeof(nbx.Diag)
    s0 = nbx.initial_conditions(N, 32)
    arrs = [s0[f].ctypes.data_as(ctypes.c_void_p) for f in nbx.FIELDS]
    with nbx.Context(N, 32) as c:
        h = c._h
        # before an upload
        for fn, args in (("nbx_step", (h, 0.1, 1, ke)), ("nbx_step_local", (h, 0.1)), ("nbx_accel", (h, buf, buf, buf)),
                         ("nbx_download", (h,) + (buf,) * 6), ("nbx_diagnostics", (h, ctypes.byref(dg)))):
            rc, text = _call(nbx, fn, *args)
            assert rc == nbx.NBX_ERR_STATE and text == fn + ": nbx_upload has not been called", (fn, rc, text)
        rc, text = _call(nbx, "nbx_step_trace", h, 0.1, 1, ke)
        assert rc == nbx.NBX_ERR_STATE and text == "nbx_step: nbx_upload has not been called", text
        # nsteps < 0 is an argument error whatever has been uploaded
        for fn in ("nbx_step", "nbx_step_trace"):
            rc, text = _call(nbx, fn, h, 0.1, -1, ke)
            assert rc == nbx.NBX_ERR_ARG and text == "nbx_step: nsteps < 0", (fn, text)
        rc, text = _call(nbx, "nbx_commit", h)
        assert rc == nbx.NBX_ERR_STATE and text == "nbx_commit: no local step pending", text
        for hole in range(7):
            rc, text = _call(nbx, "nbx_upload", h, *[null if i == hole else a for i, a in enumerate(arrs)])
            assert rc == nbx.NBX_ERR_ARG and text == "nbx_upload: NULL array", (hole, text)
        rc, text = _call(nbx, "nbx_step", h, 0.1, 1, ke)  # a refused upload uploads nothing
        assert rc == nbx.NBX_ERR_STATE and text == "nbx_step: nbx_upload has not been called", text
        rc, text = _call(nbx, "nbx_exchange_buffer", h, None, None, None, None)
        assert rc == nbx.NBX_ERR_ARG and text == "nbx_exchange_buffer: NULL argument", text
        rc, text = _call(nbx, "nbx_kenergy_partial", h, None)
        assert rc == nbx.NBX_ERR_ARG and text == "nbx_kenergy_partial: NULL argument", text
        rc, text = _call(nbx, "nbx_stats", h, None)
        assert rc == nbx.NBX_ERR_ARG and text == "nbx_stats: NULL argument", text

        c.upload(s0)
        # struct_size of another library version
        dg.struct_size = ctypes.sizeof(nbx.Diag) - 8
        rc, text = _call(nbx, "nbx_diagnostics", h, ctypes.byref(dg))
        assert rc == nbx.NBX_ERR_ARG and text == "nbx_diagnostics: nbx_diag_t.struct_size does not match this library", text
        dg.struct_size = ctypes.sizeof(nbx.Diag)
        # while a commit is pending
        c.step_local()
        for fn, args, want in (("nbx_step", (h, 0.1, 1, ke), "nbx_step: a local step awaits nbx_commit"),
                               ("nbx_step_trace", (h, 0.1, 1, ke), "nbx_step: a local step awaits nbx_commit"),
                               ("nbx_step_local", (h, 0.1), "nbx_step_local: previous step not committed"),
                               ("nbx_accel", (h, buf, buf, buf), "nbx_accel: a local step awaits nbx_commit"),
                               ("nbx_diagnostics", (h, ctypes.byref(dg)), "nbx_diagnostics: a local step awaits nbx_commit")):
            rc, text = _call(nbx, fn, *args)
            assert rc == nbx.NBX_ERR_STATE and text == want, (fn, rc, text)
        c.commit()
        rc, text = _call(nbx, "nbx_commit", h)
        assert rc == nbx.NBX_ERR_STATE and text == "nbx_commit: no local step pending", text
        assert c.stats()["steps_done"] == 1


@pytest.mark.gpu
def test_nbx_step_on_a_context_that_owns_a_slice(nbx):
    ke = (ctypes.c_double * 4)()
    with nbx.Context(N, 32, i_begin=0, i_count=32) as c:
        rc, text = _call(nbx, "nbx_step", c._h, 0.1, 1, ke)  # the upload is looked at first
        assert rc == nbx.NBX_ERR_STATE and text == "nbx_step: nbx_upload has not been called", text
        c.upload(nbx.initial_conditions(N, 32))
        for fn in ("nbx_step", "nbx_step_trace"):
            rc, text = _call(nbx, fn, c._h, 0.1, 1, ke)
            assert rc == nbx.NBX_ERR_STATE, (fn, rc)
            assert text == "nbx_step: context owns a slice; use nbx_step_local + exchange + nbx_commit", (fn, text)
        assert c.stats()["steps_done"] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# a time step that is not finite: after the NULL-handle and nsteps checks, before the state is looked at
# ---------------------------------------------------------------------------------------------------------------------------
NOT_FINITE = (float("nan"), float("inf"), float("-inf"))


def test_a_null_handle_and_nsteps_are_reported_before_a_time_step_that_is_not_finite(nbx):
    null = ctypes.c_void_p()
    ke = (ctypes.c_double * 4)()
    for dt in NOT_FINITE:
        for fn, args, want in (("nbx_step", (null, dt, 1, ke), "nbx_step: ctx is NULL"), ("nbx_step_trace", (null, dt, 1, ke), "nbx_step: ctx is NULL"),
                               ("nbx_step_local", (null, dt), "nbx_step_local: ctx is NULL"),
                               ("nbx_group_step", (null, dt, 1, ke), "nbx_group_step: group is NULL"),
                               ("nbx_group_step", (null, dt, -1, ke), "nbx_group_step: group is NULL")):
            rc, text = _call(nbx, fn, *args)
            assert rc == nbx.NBX_ERR_ARG and text == want, (fn, dt, rc, text)


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [1, 2])
def test_a_time_step_that_is_not_finite_is_refused(nbx, use_graph):
    """NaN and both infinities, before and after an upload.  A NaN equals no cached graph's dt, its own included: with graph
    replay on, every such call used to capture and keep one more graph until nbx_destroy."""
    ke = (ctypes.c_double * 8)()
    s0 = nbx.initial_conditions(N, 32)
    with nbx.Context(N, 32, use_graph=use_graph) as c:
        h = c._h
        for uploaded in (False, True):
            for dt in NOT_FINITE:
                for fn, args, want in (("nbx_step", (h, dt, 8, ke), "nbx_step"), ("nbx_step", (h, dt, 0, None), "nbx_step"),
                                       ("nbx_step_trace", (h, dt, 8, ke), "nbx_step"), ("nbx_step_local", (h, dt), "nbx_step_local")):
                    rc, text = _call(nbx, fn, *args)
                    assert rc == nbx.NBX_ERR_ARG and text == want + ": dt is not finite", (fn, dt, uploaded, rc, text)
                for fn in ("nbx_step", "nbx_step_trace"):  # nsteps is looked at first
                    rc, text = _call(nbx, fn, h, dt, -1, ke)
                    assert rc == nbx.NBX_ERR_ARG and text == "nbx_step: nsteps < 0", (fn, text)
            if not uploaded:
                rc, text = _call(nbx, "nbx_step", h, 0.1, 1, ke)  # a finite one gets as far as the state
                assert rc == nbx.NBX_ERR_STATE and text == "nbx_step: nbx_upload has not been called", text
                c.upload(s0)
        st = c.stats()
        assert st["steps_done"] == 0 and st["graph_replays"] == 0, st
        rc, text = _call(nbx, "nbx_commit", h)  # a refused local step leaves nothing to commit
        assert rc == nbx.NBX_ERR_STATE and text == "nbx_commit: no local step pending", text
        d = c.download()
        for f in d:
            assert (d[f] == s0[f]).all(), f
        # zero and negative time steps are time steps
        ke0 = c.step(8, dt=0.0)
        assert ke0 > 0 and c.step(8, dt=-0.0) == ke0 and c.step(2, dt=-0.125) > 0 and c.stats()["steps_done"] == 18


@pytest.mark.gpu
def test_a_group_refuses_a_time_step_that_is_not_finite(nbx):
    ke = ctypes.c_double()
    s0 = nbx.initial_conditions(N, 32)
    with nbx.Group(N, 32, n_ranks=1, devices=[0]) as g:
        for uploaded in (False, True):
            for dt in NOT_FINITE:
                rc, text = _call(nbx, "nbx_group_step", g._h, dt, 1, ctypes.byref(ke))
                assert rc == nbx.NBX_ERR_ARG and text == "nbx_group_step: dt is not finite", (dt, uploaded, rc, text)
                rc, text = _call(nbx, "nbx_group_step", g._h, dt, -1, ctypes.byref(ke))
                assert rc == nbx.NBX_ERR_ARG and text == "nbx_group_step: nsteps < 0", (dt, text)
            g.upload(s0)
        assert g.info(0)[2]["steps_done"] == 0
        d = g.download()
        for f in d:
            assert (d[f] == s0[f]).all(), f
