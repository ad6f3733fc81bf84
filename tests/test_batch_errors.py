"""The argument and state errors of the two batch objects -- nbx_ensemble (include/nbx_ensemble.h, nbx_ensemble_diag.h) and
nbx_ragged (include/nbx_ragged.h, nbx_ragged_diag.h) -- as the exact text nbx_last_error() gives for each.  The texts are
literal: both kinds share one host layer (csrc/nbx_batch.hpp) that puts them together from a names record per kind, and
every one of them must come out byte for byte as it did when each kind had its own copy.

The first part needs no GPU (every case returns before the first HIP call); the second creates the smallest objects, an
ensemble of 3 members of 65 bodies and a ragged ensemble of sizes (5, 65, 257), and every case returns before any launch."""
import ctypes

import pytest

KINDS = [("nbx_ensemble", "ensemble"), ("nbx_ragged", "ragged ensemble")]
RANGE = "members [first, first + count) are outside [0, members)"


def _call(nbx, name, *args):
    """(return code, nbx_last_error() text) of one raw C-ABI call"""
    L = nbx.load()
    rc = getattr(L, name)(*args)
    return rc, L.nbx_last_error().decode()


def _stats_type(nbx, prefix):
    return nbx.EnsembleStats if prefix == "nbx_ensemble" else nbx.RaggedStats


def _raw_create(nbx, prefix, out, opts):
    if prefix == "nbx_ensemble":
        return _call(nbx, prefix + "_create", out, 65, 32, 3, opts)
    sizes = (ctypes.c_int32 * 3)(5, 65, 257)
    return _call(nbx, prefix + "_create", out, 3, sizes, 32, opts)


# ---------------------------------------------------------------------------------------------------------------------------
# no GPU: everything here is refused before the first HIP call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix,noun", KINDS)
def test_null_handle_texts(nbx, prefix, noun):
    null = ctypes.c_void_p()
    d = (ctypes.c_double * 4)()
    cases = [
        ("_upload", (null, 0, 1) + (null,) * 7), ("_step", (null, 0.1, 1, None)), ("_step", (null, 0.1, 1, d)),
        ("_step_trace", (null, 0.1, 1, d)), ("_download", (null, 0, 1) + (null,) * 6), ("_sync", (null,)), ("_profile", (null, 1)),
        ("_profile", (null, 0)),
    ]
    for fn, args in cases:
        rc, text = _call(nbx, prefix + fn, *args)
        assert rc == nbx.NBX_ERR_ARG, (fn, rc, text)
        assert text == "%s%s: %s is NULL" % (prefix, fn, noun), (fn, text)


@pytest.mark.parametrize("prefix,noun", KINDS)
def test_null_ke_trace_is_reported_before_the_handle_is_looked_at(nbx, prefix, noun):
    rc, text = _call(nbx, prefix + "_step_trace", ctypes.c_void_p(), 0.1, 1, None)
    assert rc == nbx.NBX_ERR_ARG and text == prefix + "_step_trace: ke_trace is NULL", text


@pytest.mark.parametrize("prefix,noun", KINDS)
def test_stats_and_diagnostics_with_null_arguments(nbx, prefix, noun):
    null = ctypes.c_void_p()
    st = _stats_type(nbx, prefix)()
    one = (nbx.Diag * 1)()
    for fn, args in (("_stats", (null, ctypes.byref(st))), ("_stats", (null, None)),
                     ("_diagnostics", (null, 0, 1, one)), ("_diagnostics", (null, 0, 1, None))):
        rc, text = _call(nbx, prefix + fn, *args)
        assert rc == nbx.NBX_ERR_ARG and text == "%s%s: NULL argument" % (prefix, fn), (fn, text)


@pytest.mark.parametrize("prefix,noun", KINDS)
def test_create_with_null_out_and_with_a_foreign_opts_size(nbx, prefix, noun):
    rc, text = _raw_create(nbx, prefix, None, None)
    assert rc == nbx.NBX_ERR_ARG and text == prefix + "_create: out is NULL", text
    h = ctypes.c_void_p(1)
    o = nbx.Opts()
    o.struct_size = ctypes.sizeof(nbx.Opts) + 4
    o.device = -1
    rc, text = _raw_create(nbx, prefix, ctypes.byref(h), ctypes.byref(o))
    assert rc == nbx.NBX_ERR_ARG and text == prefix + "_create: nbx_opts.struct_size does not match this library", text
    assert not h.value  # *out is cleared before anything else is looked at


# ---------------------------------------------------------------------------------------------------------------------------
# on the device: state and range errors of live objects; none of them launches anything
# ---------------------------------------------------------------------------------------------------------------------------
SIZES = {"nbx_ensemble": (65, 65, 65), "nbx_ragged": (5, 65, 257)}


def _make(nbx, prefix):
    return nbx.Ensemble(65, 3, 32) if prefix == "nbx_ensemble" else nbx.Ragged(SIZES[prefix], 32)


@pytest.mark.gpu
@pytest.mark.parametrize("prefix,noun", KINDS)
def test_range_and_state_errors_of_a_live_object(nbx, prefix, noun):
    sizes = SIZES[prefix]
    null = ctypes.c_void_p()
    diag = (nbx.Diag * 4)()
    for k in range(4):
        diag[k].struct_size = ctypes.sizeof(nbx.Diag)
    ke = (ctypes.c_double * 8)()
    with _make(nbx, prefix) as o:
        h = o._h
        # [first, first + count) outside [0, 3): checked before the arrays, the uploaded flags and out[k].struct_size
        for first, count in ((2, 2), (3, 1), (-1, 1), (0, -1), (0, 4), (2**31 - 1, 2**31 - 1)):
            for fn, args in (("_upload", (h, first, count) + (null,) * 7), ("_download", (h, first, count) + (null,) * 6),
                             ("_diagnostics", (h, first, count, diag))):
                rc, text = _call(nbx, prefix + fn, *args)
                assert rc == nbx.NBX_ERR_ARG and text == "%s%s: %s" % (prefix, fn, RANGE), (fn, first, count, text)
        s0 = nbx.initial_conditions(sizes[0], 32)
        arrs = [s0[f].ctypes.data_as(ctypes.c_void_p) for f in nbx.FIELDS]
        for hole in range(7):
            rc, text = _call(nbx, prefix + "_upload", h, 0, 1, *[null if i == hole else a for i, a in enumerate(arrs)])
            assert rc == nbx.NBX_ERR_ARG and text == prefix + "_upload: NULL array", (hole, text)
        # nsteps < 0 is an argument error whatever has been uploaded
        for fn in ("_step", "_step_trace"):
            rc, text = _call(nbx, prefix + fn, h, 0.1, -1, ke)
            assert rc == nbx.NBX_ERR_ARG and text == "%s%s: nsteps < 0" % (prefix, fn), text
        # nothing uploaded, then member 0 only
        rc, text = _call(nbx, prefix + "_step", h, 0.1, 1, ke)
        assert rc == nbx.NBX_ERR_STATE and text == "%s_step: 3 of 3 members have not been uploaded (%s_upload)" % (prefix, prefix), text
        o.upload([s0])
        for fn in ("_step", "_step_trace"):
            rc, text = _call(nbx, prefix + fn, h, 0.1, 1, ke)
            assert rc == nbx.NBX_ERR_STATE, text
            assert text == "%s%s: 2 of 3 members have not been uploaded (%s_upload)" % (prefix, fn, prefix), text
        for first, count, k in ((1, 1, 1), (0, 3, 1), (2, 1, 2)):
            for fn, args in (("_download", (h, first, count) + (null,) * 6), ("_diagnostics", (h, first, count, diag))):
                rc, text = _call(nbx, prefix + fn, *args)
                assert rc == nbx.NBX_ERR_STATE and text == "%s%s: member %d has not been uploaded" % (prefix, fn, k), (fn, first, text)
        # struct_size of another library version: stats, and out[1] of diagnostics (looked at before the uploaded flags)
        st = _stats_type(nbx, prefix)()
        st.struct_size = ctypes.sizeof(st) + 8
        rc, text = _call(nbx, prefix + "_stats", h, ctypes.byref(st))
        assert rc == nbx.NBX_ERR_ARG and text == "%s_stats: %s_stats_t.struct_size does not match this library" % (prefix, prefix), text
        diag[1].struct_size = ctypes.sizeof(nbx.Diag) - 8
        rc, text = _call(nbx, prefix + "_diagnostics", h, 0, 3, diag)
        assert rc == nbx.NBX_ERR_ARG and text == prefix + "_diagnostics: out[1].struct_size does not match this library", text
        rc, text = _call(nbx, prefix + "_diagnostics", h, 0, 1, diag)  # out[1] is outside a range of one member
        assert rc == nbx.NBX_OK, text
        assert o.stats()["steps_done"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("prefix,noun", KINDS)
def test_create_on_a_device_that_is_not_there(nbx, prefix, noun):
    h = ctypes.c_void_p()
    o = nbx.Opts()
    o.struct_size = ctypes.sizeof(nbx.Opts)
    o.device = 9999
    rc, text = _raw_create(nbx, prefix, ctypes.byref(h), ctypes.byref(o))
    assert rc == nbx.NBX_ERR_ARG and text == prefix + "_create: device ordinal out of range", text
    assert not h.value


# ---------------------------------------------------------------------------------------------------------------------------
# a time step that is not finite: after the NULL-handle and nsteps checks, before the members' uploads are looked at
# ---------------------------------------------------------------------------------------------------------------------------
NOT_FINITE = (float("nan"), float("inf"), float("-inf"))


@pytest.mark.parametrize("prefix,noun", KINDS)
def test_a_null_handle_is_reported_before_a_time_step_that_is_not_finite(nbx, prefix, noun):
    d = (ctypes.c_double * 4)()
    for dt in NOT_FINITE:
        for fn in ("_step", "_step_trace"):
            rc, text = _call(nbx, prefix + fn, ctypes.c_void_p(), dt, 1, d)
            assert rc == nbx.NBX_ERR_ARG and text == "%s%s: %s is NULL" % (prefix, fn, noun), (fn, dt, text)


@pytest.mark.gpu
@pytest.mark.parametrize("prefix,noun", KINDS)
def test_a_time_step_that_is_not_finite_is_refused(nbx, prefix, noun):
    sizes = SIZES[prefix]
    ke = (ctypes.c_double * 8)()
    states = [nbx.initial_conditions(n, 32) for n in sizes]
    with _make(nbx, prefix) as o:
        for uploaded in (False, True):
            for dt in NOT_FINITE:
                for fn, args in (("_step", (o._h, dt, 1, ke)), ("_step", (o._h, dt, 0, None)), ("_step_trace", (o._h, dt, 2, ke))):
                    rc, text = _call(nbx, prefix + fn, *args)
                    assert rc == nbx.NBX_ERR_ARG and text == "%s%s: dt is not finite" % (prefix, fn), (fn, dt, uploaded, rc, text)
                for fn in ("_step", "_step_trace"):  # nsteps is looked at first
                    rc, text = _call(nbx, prefix + fn, o._h, dt, -1, ke)
                    assert rc == nbx.NBX_ERR_ARG and text == "%s%s: nsteps < 0" % (prefix, fn), (fn, text)
            if not uploaded:
                o.upload(states)
        assert o.stats()["steps_done"] == 0
        d = o.download()
        for m, s0 in enumerate(states):
            for f in nbx.FIELDS[:6]:
                assert (d[f][m] == s0[f]).all() if prefix == "nbx_ensemble" else (d[m][f] == s0[f]).all(), (m, f)
