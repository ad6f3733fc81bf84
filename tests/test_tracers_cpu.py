"""Resident tracers (include/nbx_tracers.h), the parts that need no GPU: the header and its fifteen exported symbols, the
statuses that come before the first HIP call in the header's order, the Python methods, the build files, the compiler's resource
summary of the cross-compiled gfx950 kernels of nbx_tracers.hip, and the numpy restatement tests/tracers_ref.py, whose eight
planted faults must each fail the comparison the device tests apply (tracers_ref.same against tracers_ref.round_trip).

All faults are planted at (n, m) = (2049, 1025): three tracer columns, the last with one tracer, and two j splits of 5 and 4
tiles, over two steps of dt = 0.01 -- the second step reads what the first one left, and a dt is not exact -- in both precisions."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref as R
import kick_ref as K
import tracers_ref as TR
from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_tracers.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KINDS = (("nbx", "nbx_ctx", "ctx"), ("nbx_ensemble", "nbx_ensemble", "ensemble"), ("nbx_ragged", "nbx_ragged", "ragged ensemble"))
WORDS = ("upload", "download", "count", "step", "kick")
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h", "nbx_field.h", "nbx_neighbours.h", "nbx_paircount.h")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


def _signature(prefix, handle, word):
    """(parameter list, argument count) of <prefix>_tracers_<word> as the header declares it."""
    batch = prefix != "nbx"
    rng = "int32_t, int32_t, " if batch else ""
    return {"upload": ("%s*, %sint32_t, const void*, const void*, const void*, const void*, const void*, const void*" % (handle, rng), 10 if batch else 8),
            "download": ("%s*, %svoid*, void*, void*, void*, void*, void*" % (handle, rng), 9 if batch else 7),
            "count": ("%s*, int32_t*" % handle, 2),
            "step": ("%s*, double, int32_t, double*" % handle, 4),
            "kick": ("%s*, double" % handle, 2)}[word]


def _program():
    """A main that takes the address of every function through a pointer of the declared type, and stubs that define them."""
    main = ['#include <stdio.h>', '#include <stddef.h>', '#include "nbx_tracers.h"', 'int main(void) { int ok = 1;']
    stubs = ['#include "nbx_tracers.h"']
    for prefix, handle, _ in KINDS:
        for word in WORDS:
            name = "%s_tracers_%s" % (prefix, word)
            params, _ = _signature(prefix, handle, word)
            main.append("{ int (*f)(%s) = %s; ok = ok && f != NULL; }" % (params, name))
            named = ", ".join("%s a%d" % (t.strip(), k) for k, t in enumerate(params.split(",")))
            unused = " ".join("(void)a%d;" % k for k in range(len(params.split(","))))
            stubs.append("int %s(%s) { %s return 0; }" % (name, named, unused))
    main.append('printf("ok\\n"); return ok ? NBX_ABI_VERSION - 1 : 1; }')
    return "\n".join(main) + "\n", "\n".join(stubs) + "\n"


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in zip(("main", "stubs"), _program()):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "tracers_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_fifteen_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_tracers.h")
    want = sorted("%s_tracers_%s" % (prefix, word) for prefix, _, _ in KINDS for word in WORDS)
    assert declared == want and sorted(nbx.TRACER_SYMBOLS) == want and len(want) == 15
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "tracers_" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for prefix, handle, _ in KINDS:
        for word in WORDS:
            s = "%s_tracers_%s" % (prefix, word)
            assert re.search(r" T %s$" % s, out, flags=re.M), s
            assert len(getattr(L, s).argtypes) == _signature(prefix, handle, word)[1], s
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = open(os.path.join(ROOT, "include", "nbx_tracers.h")).read()
    for word in ("Why:", "Definition", "Arrays:", "Contracts:", "Semantics:", "Status, in this order", "Unspecified results", "Deliberately not here",
                 "Bodies are untouched", "bit for bit what nbx_step(dt, N) gives", "replayed a graph", "The tracer acceleration is nbx_field's",
                 "step(3); step(2) is step(5)", "velocity-only", "kick(-dt/2) on both", "Independence", "not counted in the profile",
                 "cached graphs", "no self-exclusion", "BEFORE their step", "never contracted", "2^22", "32 bits", "before the first HIP call",
                 "NBX_ERR_ALLOC", "synchronises", "groups and sliced contexts", "tracers with mass", "back-reaction", "a different m per",
                 "per-tracer time steps", "device pointers", "tracer energies", "nbody.x", "not finite"):
        assert word in doc, word


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("prefix,handle_type,noun", KINDS)
def test_statuses_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, prefix, handle_type, noun):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies uploaded and no tracers: it
    reaches the state checks and nothing behind them, and no call writes a byte of it."""
    L = nbx.load()
    batch = prefix != "nbx"
    f = {w: getattr(L, "%s_tracers_%s" % (prefix, w)) for w in WORDS}
    where = {w: "%s_tracers_%s" % (prefix, w) for w in WORDS}
    err = lambda: L.nbx_last_error().decode()
    six = [np.full(8, 0.25, dtype=np.float64) for _ in range(6)]
    out = [np.full(8, -7.25, dtype=np.float64) for _ in range(6)]
    ke = np.full(4, -7.25)
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    rng = lambda first, count: (first, count) if batch else ()
    up = lambda h, m, arrs, first=0, count=0: f["upload"](h, *rng(first, count), m, *[_ptr(a) for a in arrs])
    down = lambda h, arrs, first=0, count=0: f["download"](h, *rng(first, count), *[_ptr(a) for a in arrs])
    m_out = ctypes.c_int32(-7)
    # 1. the handle is NULL -- whatever else is wrong
    for call, w in ((lambda: up(None, -1, [None] * 6, -1, 5), "upload"), (lambda: down(None, out, -1, 5), "download"),
                    (lambda: f["count"](None, None), "count"), (lambda: f["step"](None, math.nan, -1, None), "step"),
                    (lambda: f["kick"](None, math.inf), "kick")):
        assert call() == nbx.NBX_ERR_ARG and err() == "%s: %s is NULL" % (where[w], noun), w
    assert f["count"](handle, None) == nbx.NBX_ERR_ARG and err() == where["count"] + ": m is NULL"
    assert f["count"](handle, ctypes.byref(m_out)) == nbx.NBX_OK and m_out.value == 0
    # 2. m < 0 -- before the arrays and the range
    assert up(handle, -1, [None] * 6, -1, 5) == nbx.NBX_ERR_ARG and err() == where["upload"] + ": m < 0"
    # 3. m > 0 and a NULL array -- before the range and the bound
    for k in range(6):
        arrs = list(six)
        arrs[k] = None
        assert up(handle, (1 << 22) + 1, arrs, -1, 5) == nbx.NBX_ERR_ARG and err() == where["upload"] + ": NULL array", k
    if batch:
        # 4. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for call, w in ((lambda: up(handle, 4, six, first, count), "upload"), (lambda: down(handle, out, first, count), "download")):
                assert call() == nbx.NBX_ERR_ARG and err() == where[w] + ": members [first, first + count) are outside [0, members)", (w, first, count)
        assert up(handle, 4, six, 0, 0) == nbx.NBX_OK and up(handle, 0, [None] * 6, 0, 0) == nbx.NBX_OK  # count == 0: nothing is copied
    else:
        # 5. more than 2^22 tracers -- the arrays are not read
        assert up(handle, (1 << 22) + 1, six) == nbx.NBX_ERR_ARG and err() == where["upload"] + ": m exceeds 4194304"
        assert up(handle, 0, [None] * 6) == nbx.NBX_OK  # m == 0 removes a set that is not there
    # 6., 7. nsteps < 0, then a time step that is not finite -- before the state
    assert f["step"](handle, math.nan, -1, _ptr(ke)) == nbx.NBX_ERR_ARG and err() == where["step"] + ": nsteps < 0"
    for bad in (math.nan, math.inf, -math.inf):
        assert f["step"](handle, bad, 3, _ptr(ke)) == nbx.NBX_ERR_ARG and err() == where["step"] + ": dt is not finite"
        assert f["kick"](handle, bad) == nbx.NBX_ERR_ARG and err() == where["kick"] + ": h is not finite"
    # 8., 9. the state: a zeroed context has no bodies; a zeroed batch object has no member without them, and then no tracers
    state = "nbx_upload has not been called" if not batch else "no tracers have been uploaded"
    for nsteps in (0, 3):
        assert f["step"](handle, 0.25, nsteps, _ptr(ke)) == nbx.NBX_ERR_STATE and err() == "%s: %s" % (where["step"], state)
    assert f["kick"](handle, 0.25) == nbx.NBX_ERR_STATE and err() == "%s: %s" % (where["kick"], state)
    assert down(handle, out) == nbx.NBX_ERR_STATE and err() == where["download"] + ": no tracers have been uploaded"
    assert all((a == -7.25).all() for a in out) and (ke == -7.25).all() and zeroed.raw == bytes(1 << 16)


def test_python_methods(nbx):
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.tracers_upload).parameters
        assert list(p) == ["self", "points", "velocities", "first"] and p["first"].default == 0, cls
        p = inspect.signature(cls.tracers_download).parameters
        assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
        p = inspect.signature(cls.tracers_step).parameters
        assert list(p) == ["self", "nsteps", "dt", "kenergy"] and p["dt"].default == nbx.DT and p["kenergy"].default is True, cls
        assert list(inspect.signature(cls.tracers_kick).parameters) == ["self", "h"], cls
        p = inspect.signature(cls.tracers_leapfrog).parameters
        assert list(p)[:3] == ["self", "nsteps", "dt"] and p["dt"].default == nbx.DT, cls
        assert cls.tracers_leapfrog is nbx._Tracers.tracers_leapfrog, cls
    assert not hasattr(nbx.Group, "tracers_step")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "tracer" in f]  # no new nbx_opts field
    calls = []

    class Fake(nbx._Tracers):
        def kick(self, h, kenergy=False):
            calls.append(("kick", h, kenergy))
            return "ke" if kenergy else None

        def tracers_kick(self, h):
            calls.append(("tracers_kick", h))

        def tracers_step(self, nsteps, dt, kenergy=True):
            calls.append(("tracers_step", nsteps, dt, kenergy))

    assert Fake().tracers_leapfrog(7, 0.25) == "ke"
    assert sorted(calls[:2], key=str) == [("kick", -0.125, False), ("tracers_kick", -0.125)] and calls[2] == ("tracers_step", 7, 0.25, False)
    assert sorted(calls[3:], key=str) == [("kick", 0.125, True), ("tracers_kick", 0.125)]


def test_a_library_without_the_unit_names_the_missing_symbol(nbx):
    class Lib:
        pass

    with pytest.raises(nbx.NbxError) as e:
        nbx._need(Lib(), "nbx_tracers_step")
    assert e.value.code == nbx.NBX_ERR_STATE and "nbx_tracers_step" in str(e.value)


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_tracers\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_tracers\.o: \$\(CSRC\)/nbx_tracers\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    assert rule
    for dep in ("nbx_tracers_kernels.hpp", "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_pair.hpp", "include/nbx_tracers.h", "include/nbx_ensemble.h",
                "include/nbx_ragged.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_tracers.hip", "include/nbx_tracers.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_and_the_body_step_goes_through_the_units_hooks():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_tracers.hip":
            assert "nbx_tracers_kernels.hpp" not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_tracers.hip", "nbx_tracers_kernels.hpp"):
            assert "tracer_kernel" not in txt and "tracer_body" not in txt and "tracer_update_kernel" not in txt, f
    src = re.sub(r"//.*", "", open(SRC).read())
    kern = re.sub(r"//.*", "", open(os.path.join(CSRC, "nbx_tracers_kernels.hpp")).read())
    assert "atomic" not in src + kern and "hipGraph" not in src and "hipStreamBeginCapture" not in src
    assert '#include "nbx_field_shape.hpp"' in kern and "field_shape(" in kern and "field_shape(" in src  # the field's rule, no new one
    assert not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", src + kern)
    assert "pair2(" in kern and "pair<T>(" in kern and "euler_update<T>(" in kern and "kick_update<T>(" in kern
    assert "enqueue_one_step(c, dt)" in src and "enqueue_step(o, dt)" in src  # the step's own launches
    api = open(os.path.join(CSRC, "nbx_api.hip")).read()
    hook = api[api.index("int nbx_detail::enqueue_one_step("):]
    assert "enqueue_step_any(c, dt)" in hook[:hook.index("\n}\n")] and "c->cur ^= 1;" in hook[:hook.index("\n}\n")]
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<"):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in src, fn
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("tr_pos", "tr_vel", "tr_part", "tr_tab"):
        assert re.search(r"void\* %s = nullptr;" % field, obj) and "o->%s" % field in obj[obj.index("inline void batch_release"):], field


# ---------------------------------------------------------------------------------------------------------------------------
# the compiler's resource summary of the cross-compiled unit
# ---------------------------------------------------------------------------------------------------------------------------
def _shipped_hipflags():
    """The flags libnbx.so is built with (top-level Makefile, HIPFLAGS): the audited code must be the executed code."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel symbol: {remark name: value}} from -Rpass-analysis=kernel-resource-usage."""
    obj = tmp_path_factory.mktemp("tracers") / "nbx_tracers.o"
    p = subprocess.run(["hipcc"] + _shipped_hipflags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", str(obj)],
                       capture_output=True, text=True, check=True)
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: \s*([A-Za-z][\w \[\]/]*?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _kind(name):
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)tracer_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+tracer_update_kernelI([fd])Lb([01])EEE", name)
    if m:
        return ("kick" if m.group(2) == "1" else "update", 32 if m.group(1) == "f" else 64)
    return None


def test_the_unit_compiles_to_ten_kernels_without_scratch_or_spills(resources):
    keys = sorted(_kind(k) or ("?", k) for k in resources)
    assert keys == sorted((kind, p) for kind in ("context", "ensemble", "ragged", "update", "kick") for p in (32, 64)), keys
    for name, r in resources.items():
        kind, precision = _kind(name)
        print("%-8s fp%d: %3d VGPRs, %2d SGPRs, scratch %d, LDS %d, occupancy %d" % (kind, precision, r["VGPRs"], r["TotalSGPRs"],
              r["ScratchSize [bytes/lane]"], r["LDS Size [bytes/block]"], r["Occupancy [waves/SIMD]"]))
        assert r["ScratchSize [bytes/lane]"] == 0, name
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, name
        assert r["VGPRs"] <= 128, name  # at least four waves per SIMD
        if kind in ("update", "kick"):
            assert r["LDS Size [bytes/block]"] == 0, name
        else:
            assert r["LDS Size [bytes/block]"] == 256 * (16 if precision == 32 else 32), name  # one tile of position records


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement on its own, and its planted faults against the comparison the device tests apply
# ---------------------------------------------------------------------------------------------------------------------------
N, M, STEPS, DT = 2049, 1025, 2, 0.01  # no power of two: a dt rounds, so a fused a dt + w differs from the separate operations
_case = {}


def _setup(precision):
    if precision not in _case:
        T = R.DTYPE[precision]
        state = K.make_state(8100, N, T)
        tracers = TR.make_tracers(precision, state, M, seed=3)
        other = TR.make_tracers(precision, state, M, seed=4)  # member 0's, for the fault that reads them
        want, _ = TR.round_trip(TR.RefTwin(state, precision), tracers, precision, DT, STEPS)
        _case[precision] = (state, tracers, other, TR.body_states(state, DT, STEPS), want)
    return _case[precision]


def test_the_shape_the_faults_are_planted_at():
    assert R.field_shape(M, N) == (3, 9, 2, 5) and M % 512 == 1 and STEPS >= 2 and len(TR.FAULTS) == 8


@pytest.mark.parametrize("precision", [32, 64])
def test_the_unfaulted_restatement_holds_the_round_trips_bits(precision):
    state, tracers, other, states, want = _setup(precision)
    got = TR.restate_step(states, tracers, precision, DT, STEPS)
    assert TR.same(got, want)
    assert not TR.same(got, tracers) and all(got[k].dtype == R.DTYPE[precision] for k in TR.KEYS)
    # step(1); step(1) is step(2)
    half = TR.restate_step(states, tracers, precision, DT, 1)
    assert TR.same(TR.restate_step(states[1:], half, precision, DT, 1), want)
    # the kick: the round trip's bits, positions untouched, and a(p) h what one step from rest leaves in w
    kicked = TR.restate_kick(state, tracers, precision, -0.5 * DT)
    assert TR.same(kicked, TR.round_trip_kick(TR.RefTwin(state, precision), tracers, precision, -0.5 * DT))
    assert all(np.array_equal(kicked[k], tracers[k]) for k in TR.POS) and not any(np.array_equal(kicked[k], tracers[k]) for k in TR.VEL)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_fails_the_comparison(precision):
    state, tracers, other, states, want = _setup(precision)
    kick_want = TR.round_trip_kick(TR.RefTwin(state, precision), tracers, precision, DT)
    planted = set()
    for fault in TR.FAULTS:
        if fault == "the kick also moves positions":
            got = TR.restate_kick(state, tracers, precision, DT, fault=fault)
            assert not TR.same(got, kick_want), fault
            assert all(np.array_equal(got[k], kick_want[k]) for k in TR.VEL)  # the velocities are right: the positions show it
        else:
            got = TR.restate_step(states, tracers, precision, DT, STEPS, fault=fault, member0=other)
            assert not TR.same(got, want), fault
            differ = np.zeros(M, dtype=bool)
            for k in TR.KEYS:
                differ |= got[k] != want[k]
            print("fp%d %-46s: %4d of %d tracers differ" % (precision, fault, int(differ.sum()), M))
            if fault == "tail tracers of the last column not advanced":
                assert list(np.nonzero(differ)[0]) == [M - 1]  # the one tracer of the third column
            if fault == "cur not flipped between steps":
                assert TR.same(TR.restate_step(states, tracers, precision, DT, 1, fault=fault), TR.restate_step(states, tracers, precision, DT, 1))
        planted.add(fault)
    assert planted == set(TR.FAULTS)
