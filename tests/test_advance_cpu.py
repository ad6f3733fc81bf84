"""Adaptive power-of-two time steps chosen on the device (include/nbx_advance.h), the parts that need no GPU: the header and its six
exported symbols, the argument checks that come before the first HIP call, the Python methods, the build files, an audit of the
cross-compiled gfx950 code of nbx_advance.hip, and the numpy restatement tests/advance_ref.py, which must show by itself what the
device tests then ask of the library: that every history keeps t a multiple of h, that h at most doubles, that every system lands
on t_end exactly, that the scheme beats a fixed step of the same cost on an eccentric orbit, and that every planted fault changes
a history or an end state."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import advance_ref as A
import hermite_ref as H
import jerk_ref as R
from conftest import ROOT, PKG
from energy_ref import G32

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_advance.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_advance_kernels.hpp"
ADVANCE = ("nbx_advance", "nbx_ensemble_advance", "nbx_ragged_advance")
CLOCK = ("nbx_clock", "nbx_ensemble_clock", "nbx_ragged_clock")
ENTRY_POINTS = ADVANCE + CLOCK
NOUN = {"nbx": "ctx", "nbx_ensemble": "ensemble", "nbx_ragged": "ragged ensemble"}
HANDLE = {"nbx": "nbx_ctx", "nbx_ensemble": "nbx_ensemble", "nbx_ragged": "nbx_ragged"}
FORBIDDEN = ("hermite_step", "_jerk", "nbx_timescale", "nbx_field", "nbx_tidal", "tracers_", "_nlist", "_neighbours", "_clumps", "_fof",
             "_binaries", "_knn")


def _prefix(name):
    return name.rsplit("_", 1)[0]


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


ADV_ARGS = "double, double, int32_t, double, int32_t, int32_t"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_advance.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, %s) = nbx_advance; int (*b)(nbx_ensemble*, %s) = nbx_ensemble_advance; '
           'int (*c)(nbx_ragged*, %s) = nbx_ragged_advance; int (*d)(nbx_ctx*, nbx_clock_t*) = nbx_clock; '
           'int (*e)(nbx_ensemble*, int32_t, int32_t, nbx_clock_t*) = nbx_ensemble_clock; '
           'int (*f)(nbx_ragged*, int32_t, int32_t, nbx_clock_t*) = nbx_ragged_clock; nbx_clock_t k; k.done = 0; '
           'printf("%%d %%d %%d\\n", (int)sizeof(nbx_clock_t), (int)offsetof(nbx_clock_t, steps), (int)offsetof(nbx_clock_t, done)); '
           'return (a && b && c && d && e && f && !k.done) ? NBX_ABI_VERSION - 1 : 1; }\n' % (ADV_ARGS, ADV_ARGS, ADV_ARGS))
STUBS = '#include "nbx_advance.h"\n' + "".join(
    "int %s(%s* h, double t, double c, int32_t l, double e, int32_t m, int32_t r) { (void)h; (void)t; (void)c; (void)l; (void)e; (void)m; (void)r; return 0; }\n"
    % (f, HANDLE[_prefix(f)]) for f in ADVANCE) + (
    "int nbx_clock(nbx_ctx* h, nbx_clock_t* o) { (void)h; (void)o; return 0; }\n" + "".join(
        "int %s(%s* h, int32_t a, int32_t b, nbx_clock_t* o) { (void)h; (void)a; (void)b; (void)o; return 0; }\n" % (f, HANDLE[_prefix(f)])
        for f in CLOCK[1:]))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(nbx, tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "advance_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert out == "%d %d %d\n" % (ctypes.sizeof(nbx.Clock), nbx.Clock.steps.offset, nbx.Clock.done.offset) and ctypes.sizeof(nbx.Clock) == 56


def test_the_six_symbols_are_declared_exported_and_apart_from_every_other_header(nbx):
    declared = _declared("nbx_advance.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.ADVANCE_SYMBOLS) == ENTRY_POINTS
    for h in sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h != "nbx_advance.h"):
        assert not set(declared) & set(_declared(h)), h
        txt = open(os.path.join(ROOT, "include", h)).read()
        assert "_advance" not in txt and "nbx_clock" not in txt, h  # the other headers are as they were
    for t in (t for t in dir(nbx) if t.endswith("_SYMBOLS") and t != "ADVANCE_SYMBOLS"):
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (7 if s in ADVANCE else 2 if s == "nbx_clock" else 4)
    assert sorted(re.findall(r" T (nbx_\w*(?:advance|clock)\w*)$", out, flags=re.M)) == declared  # exactly six new exported symbols
    assert not [s for s in declared if "hermite" in s or "jerk" in s]
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()


def test_the_header_has_its_sections_its_formulas_and_its_not_here_items():
    raw = open(os.path.join(ROOT, "include", "nbx_advance.h")).read()
    assert re.findall(r'#include "(\w+\.h)"', raw) == ["nbx.h", "nbx_ensemble.h", "nbx_ragged.h"]
    for word in FORBIDDEN:
        assert word not in raw, word  # the other calls are referred to in words
    doc = re.sub(r"\n \*\s*", " ", raw)  # the comment as running text
    for word in ("Why:", "Definition:", "Arithmetic:", "Launch shape:", "Contracts:", "Semantics:", "State afterwards:",
                 "Status of the advance calls, in this order", "Deliberately not here:",
                 "d = a0 - a1", "a2 = (((-6 d) - h*((4 j0) + (2 j1))) * ih) * ih", "a3 = ((((12 d) + (6 h)*(j0 + j1)) * ih) * ih) * ih",
                 "a2 = a2 + h*a3", "|v|^2 = (vx*vx + vy*vy) + vz*vz", "s_i = (sqrt(A*S) + J) / (sqrt(J*C) + S)", "s_i = A / J where J > 0",
                 "a NaN candidate is never selected", "eta * sqrt(q)", "k_crit = floor(E / 2)", "k_floor = k_cap - levels",
                 "t * (0.5 * ih) == floor(t * (0.5 * ih))", "k6 = h * (1.0 / 6.0)", "h3 = h * (1.0 / 3.0)", "mul_rn / add_rn",
                 "exactly three launches", "no atomics", "26 packed VALU and 2 v_rsq_f32", "8 KiB in fp32 and 16 KiB in fp64", "no scratch",
                 "wave-uniform load", "one workgroup of 256 per system", "3 launches for the starting evaluation plus 3 * max_steps",
                 "done is computed and not stored", "lands on t_end exactly", "bit for bit", "never synchronise", "synchronise once",
                 "steps_done", "*_timed / *_ms_total", "cached graphs", "before the first HIP call", "power of two", "[0, 40]", "2^52",
                 "max_steps < 0", "2^22", "names the first such member", "nbx_commit", "resume cannot be honoured",
                 "max_steps == 0 and resume != 0", "NBX_ERR_ALLOC", "no advance call has been made"):
        assert word in doc, word
    not_here = doc[doc.index("Deliberately not here:"):]
    for item in ("a step per body (block steps", "P(EC)^n", "groups", "a member range", "tracers moving with the scheme", "hipGraph replay",
                 "a command-line word"):
        assert item in not_here, item
    order = [doc.index(w) for w in ("the handle is NULL", "t_end, dt_cap or eta is not finite", "dt_cap is not a power of two", "levels is outside",
                                    "t_end is not a whole multiple", "max_steps < 0", "exceed 2^22", "not uploaded;", "awaiting nbx_commit",
                                    "resume cannot be honoured", "max_steps == 0 and resume != 0", "the buffers did not fit")]
    assert order == sorted(order)


GOOD = dict(t_end=0.25, dt_cap=0.0625, levels=24, eta=0.125, max_steps=1, resume=0)


def _call(f, handle, **kw):
    a = dict(GOOD, **kw)
    return f(handle, a["t_end"], a["dt_cap"], a["levels"], a["eta"], a["max_steps"], a["resume"])


@pytest.mark.parametrize("name", ADVANCE)
def test_the_argument_checks_return_before_any_hip_call_in_the_headers_order(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no bodies and nothing uploaded.  Every case breaks the
    later checks too, so the text shows which came first."""
    L = nbx.load()
    f = getattr(L, name)
    err = lambda: L.nbx_last_error().decode()
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")
    # 1. the handle is NULL -- whatever else is wrong
    for kw in ({}, dict(t_end=nan, max_steps=-1), dict(dt_cap=0.3, levels=99)):
        assert _call(f, None, **kw) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[_prefix(name)])
    # 2. t_end, dt_cap, eta: finite and positive -- in this order, before everything else
    for bad in (nan, inf, -inf, 0.0, -1.0):
        assert _call(f, handle, t_end=bad, dt_cap=nan, eta=nan, levels=-1, max_steps=-1) == nbx.NBX_ERR_ARG
        assert err() == name + ": t_end is not finite or not positive"
        assert _call(f, handle, dt_cap=bad, eta=nan, levels=-1, max_steps=-1) == nbx.NBX_ERR_ARG
        assert err() == name + ": dt_cap is not finite or not positive"
        assert _call(f, handle, eta=bad, dt_cap=0.3, levels=-1, max_steps=-1) == nbx.NBX_ERR_ARG
        assert err() == name + ": eta is not finite or not positive"
    assert _call(f, handle, eta=1e-200) == nbx.NBX_ERR_ARG and err() == name + ": eta is not finite or not positive"  # eta * eta is 0
    # 3. dt_cap is a power of two (the zeroed object has no precision: the range is the double's)
    for bad in (0.3, 0.0625 * 3, 0.0625 * (1 + 2.0 ** -52), 5e-324, 2.0 ** -1023):
        assert _call(f, handle, dt_cap=bad, levels=-1, t_end=0.3, max_steps=-1) == nbx.NBX_ERR_ARG
        assert err() == name + ": dt_cap is not a power of two that is a normal value of the object's precision"
    # 4. levels
    for bad in (-1, 41, 1 << 30):
        assert _call(f, handle, levels=bad, t_end=0.3, max_steps=-1) == nbx.NBX_ERR_ARG
        assert err() == name + ": levels is outside [0, 40]"
    # 5. t_end is a whole multiple of dt_cap, and not more than 2^52 smallest steps away
    for kw in (dict(t_end=0.3), dict(t_end=0.0625 * 1.5), dict(t_end=0.03125), dict(t_end=2.0 ** 49, dt_cap=1.0, levels=4), dict(t_end=1e300, dt_cap=2.0 ** -1000)):
        assert _call(f, handle, max_steps=-1, **kw) == nbx.NBX_ERR_ARG
        assert err() == name + ": t_end is not a whole multiple of dt_cap, or more than 2^52 steps of the smallest size away"
    # 6. max_steps < 0 -- before the state and resume
    for resume in (0, 1):
        assert _call(f, handle, max_steps=-1, resume=resume) == nbx.NBX_ERR_ARG
        assert err() == name + ": max_steps < 0"
    assert _call(f, handle, t_end=2.0 ** 48, dt_cap=1.0, levels=4, max_steps=-1) == nbx.NBX_ERR_ARG and err() == name + ": max_steps < 0"  # 2^52 exactly
    if name == "nbx_advance":
        # 8. the zeroed context has not been uploaded -- also where nothing would be launched
        for max_steps, resume in ((0, 0), (1, 0), (0, 1)):
            assert _call(f, handle, max_steps=max_steps, resume=resume) == nbx.NBX_ERR_STATE
            assert err() == "nbx_advance: nbx_upload has not been called"
    else:
        # 10. the zeroed object has no members, hence none that is not uploaded: resume finds no previous advance call
        for max_steps in (0, 1):
            assert _call(f, handle, max_steps=max_steps, resume=1) == nbx.NBX_ERR_STATE
            assert err() == name + ": resume without a previous advance call on this object"
        assert _call(f, handle, max_steps=0, resume=0) == nbx.NBX_OK  # no member: nothing to evaluate
    assert zeroed.raw == bytes(1 << 16)


@pytest.mark.parametrize("name", CLOCK)
def test_the_clock_checks_return_before_any_hip_call(nbx, name):
    L = nbx.load()
    f = getattr(L, name)
    err = lambda: L.nbx_last_error().decode()
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    out = nbx.Clock()
    lead = () if name == "nbx_clock" else (0, 0)
    assert f(None, *lead, ctypes.byref(out)) == nbx.NBX_ERR_ARG and err() == "%s: %s is NULL" % (name, NOUN[_prefix(name)])
    assert f(handle, *lead, None) == nbx.NBX_ERR_ARG and err() == name + ": out is NULL"
    if name == "nbx_clock":
        out.struct_size = 8
        assert f(handle, ctypes.byref(out)) == nbx.NBX_ERR_ARG and err() == "nbx_clock: nbx_clock_t.struct_size does not match this library"
        out.struct_size = 0
        assert f(handle, ctypes.byref(out)) == nbx.NBX_ERR_STATE and err() == "nbx_clock: nbx_upload has not been called"
    else:
        assert f(handle, 0, 1, ctypes.byref(out)) == nbx.NBX_ERR_ARG and err() == name + ": members [first, first + count) are outside [0, members)"
        assert f(handle, 0, 0, ctypes.byref(out)) == nbx.NBX_ERR_STATE and err() == name + ": no advance call has been made on this object"
    assert zeroed.raw == bytes(1 << 16)


def test_the_checks_are_in_the_source_in_the_headers_order_and_only_the_clock_calls_copy_back_and_synchronise():
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kAdvanceMaxBodies = kFieldMaxPoints;" in hdr and "constexpr int kAdvanceMaxLevels = 40;" in hdr
    args = src[src.index("int check_arguments("):src.index("int batch_advance(")]
    order = [args.index(w) for w in ("positive(t_end)", "positive(dt_cap)", "positive(eta)", "not a power of two", "kAdvanceMaxLevels", "not a whole multiple",
                                     "max_steps < 0", "kAdvanceMaxBodies")]
    assert order == sorted(order)
    batch = src[src.index("int batch_advance("):src.index("bool size_ok(")]
    order = [batch.index(w) for w in ("is NULL", "check_arguments(", "check_uploaded(", "check_resume(", "max_steps == 0 && resume", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_advance("):src.index("int nbx_ensemble_advance(")]
    order = [ctx.index(w) for w in ("ctx is NULL", "check_arguments(", "->uploaded", "pending_commit", "c->i_begin != 0 || c->i_count != c->n",
                                    "check_resume(", "max_steps == 0 && resume", "use_device(")]
    assert order == sorted(order)
    resume = src[src.index("int check_resume("):src.index("int run_advance(")]
    order = [resume.index(w) for w in ("!o->adv_have", "o->herm_have", "o->adv_steps != o->steps_done || o->adv_cur != o->cur", "has_partials(o)",
                                       "o->adv_dt_cap != p.dt_cap || o->adv_levels != p.levels")]
    assert order == sorted(order)
    # the advance path -- everything before the clock calls' helpers -- neither copies back nor synchronises
    advance = src[:src.index("bool size_ok(")] + ctx
    assert "hipStreamSynchronize" not in advance and "hipDeviceSynchronize" not in advance and "DeviceToHost" not in advance
    assert "hipMemcpy" not in advance  # the one copy, of the ragged member table, is device_table's, from bytes that live with the object
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # which ragged_member_table reaches; the batch kinds' size-bound words are shared too
    assert "&r->herm_tab, &r->herm_tab_src" in advance and "device_table(" in shared and "device_table(" not in src
    assert '"members * n exceeds"' in shared and '"the bodies of the members exceed"' in shared
    assert "object_bodies(o) > kAdvanceMaxBodies" in args and "bodies_noun(o)" in args and '"n exceeds"' in src
    assert "timed_launch" not in src and "steps_done +=" not in src and "cur ^=" not in src
    assert "o->herm_have = false;" in advance
    # the clock path: one read-back and one synchronisation, in one helper every kind goes through
    assert src.count("hipStreamSynchronize") == 1 and src.count("DeviceToHost") == 1 and src.count("hipMemcpyAsync") == 1
    assert src.count("read_clocks(") == 3  # its definition, the batch kinds, the context
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == 5  # three kinds, one finish, one clock
    run = src[src.index("int run_advance("):src.index("int advance_t(")]
    assert len(re.findall(r"hipLaunchKernelGGL\(|launch\(PairLaunch", run)) == 3  # a step is three launches
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("adv_cand", "adv_clock"):
        assert re.search(r"void\* %s = nullptr;" % field, obj) and "o->%s" % field in obj[obj.index("inline void batch_release"):], field
    for field in ("double adv_dt_cap", "int adv_levels", "bool adv_have"):
        assert field in obj, field
    for f in ("nbx_hermite.hip", "nbx_hermite_kernels.hpp"):
        assert "adv_" not in open(os.path.join(CSRC, f)).read(), f  # the fixed stepper is as it was: it knows nothing of this call


def test_python_signatures_are_as_specified(nbx):
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.advance).parameters
        assert list(p) == ["self", "t_end", "dt_cap", "eta", "levels", "max_steps", "resume"], cls
        assert p["t_end"].default is inspect.Parameter.empty and p["dt_cap"].default is inspect.Parameter.empty, cls
        assert (p["eta"].default, p["levels"].default, p["max_steps"].default, p["resume"].default) == (0.125, 20, 32, False), cls
        assert hasattr(cls, "clock")
    assert not hasattr(nbx.Group, "advance") and not hasattr(nbx.Group, "clock")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "advance" in f]  # no new nbx_opts field
    assert [f for f, _ in nbx.Clock._fields_] == ["struct_size", "n", "t", "dt_last", "dt_next", "steps", "floor_steps", "done", "reserved"]
    assert "_advance_stale = True" in inspect.getsource(nbx._remember_mass)  # the upload hook, next to the fixed stepper's


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_advance\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_advance\.o: \$\(CSRC\)/nbx_advance\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    other = re.search(r"^\$\(PKG\)/nbx_jerk\.o: \$\(CSRC\)/nbx_jerk\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == other.group(1).replace("jerk", "advance")  # the same dependency list
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_advance.hip", "include/nbx_advance.h"):
        assert word in sh, word
    for f in sorted(os.listdir(CSRC)):
        text = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_advance.hip":
            assert KERNELS not in text, f  # nobody else includes the kernels
        if f in ("nbx_advance.hip", KERNELS):
            assert [k for k in re.findall(r"\w+_kernels\.hpp", text) if k != KERNELS] == [], f  # and they include nobody else's
    kern = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "field_shape(" in kern and '#include "nbx_field_shape.hpp"' in kern  # the shape rule of the fixed stepper, no new one
    assert "atomic" not in kern and "__shared__ T4 ptile[kTile];" in kern and "__shared__ T4 vtile[kTile];" in kern
    assert kern.count("velm[i]") == 1 and "if (i < n) {\n      v = velm[i];" in kern  # velocities and kept records only below n


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the translation unit
# ---------------------------------------------------------------------------------------------------------------------------
def _shipped_hipflags():
    """The flags libnbx.so is built with (top-level Makefile, HIPFLAGS): the audited code must be the executed code."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{kernel symbol: (code, kernel descriptor, metadata entry)}"""
    out = tmp_path_factory.mktemp("isa") / "nbx_advance.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair kernel, ("finish", precision) of a finish kernel, ("clock", 64) of the clock kernel."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)advance_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+advance_finish_kernelI([fd])EE", name)
    if m:
        return ("finish", 32 if m.group(1) == "f" else 64)
    return ("clock", 64) if re.search(r"^_ZN3nbx\d+advance_clock_kernelE", name) else None


def _pair_loops(body, ins):
    """The innermost loop bodies (label ... backward branch) that hold `ins`."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_every_kind_and_precision_is_compiled_both_finish_kernels_and_the_clock_kernel(isa):
    keys = sorted((_key(k) or ("?", k) for k in isa), key=str)
    want = [(kind, p) for kind in ("context", "ensemble", "ragged", "finish") for p in (32, 64)] + [("clock", 64)]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_no_atomics_and_lds_is_exactly_the_two_tiles_in_the_pair_kernels(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        assert not re.search(r"atomic|\bds_(?:add|min|max|cmpst|wrxchg)_", body), name
        kind, precision = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        want = {"finish": 0, "clock": 256 * 8}.get(kind, 2 * 256 * (16 if precision == 32 else 32))  # 8 KiB, 16 KiB; the clock: 256 minima
        assert lds == want, (name, lds)


def test_the_pair_loops_are_the_fixed_steppers_and_the_clock_record_is_read_by_scalar_loads(isa):
    """Per j record, relative to the 16-byte LDS reads (two per fp32 record): 6 packed adds, 14 packed fma, 6 packed multiplies,
    2 v_rsq_f32 and nothing unpacked, no fp64; fp64, per seed: 19 fma, 7 multiplies, 6 adds -- the counts tests/test_hermite_cpu.py
    states for the fixed stepper.  The fp64 predictor exists in the fp32 kernels and none of it is in the pair loop."""
    for name, (body, desc, meta) in isa.items():
        kind, precision = _key(name)
        c = lambda ins, text=body: len(re.findall(r"\b%s" % ins, text))
        if kind == "clock":
            assert c("v_rsq_") + c("v_sqrt") + c("v_div_") + c("v_rcp_") == 0, name  # the quantiser: integers, exact products, no root, no division
            continue
        if kind == "finish":
            assert c("v_fma_f64") + c("v_fmac_f64") > 0 and c("v_div_scale_f64") >= 1, name  # the root's and the quotient's expansions alone fuse
            assert c("v_mul_f64") >= 6 + 30 and c("v_add_f64") >= 12 + 20, name  # the corrector and the criterion, unfused
            continue
        if precision == 64:
            loops = _pair_loops(body, "v_rsq_f64")
            assert len(loops) == 1, (name, len(loops))
            pairs = c("v_rsq_f64", loops[0])  # one seed per pair; a record serves the lane's two bodies
            assert pairs >= 2 and pairs % 2 == 0, (name, pairs)
            got = (c("v_fma_f64", loops[0]) + c("v_fmac_f64", loops[0]), c("v_mul_f64", loops[0]), c("v_add_f64", loops[0]))
            assert got == (19 * pairs, 7 * pairs, 6 * pairs), (name, pairs, got)
        else:
            loops = _pair_loops(body, "v_pk_fma_f32")
            assert len(loops) == 1, (name, len(loops))  # nothing is masked: one loop
            loop = loops[0]
            reads = c(r"ds_(?:read|load)_b128", loop)
            assert reads >= 2 and reads % 2 == 0 and c(r"ds_(?:read|load)_b(?:32|64|96)\b", loop) == 0, (name, reads)  # whole records only
            records = reads // 2
            got = (c("v_pk_add_f32", loop), c("v_pk_fma_f32", loop), c("v_pk_mul_f32", loop), c("v_rsq_f32", loop))
            assert got == (6 * records, 14 * records, 6 * records, 2 * records), (name, records, got)
            assert sum(got[:3]) == 26 * records
            assert c(r"v_(?:add|sub|subrev|mul|fma|fmac|mad|mac)_f32", loop) == 0, name  # nothing unpacked
            assert c(r"v_\w+_f64", loop) == 0, name  # no fp64 inside the fp32 pair loop
            assert c("v_mul_f64") >= 5 and c("v_add_f64") >= 5 and c("v_fma_f64") + c("v_fmac_f64") == 0, name  # the predictor, unfused
        assert c(r"s_load_dword(?:x\d+)?\b") >= 2 and c("v_sqrt") == 0, name  # the arguments and the clock record: wave-uniform


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement on its own
# ---------------------------------------------------------------------------------------------------------------------------
K_CAP, LEVELS = -4, 24


def _check_history(r, t_end, k_cap, levels):
    """t / h is an integer before every step, h at most doubles, h stays within its range, the times add up."""
    t, last = 0.0, None
    for t0, h, _ in r["history"]:
        assert t0 == t and (t0 / h) == np.floor(t0 / h), (t0, h)
        assert 2.0 ** (k_cap - levels) <= h <= 2.0 ** k_cap and np.frexp(h)[0] == 0.5, h
        assert last is None or h <= 2.0 * last, (last, h)
        t, last = t0 + h, h
    assert r["clock"]["t"] == t and r["clock"]["steps"] == len(r["history"]) and t <= t_end


_runs = {}


def _smooth(seed, eta, fault=None):
    """jerk_ref's 96-body system `seed` to T = 0.25, dt_cap = 2^-4, in fp64."""
    key = (seed, eta, fault)
    if key not in _runs:
        _runs[key] = A.run(R.hermite_state(seed), 64, R.HERMITE_T, K_CAP, LEVELS, eta, 100000, R.direct, fault=fault)
    return _runs[key]


def _small(precision, n, family, max_steps=12, fault=None, eta=0.125):
    return A.run(R.make_state(precision, n, family), precision, 2.0 ** K_CAP, K_CAP, LEVELS, eta, max_steps, R.direct, fault=fault)


def test_every_history_keeps_t_a_multiple_of_h_lets_h_at_most_double_and_lands_on_t_end():
    for seed in R.HERMITE_SEEDS:
        for eta in (0.25, 0.125, 0.0625):
            r = _smooth(seed, eta)
            _check_history(r, R.HERMITE_T, K_CAP, LEVELS)
            assert r["clock"]["t"] == R.HERMITE_T and A.public(r["clock"], R.HERMITE_T)["done"]
            print("seed %d eta %g: %d steps, sizes 2^%d .. 2^%d" % (seed, eta, len(r["history"]), A.exponent(min(h for _, h, _ in r["history"])),
                                                                  A.exponent(max(h for _, h, _ in r["history"]))))
    for precision in (32, 64):
        for n, family in ((2, "cloud"), (5, "cloud"), (33, "clustered")):
            r = _small(precision, n, family, max_steps=100000)
            _check_history(r, 2.0 ** K_CAP, K_CAP, LEVELS)
            assert r["clock"]["t"] == 2.0 ** K_CAP, (precision, n, family)
            part = _small(precision, n, family, max_steps=5)  # a run cut short and carried on is the run
            _check_history(part, 2.0 ** K_CAP, K_CAP, LEVELS)
            rest = A.run(part["state"], precision, 2.0 ** K_CAP, K_CAP, LEVELS, 0.125, 100000, R.direct, clock=part["clock"], carry=part["carry"])
            assert H.same(rest["state"], r["state"]) and rest["clock"] == r["clock"] and part["history"] + rest["history"] == r["history"]
    # one body: no acceleration, no criterion -- the cap, at once
    r = _small(64, 1, "cloud")
    assert [h for _, h, _ in r["history"]] == [2.0 ** K_CAP] and r["clock"]["floor_steps"] == 0
    # a floor that binds: every step at the floor counts, and the clock still lands on t_end
    r = A.run(R.make_state(64, 5, "cloud"), 64, 2.0 ** K_CAP, K_CAP, 2, 0.125, 100000, R.direct)
    assert [h for _, h, _ in r["history"]] == [2.0 ** (K_CAP - 2)] * 4 and r["clock"]["t"] == 2.0 ** K_CAP
    asked_less = sum(A.k_crit(x, 1.0) < K_CAP - 2 for _, _, x in r["history"][:-1])  # what each step but the last left for the next one
    assert asked_less >= 1 and r["clock"]["floor_steps"] in (asked_less, asked_less + 1)  # + 1: the first step, chosen at the start


def test_the_quantiser_takes_the_largest_power_of_two_whose_square_fits_and_never_a_nan():
    for x in (1.0, 3.999, 4.0, 4.001, 0.25, 0.2499, 2.0 ** -31, 2.0 ** -30, 1.5 * 2.0 ** -31, 1e-300, 1e300):
        k = A.k_crit(x, 1.0)
        assert (2.0 ** k) ** 2 <= x < (2.0 ** (k + 1)) ** 2, (x, k)
    assert A.k_crit(np.inf, 1.0) == 512 and A.k_crit(0.0, 1.0) == -512
    assert A.choose(np.inf, 1.0, -4, 24) == (-4, False) and A.choose(0.0, 1.0, -4, 24) == (-28, True)
    assert A.minimum([np.nan, 3.0, np.nan, 2.0]) == 2.0 and A.minimum([np.nan]) == np.inf and A.minimum([]) == np.inf
    # after a step of 2^-6 that ends at t = 3 * 2^-6, a criterion that allows 2^-3 keeps 2^-6; at t = 4 * 2^-6 it doubles, once
    assert A.choose(2.0 ** -6, 1.0, -2, 24, k=-6, t=3 * 2.0 ** -6) == (-6, False)
    assert A.choose(2.0 ** -6, 1.0, -2, 24, k=-6, t=4 * 2.0 ** -6) == (-5, False)
    assert A.choose(2.0 ** -12, 1.0, -2, 24, k=-6, t=4 * 2.0 ** -6) == (-6, False)  # k_crit == k: stay
    assert A.choose(2.0 ** -20, 1.0, -2, 24, k=-6, t=4 * 2.0 ** -6) == (-10, False)  # shrink at once, by any factor
    assert A.boundary_distance(4.0) == 0.0 and A.boundary_distance(1.0) == 0.0 and abs(A.boundary_distance(0.25 * (1 + 1e-6)) - 1e-6) < 1e-12
    assert abs(A.boundary_distance(16.0 * (1 - 1e-6)) - 1e-6) < 1e-12 and A.boundary_distance(2.0) == 0.5


def _orbit():
    """Two bodies of G m = 1 each, semi-major axis 1, eccentricity 0.9, at apocentre, in the centre-of-mass frame."""
    e, a, gm = 0.9, 1.0, 2.0
    r = a * (1.0 + e)
    v = np.sqrt(gm * (2.0 / r - 1.0 / a))
    z = np.zeros(2)
    m = np.full(2, 1.0 / float(G32))
    s = dict(pos_x=np.array([-r / 2, r / 2]), pos_y=z, pos_z=z, vel_x=z, vel_y=np.array([-v / 2, v / 2]), vel_z=z, mass=m)
    return {k: np.ascontiguousarray(x, dtype=np.float64) for k, x in s.items()}


def test_on_an_eccentric_orbit_the_adaptive_run_beats_a_fixed_step_of_the_same_cost_a_hundredfold():
    """fp64, t_end = 4, dt_cap = 2^-2, eta = 0.25, against a fixed run of 65536 steps; the fixed run of the comparison takes as many
    steps as the adaptive one took.  The prototype of the issue saw 132 steps of 2^-9 .. 2^-2 and errors of 8.0e-5 and 2.76."""
    s0, t_end = _orbit(), 4.0
    r = A.run(s0, 64, t_end, -2, 20, 0.25, 100000, R.direct)
    _check_history(r, t_end, -2, 20)
    steps = len(r["history"])
    sizes = sorted({A.exponent(h) for _, h, _ in r["history"]})
    ref = H.steps(s0, t_end / 65536, 65536, 64, R.direct)[0]
    fixed = H.steps(s0, t_end / steps, steps, 64, R.direct)[0]
    e_adaptive, e_fixed = R.state_error(r["state"], ref), R.state_error(fixed, ref)
    print("eccentric orbit: %d steps of 2^%d .. 2^%d, adaptive error %.3g, fixed-step error %.3g, ratio %.3g" % (
        steps, sizes[0], sizes[-1], e_adaptive, e_fixed, e_fixed / e_adaptive))
    assert r["clock"]["t"] == t_end and r["clock"]["floor_steps"] == 0
    assert len(sizes) >= 4  # the step follows the orbit
    assert e_adaptive <= e_fixed / 100.0, (e_adaptive, e_fixed)


def test_eta_is_an_accuracy_knob_on_the_smooth_systems():
    """The 96-body systems to T = 0.25: the error against the fixed run of 256 steps falls with eta, and stays within a factor of 4
    of the fixed run of the same number of steps (the prototype: about 2)."""
    for seed in R.HERMITE_SEEDS:
        s0 = R.hermite_state(seed)
        ref = H.steps(s0, R.HERMITE_T / 4096, 4096, 64, R.direct)[0]
        errs = []
        for eta in (0.25, 0.125, 0.0625):
            r = _smooth(seed, eta)
            steps = len(r["history"])
            fixed = H.steps(s0, R.HERMITE_T / steps, steps, 64, R.direct)[0]
            e, ef = R.state_error(r["state"], ref), R.state_error(fixed, ref)
            print("seed %d eta %g: %d steps, adaptive error %.3g, fixed-step error %.3g" % (seed, eta, steps, e, ef))
            errs.append(e)
            assert e <= 4.0 * ef, (seed, eta, e, ef)
        assert errs[0] > errs[1] > errs[2], (seed, errs)


def test_every_planted_fault_changes_a_history_or_an_end_state():
    assert len(A.FAULTS) >= 6 and len(set(A.FAULTS)) == len(A.FAULTS)
    cases = [("smooth %d" % seed, lambda f, seed=seed: _smooth(seed, 0.125, fault=f)) for seed in R.HERMITE_SEEDS]
    cases += [("%d %s fp%d" % (n, fam, p), lambda f, n=n, fam=fam, p=p: _small(p, n, fam, fault=f)) for p in (32, 64)
              for n, fam in ((5, "cloud"), (33, "clustered"), (257, "clustered"))]
    caught = {f: [] for f in A.FAULTS}
    for name, run in cases:
        good = run(None)
        again = run(None)
        assert H.same(good["state"], again["state"]) and good["history"] == again["history"], name
        for fault in A.FAULTS:
            bad = run(fault)
            hist = [h for _, h, _ in bad["history"]] != [h for _, h, _ in good["history"]]
            end = not H.same(bad["state"], good["state"])
            if hist or end:
                caught[fault].append(name)
            print("%-18s %-44s: %s%s" % (name, fault, "history changes" if hist else "same history", ", end state changes" if end else ""))
    assert all(caught.values()), caught
