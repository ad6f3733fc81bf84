"""The resident fourth-order Hermite stepper (include/nbx_hermite.h), the parts that need no GPU: the header and its three exported
symbols, the argument checks that come before the first HIP call, the Python methods, the build files, an audit of the
cross-compiled gfx950 code of nbx_hermite.hip, and the numpy restatement tests/hermite_ref.py, which must show by itself what the
device tests then ask of the library: that the scheme of the header is of fourth order on jerk_ref's two 96-body states, and that
every planted fault either costs it that order or changes bits against the unfaulted restatement."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_ref as H
import jerk_ref as R
from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_hermite.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_hermite_kernels.hpp"
ENTRY_POINTS = ("nbx_hermite_step", "nbx_ensemble_hermite_step", "nbx_ragged_hermite_step")
NOUN = {"nbx_hermite_step": "ctx", "nbx_ensemble_hermite_step": "ensemble", "nbx_ragged_hermite_step": "ragged ensemble"}
HANDLE = {"nbx_hermite_step": "nbx_ctx", "nbx_ensemble_hermite_step": "nbx_ensemble", "nbx_ragged_hermite_step": "nbx_ragged"}


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_hermite.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, double, int32_t, int32_t) = nbx_hermite_step; '
           'int (*b)(nbx_ensemble*, double, int32_t, int32_t) = nbx_ensemble_hermite_step; '
           'int (*c)(nbx_ragged*, double, int32_t, int32_t) = nbx_ragged_hermite_step; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')
STUBS = '#include "nbx_hermite.h"\n' + "".join(
    "int %s(%s* h, double dt, int32_t n, int32_t r) { (void)h; (void)dt; (void)n; (void)r; return 0; }\n" % (f, HANDLE[f]) for f in ENTRY_POINTS)


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "hermite_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_the_three_symbols_are_declared_exported_and_apart_from_every_other_header(nbx):
    declared = _declared("nbx_hermite.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.HERMITE_SYMBOLS) == ENTRY_POINTS
    for h in sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h != "nbx_hermite.h"):
        assert not set(declared) & set(_declared(h)), h
        assert "hermite_step" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in (t for t in dir(nbx) if t.endswith("_SYMBOLS") and t != "HERMITE_SYMBOLS"):
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == 4
    assert sorted(re.findall(r" T (nbx_\w*hermite\w*)$", out, flags=re.M)) == declared  # exactly three new exported symbols
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()


def test_the_header_has_its_sections_its_formulas_and_its_not_here_items():
    raw = open(os.path.join(ROOT, "include", "nbx_hermite.h")).read()
    doc = re.sub(r"\n \*\s*", " ", raw)  # the comment as running text
    for word in ("Why:", "Definition:", "Arithmetic:", "Starting values and resume:", "Launch shape:", "Contracts:", "Semantics:",
                 "State afterwards:", "Status, in this order", "Deliberately not here:",
                 "vp = v + h*(a0 + k2*j0)", "xp = x + h*(v + k2*(a0 + h3*j0))", "v1 = v + k2*((a0 + a1) + k6*(j0 - j1))",
                 "x1 = x + k2*((v + v1) + k6*(a0 - a1))", "k2 = h * 0.5", "k6 = h / 6.0", "h3 = h / 3.0", "mul_rn / add_rn",
                 "The unrounded fp64 v1 enters the formula for x1", "rounded once to T", "P(EC)", "no second one",
                 "exactly two launches", "only where j < n", "nothing is masked", "No predicted state is ever written to memory",
                 "26 packed VALU and 2 v_rsq_f32", "8 KiB in fp32 and 16 KiB in fp64", "no scratch", ".w (gm) untouched",
                 ".w (the mass) untouched", "2 + 2 * nsteps", "2 * nsteps", "No atomics", "bit for bit", "never synchronises",
                 "steps_done", "*_timed / *_ms_total", "cached graphs", "tracers do not move", "analysis call's scratch",
                 "reports 0", "an upload of the downloaded state", "before the first HIP call", "dt is not finite", "nsteps < 0", "2^22",
                 "names the first such member", "nbx_commit", "does not own all n bodies", "resume cannot be honoured",
                 "nsteps == 0", "NBX_ERR_ALLOC"):
        assert word in doc, word
    not_here = doc[doc.index("Deliberately not here:"):]
    for item in ("groups", "a member range", "a time step per member or per body (block steps)", "kenergy_out", "P(EC)^n",
                 "tracers moving with the scheme", "hipGraph replay", "a command-line word"):
        assert item in not_here, item
    order = [doc.index(w) for w in ("the handle is NULL", "dt is not finite", "nsteps < 0", "exceed 2^22", "not uploaded;",
                                    "awaiting nbx_commit", "does not own all n bodies", "resume cannot be honoured", "nsteps == 0:",
                                    "the buffers did not fit")]
    assert order == sorted(order)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_the_null_dt_and_nsteps_checks_return_before_any_hip_call(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no bodies and nothing uploaded."""
    L = nbx.load()
    f = getattr(L, name)
    err = lambda: L.nbx_last_error().decode()
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for dt, nsteps, resume in ((0.01, 1, 0), (float("nan"), -1, 1), (float("inf"), 0, 0)):
        assert f(None, dt, nsteps, resume) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. dt is not finite -- before nsteps and the state
    for dt in (float("nan"), float("inf"), -float("inf")):
        for nsteps, resume in ((1, 0), (-1, 1), (0, 0)):
            assert f(handle, dt, nsteps, resume) == nbx.NBX_ERR_ARG
            assert err() == name + ": dt is not finite"
    # 3. nsteps < 0 -- before the state and resume
    for resume in (0, 1):
        assert f(handle, 0.01, -1, resume) == nbx.NBX_ERR_ARG
        assert err() == name + ": nsteps < 0"
    if name == "nbx_hermite_step":
        # 5. the zeroed context has not been uploaded -- also where nothing would be launched
        for nsteps in (0, 1):
            assert f(handle, 0.01, nsteps, 0) == nbx.NBX_ERR_STATE
            assert err() == "nbx_hermite_step: nbx_upload has not been called"
    else:
        # 8. the zeroed object has no members, hence none that is not uploaded: resume finds no previous Hermite call
        assert f(handle, 0.01, 0, 1) == nbx.NBX_ERR_STATE
        assert err() == name + ": resume without a previous Hermite call on this object"
        # 9. nsteps == 0: NBX_OK, nothing launched
        assert f(handle, 0.01, 0, 0) == nbx.NBX_OK
    assert zeroed.raw == bytes(1 << 16)


def test_the_checks_are_in_the_source_in_the_headers_order_and_the_call_neither_copies_back_nor_synchronises():
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kHermiteMaxBodies = kFieldMaxPoints;" in hdr
    batch = src[src.index("int batch_hermite("):src.index('extern "C"')]
    order = [batch.index(w) for w in ("is NULL", "dt is not finite", "nsteps < 0", "kHermiteMaxBodies", "check_uploaded(", "check_resume(",
                                      "nsteps == 0", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_hermite_step("):]
    order = [ctx.index(w) for w in ("ctx is NULL", "dt is not finite", "nsteps < 0", "kHermiteMaxBodies", "->uploaded", "pending_commit",
                                    "c->i_begin != 0 || c->i_count != c->n", "check_resume(", "nsteps == 0", "use_device(")]
    assert order == sorted(order)
    assert "hipStreamSynchronize" not in src and "hipDeviceSynchronize" not in src and "DeviceToHost" not in src
    assert "hipMemcpy" not in src  # the one copy, of the ragged member table, is device_table's, from bytes that live with the object
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # which ragged_member_table reaches; the size bound's words are shared too
    assert "&r->herm_tab, &r->herm_tab_src" in src and "device_table(" in shared and "device_table(" not in src
    assert '"members * n exceeds"' in shared and '"the bodies of the members exceed"' in shared
    assert "object_bodies(o) > kHermiteMaxBodies" in src and "bodies_noun(o)" in src and '"nbx_hermite_step: n exceeds 4194304"' in src
    assert "timed_launch" not in src and "steps_done +=" not in src and "cur ^=" not in src
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == 4  # three kinds, one finish
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("herm_part", "herm_keep", "herm_tab"):
        assert re.search(r"void\* %s = nullptr;" % field, obj) and "o->%s" % field in obj[obj.index("inline void batch_release"):], field


def test_python_signatures_are_as_specified_and_hermite_stays_as_it_is(nbx):
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.hermite_step).parameters
        assert list(p) == ["self", "dt", "nsteps", "resume"], cls
        assert p["dt"].default is inspect.Parameter.empty and p["nsteps"].default == 1 and p["resume"].default is False, cls
    assert not hasattr(nbx.Group, "hermite_step")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "hermite" in f]  # no new nbx_opts field
    assert list(inspect.signature(nbx.hermite).parameters) == ["obj", "dt", "nsteps"]
    assert "what a device-resident stepper would not" in " ".join(nbx.hermite.__doc__.split())


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_hermite\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_hermite\.o: \$\(CSRC\)/nbx_hermite\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    other = re.search(r"^\$\(PKG\)/nbx_jerk\.o: \$\(CSRC\)/nbx_jerk\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == other.group(1).replace("jerk", "hermite")  # the same dependency list
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_hermite.hip", "include/nbx_hermite.h"):
        assert word in sh, word
    for f in sorted(os.listdir(CSRC)):
        if f != "nbx_hermite.hip":
            assert KERNELS not in re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read()), f  # nobody else includes the kernels
    kern = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "field_shape(" in kern and '#include "nbx_field_shape.hpp"' in kern  # the shape rule of the jerk call, no new one
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
    out = tmp_path_factory.mktemp("isa") / "nbx_hermite.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair-work kernel, ("finish", precision) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)hermite_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+hermite_finish_kernelI([fd])EE", name)
    return ("finish", 32 if m.group(1) == "f" else 64) if m else None


def _pair_loops(body, ins):
    """The innermost loop bodies (label ... backward branch) that hold `ins`."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_every_kind_and_precision_is_compiled_and_the_finish(isa):
    keys = sorted((_key(k) or ("?", k) for k in isa), key=str)
    assert keys == sorted([(kind, p) for kind in ("context", "ensemble", "ragged", "finish") for p in (32, 64)], key=str), keys


def test_no_scratch_no_spills_and_lds_is_exactly_the_two_tiles(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        kind, precision = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (0 if kind == "finish" else 2 * 256 * (16 if precision == 32 else 32)), (name, lds)  # 8 KiB, 16 KiB


def test_the_pair_loops_are_the_jerk_calls_and_the_predictor_sits_outside_them(isa):
    """Per j record, relative to the 16-byte LDS reads (two per fp32 record): the counts tests/test_jerk_cpu.py states for the
    jerk call -- 6 packed adds, 14 packed fma, 6 packed multiplies, 2 v_rsq_f32 and nothing unpacked; fp64, per seed: 19 fma, 7
    multiplies, 6 adds.  The fp64 predictor exists in the fp32 kernels (v_mul_f64, v_add_f64) and none of it is in the pair loop."""
    for name, (body, desc, meta) in isa.items():
        kind, precision = _key(name)
        c = lambda ins, text=body: len(re.findall(r"\b%s" % ins, text))
        assert c(r"(?:global|flat|ds|buffer)_atomic") + c(r"ds_(?:add|min|max)_") == 0, name
        assert c("v_sqrt") == 0, name
        if kind == "finish":
            assert c("v_rsq_") == 0 and c("v_fma_f64") + c("v_fmac_f64") == 0, name  # the corrector: multiplies and adds, none fused
            assert c("v_mul_f64") >= 6 and c("v_add_f64") >= 12, name
            continue
        if precision == 64:
            loops = _pair_loops(body, "v_rsq_f64")
            assert len(loops) == 1, (name, len(loops))
            pairs = c("v_rsq_f64", loops[0])  # one seed per pair; a record serves the lane's two bodies
            assert pairs >= 2 and pairs % 2 == 0, (name, pairs)
            got = (c("v_fma_f64", loops[0]) + c("v_fmac_f64", loops[0]), c("v_mul_f64", loops[0]), c("v_add_f64", loops[0]))
            assert got == (19 * pairs, 7 * pairs, 6 * pairs), (name, pairs, got)
            continue
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


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _run(state, steps, precision=64, fault=None):
    return H.steps(state, R.HERMITE_T / steps, steps, precision, R.direct, fault=fault)[0]


def test_the_numpy_scheme_is_of_fourth_order_and_every_planted_fault_costs_the_order_or_changes_bits():
    """jerk_ref's two 96-body states, T = 0.25 in 16 and in 32 steps, both measured against the unfaulted run of 256 steps
    (dt / 16): a fourth-order scheme gains 16 per halving and a second-order one 4; 8, their geometric mean, is the gate of the
    device tests.  A planted fault either drops the ratio below 8 or -- "v1 is rounded to T before x1" is the identity in fp64, and
    a fault may leave an error that still shrinks fast -- changes the bits of four fp32 steps against the unfaulted restatement,
    which is what the device tests compare.  The table printed shows which."""
    assert len(H.FAULTS) >= 6 and len(set(H.FAULTS)) == len(H.FAULTS)
    n1 = R.HERMITE_STEPS
    caught = {f: set() for f in H.FAULTS}
    for seed in R.HERMITE_SEEDS:
        s0 = R.hermite_state(seed)
        ref = _run(s0, 16 * n1)
        e1, e2 = R.state_error(_run(s0, n1), ref), R.state_error(_run(s0, 2 * n1), ref)
        print("seed %d: errors %.3g %.3g ratio %.1f" % (seed, e1, e2, e1 / e2))
        assert e1 / e2 >= 8.0, (seed, e1, e2)
        # the restatement is jerk_ref.hermite's scheme: the two differ by rounding, orders below the scheme's own error
        assert R.state_error(_run(s0, n1), R.hermite(s0, R.HERMITE_T / n1, n1)) <= 1e-6 * e1
        # The bits: fp32, four steps of T / 4.  Rounding v1 early moves x1 by k2 u |v|, which flips a bit of x1 in about one
        # component in 1 / (2 k2) where |v| ~ |x|: k2 = 1 / 32 and 96 * 3 * 4 component-steps make some twenty flips likely, where
        # T / 16 would leave about five.
        s32 = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in s0.items()}
        dt, nbits = R.HERMITE_T / 4, 4
        good = H.steps(s32, dt, nbits, 32, R.direct)[0]
        assert H.same(good, H.steps(s32, dt, nbits, 32, R.direct)[0]) and good["pos_x"].dtype == np.float32
        for fault in H.FAULTS:
            f1, f2 = R.state_error(_run(s0, n1, fault=fault), ref), R.state_error(_run(s0, 2 * n1, fault=fault), ref)
            bits = not H.same(good, H.steps(s32, dt, nbits, 32, R.direct, fault=fault)[0])
            order = f1 / f2 < 8.0
            print("seed %d %-34s: errors %.3g %.3g ratio %5.1f -> %s%s" % (seed, fault, f1, f2, f1 / f2, "order lost" if order else "order kept",
                                                                           ", bits change" if bits else ", same bits"))
            assert order or bits, (seed, fault)
            caught[fault].update((["order"] if order else []) + (["bits"] if bits else []))
    assert all(caught.values()), caught


def test_a_carried_call_continues_the_steps_and_a_fresh_evaluation_does_not():
    """steps(3) then steps(2, carry) is steps(5) bit for bit; without the carry the second call evaluates at the corrected state,
    a different quantity from (a1, j1) at the predicted one -- what `resume` is about."""
    for precision in (32, 64):
        s0 = {k: np.ascontiguousarray(v.astype(R.DTYPE[precision])) for k, v in R.hermite_state().items()}
        dt = R.HERMITE_T / R.HERMITE_STEPS
        five, kept5 = H.steps(s0, dt, 5, precision, R.direct)
        three, kept = H.steps(s0, dt, 3, precision, R.direct)
        carried, kept2 = H.steps(three, dt, 2, precision, R.direct, carry=kept)
        assert H.same(carried, five) and all(np.array_equal(a, b) for a, b in zip(kept2, kept5)), precision
        assert not H.same(H.steps(three, dt, 2, precision, R.direct)[0], five), precision
        assert H.consts(dt, precision)[0] == float(R.DTYPE[precision](dt))
