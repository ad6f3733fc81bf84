"""Velocity-only half steps (include/nbx_kick.h), the parts that need no GPU: the header and its four exported symbols, the
argument checks that come before the first HIP call, the Python methods, the build files, an audit of the cross-compiled gfx950
code of nbx_kick.hip, and the numpy restatement tests/kick_ref.py, which must show by itself what the device tests then ask of the
library on the same systems: plain stepping is first order in the energy it reads out, the two half kicks make it second order and
time reversible."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import kick_ref as K
from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_kick.hip")
DRIVER = os.path.join(ROOT, "tests", "ragged_accel_plan_driver.cpp")  # its "instances" mode prints kEnsembleInstances
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h")
ENTRY_POINTS = ("nbx_kick", "nbx_ensemble_kick", "nbx_ragged_kick", "nbx_group_kick")
NULL_TEXT = {"nbx_kick": "ctx is NULL", "nbx_ensemble_kick": "ensemble is NULL", "nbx_ragged_kick": "ragged ensemble is NULL",
             "nbx_group_kick": "group is NULL"}


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_kick.h"\n'
           'int main(void) { nbx_ensemble_stats_t es; nbx_ragged_stats_t rs; nbx_stats_t cs; '
           'int (*a)(nbx_ctx*, double, double*) = nbx_kick; '
           'int (*b)(nbx_ensemble*, double, double*) = nbx_ensemble_kick; '
           'int (*c)(nbx_ragged*, double, double*) = nbx_ragged_kick; '
           'int (*d)(nbx_group*, double, double*) = nbx_group_kick; '
           'printf("%d %d %d\\n", (int)sizeof es, (int)sizeof rs, (int)sizeof cs); '
           'return (a != NULL && b != NULL && c != NULL && d != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_and_brings_its_parents(tmp_path, compiler, std, ext):
    src = tmp_path / ("kick." + ext)
    src.write_text(PROGRAM)
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "kick.o")])


def test_declared_set_is_the_four_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_kick.h")
    assert declared == sorted(ENTRY_POINTS) and set(declared) == set(nbx.KICK_SYMBOLS) and len(nbx.KICK_SYMBOLS) == 4
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS) |
                                set(nbx.RAGGED_SYMBOLS) | set(nbx.RAGGED_DIAG_SYMBOLS) | set(nbx.BATCH_ACCEL_SYMBOLS))
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == 3
    assert L.nbx_abi_version() == 1


def test_the_parent_headers_declare_what_they_declared_and_point_here_in_a_comment_only(nbx):
    assert len(_declared("nbx_ensemble.h")) == 9 and set(_declared("nbx_ensemble.h")) == set(nbx.ENSEMBLE_SYMBOLS)
    assert len(_declared("nbx_ragged.h")) == 9 and set(_declared("nbx_ragged.h")) == set(nbx.RAGGED_SYMBOLS)
    assert set(_declared("nbx.h")) == set(nbx.SYMBOLS)
    assert set(_declared("nbx_batch_accel.h")) == set(nbx.BATCH_ACCEL_SYMBOLS)
    for h in ("nbx.h", "nbx_ensemble.h", "nbx_ragged.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        assert txt.count("nbx_kick.h") == 1, h
        assert "nbx_kick" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S), h  # no new include or symbol
    hdr = open(os.path.join(ROOT, "include", "nbx.h")).read()
    assert "#define NBX_ABI_VERSION 1" in hdr
    at = hdr.index("does not retrace a forward step")
    assert "nbx_kick.h" in hdr[at:at + 120]  # next to that sentence
    doc = open(os.path.join(ROOT, "include", "nbx_kick.h")).read()
    for word in ("Deliberately not here", "kick size per member", "member range", "drift-only", "nbody.x", "hipGraph", "add_rn", "mul_rn",
                 "h is not finite", "NBX_ERR_STATE", "nbx_commit", "kick-drift-kick", "nbx_accel", "nbx_ensemble_accel", "nbx_ragged_accel",
                 "not a collective", "before the first HIP call"):
        assert word in doc, word


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_null_handles_and_non_finite_kicks_are_rejected_before_hip_with_the_entry_point_named(nbx, name):
    """No device exists here: a status other than NBX_ERR_ARG, or another text, would mean a check came after a HIP call.  The
    kick size is looked at after the handle and before the state, so a handle that is merely not NULL -- zeroed memory that is no
    object -- reaches that check and nothing behind it."""
    L = nbx.load()
    f = getattr(L, name)
    ke = (ctypes.c_double * 4)(-7.25, -7.25, -7.25, -7.25)
    out = ctypes.cast(ke, f.argtypes[2]) if f.argtypes[2] is not ctypes.c_void_p else ctypes.c_void_p(ctypes.addressof(ke))
    for h in (0.05, 0.0, -0.05, math.nan, math.inf):
        for o in (None, out):
            assert f(None, h, o) == nbx.NBX_ERR_ARG
            assert L.nbx_last_error().decode() == "%s: %s" % (name, NULL_TEXT[name])  # the handle first, whatever h is
    zeroed = ctypes.create_string_buffer(1 << 16)
    for h in (math.nan, -math.nan, math.inf, -math.inf):
        for o in (None, out):
            assert f(ctypes.cast(zeroed, ctypes.c_void_p), h, o) == nbx.NBX_ERR_ARG
            assert L.nbx_last_error().decode() == name + ": h is not finite"
    assert list(ke) == [-7.25] * 4 and zeroed.raw == bytes(1 << 16)


def test_python_methods(nbx):
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged, nbx.Group):
        p = inspect.signature(cls.kick).parameters
        assert list(p) == ["self", "h", "kenergy"] and p["h"].default is inspect.Parameter.empty and p["kenergy"].default is False, cls
        p = inspect.signature(cls.leapfrog).parameters
        assert list(p) == ["self", "nsteps", "dt", "kenergy"] and p["dt"].default == nbx.DT and p["kenergy"].default is True, cls
    assert not [f for f, _ in nbx.Opts._fields_ if "kick" in f or "leap" in f]  # no new nbx_opts field


def test_leapfrog_is_the_two_half_kicks_around_the_plain_steps(nbx):
    calls = []

    class Fake(nbx._Leapfrog):
        def kick(self, h, kenergy=False):
            calls.append(("kick", h, kenergy))
            return "ke" if kenergy else None

        def step(self, nsteps, dt, kenergy=True):
            calls.append(("step", nsteps, dt, kenergy))

    assert Fake().leapfrog(7, 0.25) == "ke" and Fake().leapfrog(3, -0.5, kenergy=False) is None
    assert calls == [("kick", -0.125, False), ("step", 7, 0.25, False), ("kick", 0.125, True),
                     ("kick", 0.25, False), ("step", 3, -0.5, False), ("kick", -0.25, False)]
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged, nbx.Group):
        assert cls.leapfrog is nbx._Leapfrog.leapfrog, cls


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_kick\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_kick\.o: \$\(CSRC\)/nbx_kick\.hip(.*)$", mk, re.M)
    assert rule
    for dep in ("nbx_kick_kernels.hpp", "nbx_jlane.hpp", "nbx_jlane_loop.inc", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp",
                "nbx_internal.hpp", "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_pair.hpp", "include/nbx_kick.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_kick.hip", "include/nbx_kick.h"):
        assert word in sh, word


def test_the_kick_kernels_live_in_their_own_translation_unit_and_choose_the_epilogue_at_compile_time():
    for f in sorted(os.listdir(CSRC)):
        txt = open(os.path.join(CSRC, f)).read()
        if f not in ("nbx_kick.hip", "nbx_kick_kernels.hpp"):
            assert "nbx_kick_kernels.hpp" not in re.sub(r"//.*", "", txt), f  # nobody else includes the kernels
    txt = open(os.path.join(CSRC, "nbx_kick_kernels.hpp")).read()
    assert len(re.findall(r"jlane_step<NB, D, LOOP, JLANE_EPI_KICK>\(", txt)) == 2
    assert len(re.findall(r"jlane_step_f64<NB, D, JLANE_EPI_KICK>\(", txt)) == 2
    body = open(os.path.join(CSRC, "nbx_jlane.hpp")).read()
    assert "template <int NB, int D, int LOOP, int EPI = JLANE_EPI_ARG>" in body and "template <int NB, int D, int EPI = JLANE_EPI_ARG>" in body
    assert body.count("if constexpr (EPI == JLANE_EPI_KICK)") == 2
    for f in ("nbx_ensemble_kernels.hpp", "nbx_ragged_kernels.hpp", "nbx_batch_accel_kernels.hpp", "nbx_kernels.hpp"):
        assert "JLANE_EPI" not in open(os.path.join(CSRC, f)).read(), f  # the existing call sites are as they were


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the translation unit (positive statements about what it is made of)
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
    out = tmp_path_factory.mktemp("isa") / "nbx_kick.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _kick_key(name):
    """(kind, precision, NB, loop) of a kick kernel's symbol; kind "context" for kick_kernel<T>."""
    m = re.search(r"\d+(ensemble|ragged)_kick_kernelILi(\d+)ELi\d+ELi(\d)EE", name)
    if m:
        return (m.group(1), 32, int(m.group(2)), int(m.group(3)))
    m = re.search(r"\d+(ensemble|ragged)_kick_kernel_f64ILi(\d+)ELi\d+EE", name)
    if m:
        return (m.group(1), 64, int(m.group(2)), 0)
    m = re.search(r"^_ZN3nbx11kick_kernelI([fd])EE", name)
    if m:
        return ("context", 32 if m.group(1) == "f" else 64, 0, 0)
    return None


@pytest.fixture(scope="module")
def step_instances(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inst") / "instances")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe])
    out = subprocess.run([exe, "instances"], capture_output=True, text=True, check=True).stdout
    return sorted(tuple(map(int, line.split())) for line in out.splitlines())


def test_the_kernels_are_the_step_instances_once_per_kind_and_kick_kernel_in_two_precisions(isa, step_instances):
    assert len(step_instances) == 10
    keys = [_kick_key(k) for k in isa]
    assert None not in keys, list(isa)
    for kind in ("ensemble", "ragged"):
        assert sorted(k[1:] for k in keys if k[0] == kind) == step_instances, kind
    assert sorted(k[1] for k in keys if k[0] == "context") == [32, 64]
    assert len(isa) == 2 * len(step_instances) + 2


def test_a_batch_kick_stores_one_velocity_record_and_one_energy_partial_and_no_position(isa):
    """The epilogue is a compile-time choice: neither the integrating nor the storing one is in the code.  Per kernel the global
    stores are the velocity record -- 16 bytes in fp32, 32 in fp64 -- and the workgroup's fp64 partial, and there is no atomic: a
    position record would be a second record-sized store."""
    for name, (body, _, _) in isa.items():
        kind, precision = _kick_key(name)[:2]
        if kind == "context":
            continue
        stores = re.findall(r"\b((?:global|flat|buffer)_(?:store|atomic)\w*)", body)
        assert stores == ["global_store_dwordx4"] * (1 if precision == 32 else 2) + ["global_store_dwordx2"], (name, stores)


def test_the_context_kick_kernel_stores_three_velocity_components_and_one_energy_partial(isa):
    """kick_kernel<T> reads no position and has no position argument; its pointers are restrict-qualified, so the unchanged mass
    is not stored back: 12 bytes in fp32, 24 in fp64, then the partial."""
    want = {32: ["global_store_dwordx3", "global_store_dwordx2"], 64: ["global_store_dwordx4", "global_store_dwordx2", "global_store_dwordx2"]}
    for name, (body, _, _) in isa.items():
        kind, precision = _kick_key(name)[:2]
        if kind == "context":
            assert re.findall(r"\b((?:global|flat|buffer)_(?:store|atomic)\w*)", body) == want[precision], name


def test_no_scratch_and_no_spills(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_", body), name


def test_the_batch_kicks_keep_the_force_loop_of_the_step(isa):
    for name, (body, desc, _) in isa.items():
        kind, precision, NB, loop = _kick_key(name)
        if kind == "context":
            continue
        if precision == 64:
            assert re.search(r"\bv_rsq_f64", body), name
        else:
            for ins in ("v_pk_fma_f32", "v_pk_mul_f32", "v_rsq_f32"):
                assert re.search(r"\b%s" % ins, body), (name, ins)
            assert not re.search(r"\bv_div_scale|\bv_sqrt_f32", body), name
            assert ("#ASMSTART" in body) == (loop == 1), name
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_y %d\b" % (kind == "ensemble"), desc), name


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement: what the device tests ask of the library holds for the update itself, on the same systems
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def errors():
    """{(precision, seed, leap, 1/dt): |E(T) - E(0)| / |E(0)|}, computed once."""
    out = {}
    for prec, T in ((64, np.float64), (32, np.float32)):
        for seed in K.SEEDS:
            s = K.make_state(seed, dtype=T)
            for leap in (False, True):
                for inv in (64, 128, 256):
                    out[prec, seed, leap, inv] = K.energy_error(s, 1.0 / inv, leap)
    return out


def test_the_systems_are_what_the_issue_describes():
    for seed in K.SEEDS:
        s = K.make_state(seed)
        assert all(len(s[f]) == 96 and s[f].dtype == np.float64 for f in K.FIELDS)
        assert abs(float(np.float32(6.67259e-11)) * s["mass"].sum() - 1.0) < 0.1
        assert all(np.abs(s[f]).max() <= 1.0 for f in K.FIELDS[:3]) and all(np.abs(s[f]).max() <= 0.3 for f in K.FIELDS[3:6])
        again = K.make_state(seed)
        assert all((s[f] == again[f]).all() for f in K.FIELDS)  # a fixed seed
        s32 = K.make_state(seed, dtype=np.float32)
        assert all((s32[f] == s[f].astype(np.float32)).all() for f in K.FIELDS)


def test_plain_stepping_reads_out_a_first_order_energy_error(errors):
    for prec in (64, 32):
        for seed in K.SEEDS:
            e = [errors[prec, seed, False, inv] for inv in (64, 128, 256)]
            print("f%d seed %d plain: %.3e %.3e %.3e  ratios %.3f %.3f" % (prec, seed, e[0], e[1], e[2], e[0] / e[1], e[1] / e[2]))
            assert 2.1e-3 <= e[0] <= 2.8e-3 and 1.1e-3 <= e[1] <= 1.4e-3 and 5.4e-4 <= e[2] <= 7.0e-4, (prec, seed, e)
            assert 1.97 <= e[0] / e[1] <= 2.00 and 1.97 <= e[1] / e[2] <= 2.00, (prec, seed, e)
            assert 1.8 <= e[0] / e[1] <= 2.2  # the device tests' window


def test_the_two_half_kicks_make_it_second_order(errors):
    for seed in K.SEEDS:
        e = [errors[64, seed, True, inv] for inv in (64, 128, 256)]
        plain = errors[64, seed, False, 64]
        print("f64 seed %d leapfrog: %.3e %.3e %.3e  ratios %.3f %.3f  plain / leapfrog at 1/64: %.0f" % (seed, e[0], e[1], e[2], e[0] / e[1], e[1] / e[2], plain / e[0]))
        assert 1.4e-5 <= e[0] <= 3.0e-5 and 3.6e-6 <= e[1] <= 7.6e-6 and 0.9e-6 <= e[2] <= 1.9e-6, (seed, e)
        assert 3.9 <= e[0] / e[1] <= 4.1 and 3.9 <= e[1] / e[2] <= 4.1, (seed, e)
        assert 70 <= plain / e[0] <= 190, (seed, plain / e[0])
        assert 3.5 <= e[0] / e[1] <= 4.5 and e[0] <= plain / 20  # the device tests' gates
    for seed in K.SEEDS:
        e = [errors[32, seed, True, inv] for inv in (64, 128)]
        print("f32 seed %d leapfrog: %.3e %.3e  ratio %.3f" % (seed, e[0], e[1], e[0] / e[1]))
        assert 3.87 <= e[0] / e[1] <= 4.12, (seed, e)
        assert 3.3 <= e[0] / e[1] <= 4.7  # the device tests' window in fp32


def test_the_two_half_kicks_make_it_time_reversible():
    for seed in K.SEEDS:
        s = K.make_state(seed)
        leap, plain = K.there_and_back(s, 32, 1.0 / 64, True), K.there_and_back(s, 32, 1.0 / 64, False)
        leap32 = K.there_and_back(K.make_state(seed, dtype=np.float32), 32, 1.0 / 64, True)
        print("seed %d there and back: leapfrog %.2e (fp32 %.2e), plain %.2e" % (seed, leap, leap32, plain))
        assert leap <= 4e-15 and leap32 <= 2e-6 and 8e-3 <= plain <= 1.5e-1 * 1.5, (seed, leap, leap32, plain)
        assert leap <= 1e-10 and leap32 <= 1e-4 and plain > 1e-3  # the device tests' gates


def test_a_kick_of_the_restatement_is_the_velocity_half_of_its_step():
    for T in (np.float32, np.float64):
        s = K.make_state(K.SEEDS[0], dtype=T)
        a, b = K.copy(s), K.copy(s)
        K.kick(a, 1.0 / 64)
        K.step(b, 1, 1.0 / 64)
        assert all((a[f] == s[f]).all() for f in K.FIELDS[:3]) and all((a[f] == b[f]).all() for f in K.FIELDS[3:6])
        assert all(a[f].dtype == T for f in K.FIELDS)
