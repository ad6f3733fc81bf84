"""Member accelerations of ensembles and ragged ensembles (include/nbx_batch_accel.h), the parts that need no GPU: the header and
its two exported symbols, the argument checks that come before the first HIP call, the Python methods, the host-only work list
plan_ragged_accel through a g++ driver (also built with the address and undefined-behaviour sanitizers, as a stand-alone program),
the build files, and an audit of the cross-compiled gfx950 code of nbx_batch_accel.hip."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_batch_accel.hip")
DRIVER = os.path.join(ROOT, "tests", "ragged_accel_plan_driver.cpp")
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h")
ENTRY_POINTS = ("nbx_ensemble_accel", "nbx_ragged_accel")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_batch_accel.h"\n'
           'int main(void) { nbx_ensemble* e = NULL; nbx_ragged* r = NULL; nbx_ensemble_stats_t es; nbx_ragged_stats_t rs; '
           'int (*f)(nbx_ensemble*, int32_t, int32_t, void*, void*, void*) = nbx_ensemble_accel; '
           'int (*g)(nbx_ragged*, int32_t, int32_t, void*, void*, void*) = nbx_ragged_accel; '
           'int (*h)(nbx_ctx*, void*, void*, void*) = nbx_accel; '
           'printf("%d %d\\n", (int)sizeof es, (int)sizeof rs); return (f != NULL && g != NULL && h != NULL && e == NULL && r == NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_and_brings_both_of_its_parents(tmp_path, compiler, std, ext):
    src = tmp_path / ("accel." + ext)
    src.write_text(PROGRAM)
    obj = str(tmp_path / "accel.o")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])


def test_declared_set_is_the_two_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_batch_accel.h")
    assert declared == sorted(ENTRY_POINTS) and set(declared) == set(nbx.BATCH_ACCEL_SYMBOLS)
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS) |
                                set(nbx.RAGGED_SYMBOLS) | set(nbx.RAGGED_DIAG_SYMBOLS))
    # the parents' own sets are what they were
    assert len(_declared("nbx_ragged.h")) == 9 and len(_declared("nbx_ensemble.h")) == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == 6
    assert L.nbx_abi_version() == 1


def test_the_parent_headers_point_here_and_are_otherwise_as_they_were():
    for h in ("nbx_ensemble.h", "nbx_ragged.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        assert txt.count("nbx_batch_accel.h") == 1 and "Deliberately not here" in txt, h
        assert "nbx_batch_accel" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S), h  # in a comment only: no new include or symbol
    doc = open(os.path.join(ROOT, "include", "nbx_batch_accel.h")).read()
    for word in ("Deliberately not here", "device pointer", "reference summation", "hipGraph", "NBX_ERR_STATE", "NBX_KERNEL_JLANE"):
        assert word in doc, word


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_null_handles_are_rejected_with_a_text_that_names_the_entry_point(nbx, name):
    L = nbx.load()
    f = getattr(L, name)
    a = (ctypes.c_float * 4)()
    p = ctypes.c_void_p(ctypes.addressof(a))
    for h in (ctypes.c_void_p(), None):
        for args in ((0, 1, p, p, p), (0, 0, None, None, None), (-1, 5, p, None, None)):
            assert f(h, *args) == nbx.NBX_ERR_ARG
            text = L.nbx_last_error().decode()
            assert text.startswith(name + ": ") and "NULL" in text, text
    assert list(a) == [0.0] * 4


def test_python_methods(nbx):
    for cls in (nbx.Ensemble, nbx.Ragged):
        assert callable(cls.accel)
        p = inspect.signature(cls.accel).parameters
        assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None


# ---------------------------------------------------------------------------------------------------------------------------
# the work list
# ---------------------------------------------------------------------------------------------------------------------------
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra + [DRIVER, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("raplan"), "ragged_accel_plan_driver", [])


def test_the_driver_checks_its_own_lists(driver):
    r = subprocess.run([driver, "check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # six lists per precision; auto and 2, 4, 8 bodies per wave, fp32 also 16
    assert r.stdout.split() == ["54", "plans"], r.stdout


def test_the_driver_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program with the sanitizer runtimes linked into it."""
    exe = _build(tmp_path, "ragged_accel_plan_driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["54", "plans"], r.stdout[-2000:] + r.stderr[-4000:]
    text = "32 0 5 257 1 700 2048 5\n64 8 3 63 64 65\n32 16 1 16383\n"
    r = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 3 and not r.stderr, r.stderr[-4000:]


def _plan(driver, sizes, precision=32, nb=0):
    text = "%d %d %d %s\n" % (precision, nb, len(sizes), " ".join(map(str, sizes)))
    out = subprocess.run([driver, "plan"], input=text, capture_output=True, text=True, check=True).stdout
    p = json.loads(out)
    assert "error" not in p, p
    return p


LISTS = [(1,), (63, 64, 65), (257, 1, 700, 2048, 5), (2048,) * 64, (16383,), (12288,), (2048, 5, 2048, 700)]


@pytest.mark.parametrize("sizes", LISTS, ids=lambda s: "x".join(map(str, s[:5])) + ("..." if len(s) > 5 else ""))
@pytest.mark.parametrize("precision,nb", [(32, 0), (32, 2), (32, 16), (64, 0), (64, 8)])
def test_work_list_is_the_step_list_in_member_order(driver, sizes, precision, nb):
    """The same statements as the driver's own check, made here from its dump: nothing below calls the code under test."""
    if precision == 64:
        sizes = tuple(min(n, 12288) for n in sizes)
    p = _plan(driver, sizes, precision, nb)
    M, NB = len(sizes), p["NB"]
    assert nb in (0, NB)
    member, begin, work, step = p["member"], p["work_begin"], p["work"], p["step_work"]
    assert len(member) == M and len(begin) == M + 1
    grids = [-(-(-(-n // NB)) // 4) for n in sizes]          # ceil(ceil(n / NB) / 4): the workgroups of a context of n bodies
    assert [m[3] for m in member] == grids and [m[4] for m in member] == list(sizes)
    assert begin == [sum(grids[:k]) for k in range(M + 1)]    # the prefix sum of the members' workgroup counts
    assert len(work) == begin[M] == p["W"] == len(step)
    for k in range(M):
        pos, vel, ke, grid, n, n_alloc = member[k]
        assert n_alloc == -(-n // 256) * 256
        # wg = 0 .. grid_k - 1 in order, each with the offsets of plan_ragged's member table
        assert work[begin[k]:begin[k + 1]] == [[pos, vel, ke, wg, n, n_alloc, k] for wg in range(grid)], k
    # every workgroup of the step's list exactly once
    assert sorted(map(tuple, work)) == sorted(map(tuple, step))
    assert len({(w[6], w[3]) for w in work}) == len(work)
    # a member's records lie inside a slab laid out as velm, and members do not overlap
    ends = [m[1] + m[5] for m in member]
    assert [m[1] for m in member] == [0] + ends[:-1]


def test_the_step_list_is_longest_first_so_a_range_is_not_contiguous_in_it(driver):
    p = _plan(driver, (257, 1, 700, 2048, 5))
    assert [w[6] for w in p["step_work"]][0] == 3 and p["work"] != p["step_work"]
    assert [w[6] for w in p["work"]] == sorted(w[6] for w in p["work"])


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_batch_accel\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_batch_accel\.o: \$\(CSRC\)/nbx_batch_accel\.hip(.*)$", mk, re.M)
    assert rule
    for dep in ("nbx_batch_accel_kernels.hpp", "nbx_jlane.hpp", "nbx_jlane_loop.inc", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_pair.hpp", "include/nbx_ensemble.h", "include/nbx_ragged.h",
                "include/nbx_batch_accel.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_batch_accel.hip", "include/nbx_batch_accel.h"):
        assert word in sh, word


def test_the_step_kernels_still_pass_the_literal_zero():
    for f in ("nbx_ensemble_kernels.hpp", "nbx_ragged_kernels.hpp"):
        txt = open(os.path.join(CSRC, f)).read()
        assert len(re.findall(r"jlane_step(?:_f64)?<[^>]+>\([^;]*\), 0, ", txt)) == 2, f
    txt = open(os.path.join(CSRC, "nbx_batch_accel_kernels.hpp")).read()
    assert len(re.findall(r"jlane_step(?:_f64)?<[^>]+>\([^;]*\), 1, ", txt)) == 4


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
    out = tmp_path_factory.mktemp("isa") / "nbx_batch_accel.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3))
    return ks


def _accel_key(name):
    """(kind, precision, NB, loop) of an accel kernel's symbol."""
    m = re.search(r"\d+(ensemble|ragged)_accel_kernelILi(\d+)ELi\d+ELi(\d)EE", name)
    if m:
        return (m.group(1), 32, int(m.group(2)), int(m.group(3)))
    m = re.search(r"\d+(ensemble|ragged)_accel_kernel_f64ILi(\d+)ELi\d+EE", name)
    if m:
        return (m.group(1), 64, int(m.group(2)), 0)
    return None


def test_the_kernels_are_the_one_launch_instances_once_per_kind(isa, driver):
    """Exactly the rows of kEnsembleInstances, as ensemble_accel_kernel and as ragged_accel_kernel, and no step, reduce or
    diagnostics kernel."""
    out = subprocess.run([driver, "instances"], capture_output=True, text=True, check=True).stdout
    jlane = sorted(tuple(map(int, line.split())) for line in out.splitlines())
    assert len(jlane) == 10
    keys = [_accel_key(k) for k in isa]
    assert None not in keys, list(isa)
    for kind in ("ensemble", "ragged"):
        assert sorted(k[1:] for k in keys if k[0] == kind) == jlane, kind
    assert len(isa) == 2 * len(jlane)


def test_no_scratch_and_one_store_of_one_record(isa):
    """acc_only is a literal: the integrating branch is not in the code.  The only write to memory is the record {ax, ay, az, 0}
    -- 16 bytes in fp32, 32 in fp64 -- and there is no atomic."""
    for name, (body, desc) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        stores = re.findall(r"\b((?:global|flat|buffer)_(?:store|atomic)\w*)", body)
        assert stores == ["global_store_dwordx4"] * (1 if _accel_key(name)[1] == 32 else 2), (name, stores)


def test_fp32_kernels_keep_the_packed_pair_and_the_raw_rsq_and_the_generated_loop(isa):
    for name, (body, _) in isa.items():
        kind, precision, NB, loop = _accel_key(name)
        if precision == 64:
            assert re.search(r"\bv_rsq_f64", body), name
            continue
        for ins in ("v_pk_fma_f32", "v_pk_mul_f32", "v_rsq_f32"):
            assert re.search(r"\b%s" % ins, body), (name, ins)
        assert not re.search(r"\bv_div_scale|\bv_sqrt_f32", body), name
        assert ("#ASMSTART" in body) == (loop == 1), name


def test_grid_shapes(isa):
    for name, (body, desc) in isa.items():
        kind = _accel_key(name)[0]
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_x 1\b", desc), name
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_y %d\b" % (kind == "ensemble"), desc), name
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_z 0\b", desc), name
