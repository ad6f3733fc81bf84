"""Per-member diagnostics of a ragged ensemble (include/nbx_ragged_diag.h), the parts that need no GPU: the header and its one
exported symbol, the argument checks that come before the first HIP call, the Python method, the host-only work list
plan_ragged_diag through a g++ driver -- every member's shape against the shapes derived by hand from diag_splits -- the build
files, and an audit of the cross-compiled gfx950 code of nbx_ragged_diag.hip."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_ragged_diag.hip")
DRIVER = os.path.join(ROOT, "tests", "ragged_diag_plan_driver.cpp")
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


def test_header_compiles_as_c99_and_brings_both_of_its_parents(tmp_path):
    src = tmp_path / "ragdiag.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_ragged_diag.h"\n'
                   'int main(void) { nbx_ragged* r = NULL; nbx_diag_t d[2]; nbx_ragged_stats_t s; '
                   'int (*f)(nbx_ragged*, int32_t, int32_t, nbx_diag_t*) = nbx_ragged_diagnostics; '
                   'int (*g)(nbx_ctx*, nbx_diag_t*) = nbx_diagnostics; '
                   'printf("%zu %zu %d\\n", sizeof d, sizeof s, f != NULL && g != NULL && r == NULL); return NBX_ABI_VERSION - 1; }\n')
    obj = str(tmp_path / "ragdiag.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])


def test_declared_set_is_the_one_symbol_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_ragged_diag.h")
    assert declared == ["nbx_ragged_diagnostics"] and set(declared) == set(nbx.RAGGED_DIAG_SYMBOLS)
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS) |
                                set(nbx.RAGGED_SYMBOLS))
    # the parents' own sets are what they were
    assert len(_declared("nbx_ragged.h")) == 9 and len(_declared("nbx_ensemble.h")) == 9
    assert len(_declared("nbx_diag.h")) == 2 and len(_declared("nbx_ensemble_diag.h")) == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert getattr(L, s).argtypes is not None


def test_null_arguments_are_rejected_with_a_text_before_any_device_call(nbx):
    L = nbx.load()
    null = ctypes.c_void_p()
    d = (nbx.Diag * 2)()
    not_null = ctypes.c_void_p(ctypes.addressof(d))  # never dereferenced: `out` is NULL in that call
    for r, out in ((null, d), (None, d), (null, None), (not_null, None)):
        assert L.nbx_ragged_diagnostics(r, 0, 1, out) == nbx.NBX_ERR_ARG
        text = L.nbx_last_error().decode()
        assert text.startswith("nbx_ragged_diagnostics: ") and "NULL" in text, text


def test_python_method_signature(nbx):
    assert callable(nbx.Ragged.diagnostics)
    p = inspect.signature(nbx.Ragged.diagnostics).parameters
    assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None


# ---------------------------------------------------------------------------------------------------------------------------
# the work list
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rdplan") / "ragged_diag_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def _plan(driver, sizes, precision=32):
    text = "%d %d %s\n" % (precision, len(sizes), " ".join(map(str, sizes)))
    out = subprocess.run([driver, "plan"], input=text, capture_output=True, text=True, check=True).stdout
    p = json.loads(out)
    assert "error" not in p, p
    return p


# n -> (cols, tiles, splits, tiles_per_split, rows), derived by hand from diag_splits: cols = ceil(n / 512), tiles = ceil(n / 256),
# s = max(1, tiles // 4) (the 1024-workgroup target never binds below 33 columns), per = ceil(tiles / s), splits = ceil(tiles / per)
SHAPES = {
    5: (1, 1, 1, 1, 1), 65: (1, 1, 1, 1, 1), 256: (1, 1, 1, 1, 1),
    257: (1, 2, 1, 2, 1), 512: (1, 2, 1, 2, 1),
    513: (2, 3, 1, 3, 2),
    1000: (2, 4, 1, 4, 2),
    2000: (4, 8, 2, 4, 8), 2048: (4, 8, 2, 4, 8),
    2049: (5, 9, 2, 5, 10),       # the last split holds 4 tiles
    4099: (9, 17, 4, 5, 36),      # the last split holds 2
    6300: (13, 25, 5, 5, 65),     # diag_splits asks for 6 splits and 5 remain
    8192: (16, 32, 8, 4, 128),
    12288: (24, 48, 12, 4, 288),
    16383: (32, 64, 16, 4, 512),
}


def test_every_member_gets_the_shape_of_a_context_of_its_size(driver):
    sizes = sorted(SHAPES)
    p32 = _plan(driver, sizes, 32)
    for n, got in zip(sizes, p32["shape"]):
        assert tuple(got) == SHAPES[n], (n, got)
    # fp64 (members up to 12288 bodies): two bodies per lane as well, hence the same shapes
    capped = [n for n in sizes if n <= 12288]
    p64 = _plan(driver, capped, 64)
    assert p32["bodies"] == p64["bodies"] == 2
    for n, got in zip(capped, p64["shape"]):
        assert tuple(got) == SHAPES[n], (n, got)


POPULATIONS = [(5, 65, 1000, 256, 257, 513, 2000, 63), (16383, 5, 8192)]


@pytest.mark.parametrize("sizes", POPULATIONS)
@pytest.mark.parametrize("precision", [32, 64])
def test_work_list_is_in_member_order_and_tiles_the_partial_rows(driver, sizes, precision):
    if precision == 64:
        sizes = tuple(min(n, 12288) for n in sizes)
    p = _plan(driver, sizes, precision)
    M = len(sizes)
    shape, rows, begin, work, member = p["shape"], p["rows"], p["work_begin"], p["work"], p["member"]
    assert len(shape) == len(rows) == len(member) == M and len(begin) == M + 1
    assert [m[2] for m in member] == list(sizes)
    # every (member, split, col) exactly once; member order, then split, then column
    expect = [(k, s, c) for k in range(M) for s in range(shape[k][2]) for c in range(shape[k][0])]
    assert p["total_rows"] == p["total_groups"] == len(work) == len(expect) == sum(s[4] for s in shape)
    at = 0
    for k in range(M):
        cols, tiles, splits, per, nrows = shape[k]
        assert nrows == cols * splits and per <= 7 and splits * per >= tiles > (splits - 1) * per
        assert begin[k] == at and rows[k] == [at, nrows]  # work_begin: the prefix sum of rows; a member's rows follow its predecessor's
        for i in range(nrows):
            pos, vel, row_off, n, col, split, wcols, wper = work[at + i]
            assert (k, split, col) == expect[at + i], (k, i)
            assert [pos, vel, n] == member[k], (k, i)  # the member's own offsets, from RaggedPlan::member
            assert (row_off, wcols, wper) == (at, cols, per), (k, i)
            assert split * wcols + col == i  # diag_body's row within the member = the descriptor's place within the member
        at += nrows
    assert begin[M] == at == p["total_rows"]  # row ranges are disjoint and tile [0, total_rows)
    assert all(w[7] <= 7 for w in work)


def test_every_size_takes_diag_splits_own_answer_and_at_most_seven_tiles(driver):
    r = subprocess.run([driver, "walk"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert int(r.stdout.split()[0]) == 16383 + 12288, r.stdout


def test_one_shape_rule_for_all_three_callers():
    """diag_splits is defined once, in a header the device code and the host-only planner both include."""
    defs = [f for f in sorted(os.listdir(CSRC)) if re.search(r"^inline void diag_splits\(", open(os.path.join(CSRC, f)).read(), re.M)]
    assert defs == ["nbx_diag_shape.hpp"], defs
    for f in ("nbx_diag_body.hpp", "nbx_plan.hpp"):
        assert '#include "nbx_diag_shape.hpp"' in open(os.path.join(CSRC, f)).read(), f
    for f in ("nbx_diag.hip", "nbx_ensemble_diag.hip", "nbx_plan.hpp"):
        assert re.search(r"\bdiag_splits\(", open(os.path.join(CSRC, f)).read()), f


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_ragged_diag\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_ragged_diag\.o: \$\(CSRC\)/nbx_ragged_diag\.hip(.*)$", mk, re.M)
    assert rule
    for dep in ("nbx_ragged_diag_kernels.hpp", "nbx_diag_body.hpp", "nbx_diag_shape.hpp", "nbx_ragged_internal.hpp", "nbx_plan.hpp",
                "include/nbx_ragged.h", "include/nbx_ragged_diag.h"):
        assert dep in rule.group(1), dep
    assert re.search(r"^\$\(PKG\)/nbx_ragged\.o:.*nbx_ragged_internal\.hpp", mk, re.M)
    for unit in ("nbx_ragged", "nbx_ragged_diag"):  # both include the host layer shared with ensembles
        assert re.search(r"^\$\(PKG\)/%s\.o:.*\$\(CSRC\)/nbx_batch\.hpp" % unit, mk, re.M), unit
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_ragged.hip", "-c nbx_ragged_diag.hip", "include/nbx_ragged.h", "include/nbx_ragged_diag.h"):
        assert word in sh, word


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the translation unit (positive statements about what it is made of)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    from test_isa_audit import _shipped_hipflags
    out = tmp_path_factory.mktemp("isa") / "nbx_ragged_diag.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3))
    return ks


def _kernel(ks, pattern):
    names = [k for k in ks if re.search(pattern, k)]
    assert len(names) == 1, (pattern, list(ks))
    return ks[names[0]]


def test_exactly_three_kernels(isa):
    assert len(isa) == 3, list(isa)
    _kernel(isa, r"18ragged_diag_kernelIfE")
    _kernel(isa, r"18ragged_diag_kernelIdE")
    _kernel(isa, r"25ragged_diag_reduce_kernel")
    # a context's and an ensemble's diagnostics kernels and every step kernel stay in their own translation units
    assert all(re.search(r"_ZN3nbx(18ragged_diag_kernelI|25ragged_diag_reduce_kernel)", k) for k in isa), list(isa)


def test_no_scratch(isa):
    for name, (_, desc) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name


def test_fp32_kernel_keeps_the_packed_pair_the_raw_rsq_and_the_lds_broadcast(isa):
    body, _ = _kernel(isa, r"ragged_diag_kernelIfE")
    for ins in ("v_pk_fma_f32", "v_pk_add_f32", "v_rsq_f32", "ds_read_b128"):
        assert re.search(r"\b%s" % ins, body), ins
    assert not re.search(r"\bv_div_scale|\bv_sqrt_f32", body)


def test_fp64_kernel_keeps_the_newton_refined_rsq(isa):
    body, _ = _kernel(isa, r"ragged_diag_kernelIdE")
    assert re.search(r"\bv_rsq_f64", body)


def test_the_grid_is_one_dimensional_and_the_descriptor_arrives_by_one_scalar_load(isa):
    for pat in (r"ragged_diag_kernelIfE", r"ragged_diag_kernelIdE"):
        body, desc = _kernel(isa, pat)
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_x 1\b", desc), pat
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_y 0\b", desc) and re.search(r"\.amdhsa_system_sgpr_workgroup_id_z 0\b", desc), pat
        # the 32-byte descriptor at a wave-uniform index: the index shifted by 5 on the scalar unit, then one 8-dword scalar load
        # (a second one brings the kernel arguments)
        assert re.search(r"\bs_lshl_b64 s\[\d+:\d+\], s\[\d+:\d+\], 5\b", body), pat
        assert len(re.findall(r"\bs_load_dwordx8\b", body)) >= 2, pat
    _, desc = _kernel(isa, r"ragged_diag_reduce_kernel")
    assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_x 1\b", desc)
