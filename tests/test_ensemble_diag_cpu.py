"""Per-member diagnostics of an ensemble (include/nbx_ensemble_diag.h), the parts that need no GPU: the header and its one
exported symbol, the argument checks that come before the first HIP call, the Python method, and an audit of the
cross-compiled gfx950 code of nbx_ensemble_diag.hip."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG

SRC = os.path.join(PKG, "csrc", "nbx_ensemble_diag.hip")
HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


def test_header_compiles_as_c99_and_brings_both_of_its_parents(tmp_path):
    src = tmp_path / "ensdiag.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_ensemble_diag.h"\n'
                   'int main(void) { nbx_ensemble* e = NULL; nbx_diag_t d[2]; nbx_ensemble_stats_t s; '
                   'int (*f)(nbx_ensemble*, int32_t, int32_t, nbx_diag_t*) = nbx_ensemble_diagnostics; '
                   'printf("%zu %zu %d\\n", sizeof d, sizeof s, f != NULL && e == NULL); return NBX_ABI_VERSION - 1; }\n')
    obj = str(tmp_path / "ensdiag.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])


def test_declared_set_is_the_one_symbol_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_ensemble_diag.h")
    assert declared == ["nbx_ensemble_diagnostics"] and set(declared) == set(nbx.ENSEMBLE_DIAG_SYMBOLS)
    for h in HEADERS[:3]:
        assert not set(declared) & set(_declared(h)), h
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS))
    # the parents' own sets are what they were
    assert len(_declared("nbx_ensemble.h")) == 9 and len(_declared("nbx_diag.h")) == 2
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
    for e, out in ((null, d), (None, d), (null, None), (not_null, None)):
        assert L.nbx_ensemble_diagnostics(e, 0, 1, out) == nbx.NBX_ERR_ARG
        text = L.nbx_last_error().decode()
        assert text.startswith("nbx_ensemble_diagnostics: ") and "NULL" in text, text


def test_python_method_exists(nbx):
    assert callable(nbx.Ensemble.diagnostics)
    import inspect
    p = inspect.signature(nbx.Ensemble.diagnostics).parameters
    assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the translation unit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    mk = open(os.path.join(ROOT, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags
    out = tmp_path_factory.mktemp("isa") / "nbx_ensemble_diag.s"
    subprocess.check_call(["hipcc"] + flags + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
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
    _kernel(isa, r"ensemble_diag_kernelIfE")
    _kernel(isa, r"ensemble_diag_kernelIdE")
    _kernel(isa, r"ensemble_diag_reduce_kernel")
    assert not [k for k in isa if re.search(r"\d+diag_(reduce_)?kernel", k)], list(isa)  # a context's kernels stay in nbx_diag.hip


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_ensemble_diag\.o", mk, re.M)
    assert re.search(r"^\$\(PKG\)/nbx_ensemble_diag\.o: \$\(CSRC\)/nbx_ensemble_diag\.hip", mk, re.M)
    for unit in ("nbx_ensemble", "nbx_ensemble_diag"):  # both include the host layer shared with ragged ensembles
        assert re.search(r"^\$\(PKG\)/%s\.o:.*\$\(CSRC\)/nbx_ensemble_internal\.hpp.*\$\(CSRC\)/nbx_batch\.hpp" % unit, mk, re.M), unit
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    assert "-c nbx_ensemble_diag.hip" in sh and "include/nbx_ensemble_diag.h" in sh


def test_no_scratch_no_atomics_and_every_store_is_a_global_store(isa):
    for name, (body, desc) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert not re.search(r"\w+_atomic", body), name
        # results leave through vector stores: every instruction that stores to memory is a global_store
        stores = re.findall(r"^\s+(\w*store\w*)", body, re.M)
        assert stores and all(s.startswith("global_store") for s in stores), (name, sorted(set(stores)))


def test_fp32_kernel_keeps_the_packed_pair_the_raw_rsq_and_the_lds_broadcast(isa):
    body, _ = _kernel(isa, r"ensemble_diag_kernelIfE")
    for ins in ("v_pk_fma_f32", "v_pk_add_f32", "v_rsq_f32", "ds_read_b128"):
        assert re.search(r"\b%s" % ins, body), ins
    assert not re.search(r"\bv_div_scale|\bv_sqrt_f32|\bv_rcp_f32", body)
    # as diag_kernel<float, 2>: 3 sub + 4 FMA per two bodies, in both the plain and the masked tile loop
    assert len(re.findall(r"\bv_pk_fma_f32", body)) >= 8 and len(re.findall(r"\bv_pk_add_f32", body)) >= 6


def test_fp64_kernel_keeps_the_newton_refined_rsq(isa):
    body, _ = _kernel(isa, r"ensemble_diag_kernelIdE")
    assert re.search(r"\bv_rsq_f64", body)
    assert not re.search(r"\bv_div_scale|\bv_sqrt_f64", body)


def test_the_member_index_is_the_workgroup_id_z(isa):
    for pat in (r"ensemble_diag_kernelIfE", r"ensemble_diag_kernelIdE"):
        _, desc = _kernel(isa, pat)
        for dim in "xyz":
            assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_%s 1\b" % dim, desc), (pat, dim)
    _, desc = _kernel(isa, r"ensemble_diag_reduce_kernel")
    assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_x 1\b", desc)
