"""Friends-of-friends groups (include/nbx_fof.h), the parts that need no GPU: the header and its three exported symbols, the
argument checks that come before the first HIP call, the Python methods and the catalogue helper, the build files, an audit of
the cross-compiled gfx950 code of nbx_fof.hip, and the numpy reference tests/fof_ref.py, which must show by itself what the
device tests then ask of the library: that its restatement of the pass scheme is the plain definition, that EVERY (state,
radius) the device tests compare with it is unambiguous, and that every planted fault is caught.

Which state catches which planted fault ("caught" = fof_ref.differs, the comparison of the device tests):
    chain(4097, random): no hook, no shortcut (the labels are right, the passes are not: 9 become hundreds)
    cloud(513), many groups: padding label 0 (255 padding records at the origin, inside the cloud, within h2 of a body that is
        not of body 0's group)
    lattice(13) at the tie radius 1/8: < instead of <= (every r2 of a face neighbour IS h2: one group becomes 2197)
    cloud(2049), one giant group: a split row dropped in the finish (two splits)
    cloud(2049): label is any member, size without the body itself, labels offset by the member's place
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fof_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2
from field_ref import field_shape

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_fof.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_fof_kernels.hpp"
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h", "nbx_field.h", "nbx_neighbours.h", "nbx_paircount.h", "nbx_tracers.h", "nbx_knn.h")
ENTRY_POINTS = ("nbx_fof", "nbx_ensemble_fof", "nbx_ragged_fof")
NOUN = {"nbx_fof": "ctx", "nbx_ensemble_fof": "ensemble", "nbx_ragged_fof": "ragged ensemble"}
OTHER_TUPLES = ("SYMBOLS", "DIAG_SYMBOLS", "ENSEMBLE_SYMBOLS", "ENSEMBLE_DIAG_SYMBOLS", "RAGGED_SYMBOLS", "RAGGED_DIAG_SYMBOLS",
                "BATCH_ACCEL_SYMBOLS", "KICK_SYMBOLS", "TIMESCALE_SYMBOLS", "FIELD_SYMBOLS", "NEIGHBOUR_SYMBOLS", "PAIRCOUNT_SYMBOLS",
                "TRACER_SYMBOLS", "KNN_SYMBOLS")
FORBIDDEN = ("neighbour_kernel", "nb_body", "field_kernel", "field_body", "timescale_kernel", "tracer_kernel", "tracer_body",
             "tracer_update_kernel", "knn_kernel", "knn_body", "knn_insert")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


OUT4 = "int32_t*, int32_t*, nbx_fof_info_t*, int32_t*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_fof.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, double, %s) = nbx_fof; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, double, %s) = nbx_ensemble_fof; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, double, %s) = nbx_ragged_fof; '
           'nbx_fof_info_t i; i.groups = 1; i.largest = 1; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL && sizeof(i) == 8 && i.groups == i.largest && NBX_ERR_INTERNAL == -5) '
           '? NBX_ABI_VERSION - 1 : 1; }\n' % (OUT4, OUT4, OUT4))
PARAMS = "double r, int32_t* l, int32_t* s, nbx_fof_info_t* i, int32_t* p"
UNUSED = "(void)r; (void)l; (void)s; (void)i; (void)p;"
STUBS = ('#include "nbx_fof.h"\n'
         'int nbx_fof(nbx_ctx* h, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_fof(nbx_ensemble* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_fof(nbx_ragged* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "fof_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_three_symbols_exported_and_apart_from_every_other_tuple(nbx):
    declared = _declared("nbx_fof.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.FOF_SYMBOLS) == ENTRY_POINTS and len(nbx.FOF_SYMBOLS) == 3
    assert nbx.FOF_KEYS == ("label", "size", "groups", "largest", "passes") == R.KEYS + ("passes",) and nbx.NBX_ERR_INTERNAL == -5
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "_fof" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in OTHER_TUPLES:
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (6 if s == "nbx_fof" else 8)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_fof.h")).read())  # the comment as running text
    for word in ("Why:", "Definition", "Per-pair arithmetic", "Consequences", "How:", "Semantics", "Status, in this order", "Unspecified results",
                 "Deliberately not here", "fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))", "h2        = fma(rT, rT, eps2)", "i != j, both < n",
                 "the LOWEST index", "member-local", "label[i] == i", "the number of pair-work launches", "label = 0, size = 1, groups = 1",
                 "never anybody's", "compared as integers", "r2(i, j) and r2(j, i) are the same bits",
                 "label[i] == label[index[i]]", "size[i] >= within[i] + 1", "groups == n iff", "N[L[i]] = min(N[L[i]], m[i])", "N[i] = N[N[i]]",
                 "that pass counts", "Labels only decrease", "gives the same bits", "a NULL array is never written",
                 "member-major", "end to end", "sliced context", "nbx_commit", "synchronises once per pass", "4-byte read-back", "steps_done",
                 "*_timed / *_ms_total", "kinetic-energy partials", "the state of graph", "radius is NaN or negative", "checked in 64 bits", "2^22",
                 "names the first such member", "before the first HIP call", "NBX_ERR_ALLOC", "NBX_ERR_INTERNAL", "n + 1 passes", "not finite",
                 "groups (multi-GPU)", "periodic boxes", "bound or unbound", "a linking length per member", "device pointers",
                 "nbody.x"):
        assert word in doc, word
    old = open(os.path.join(ROOT, "include", "nbx_neighbours.h")).read()
    assert "a neighbour list (variable length)" in old  # the gap this header works around, named by the one it extends


def _call(nbx, name, handle, radius, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    args = [radius] + [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in out]
    return f(handle, *args) if name == "nbx_fof" else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    out = [np.full(64, -7, dtype=np.int32) for _ in range(4)]
    none4 = [None] * 4
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    nan = float("nan")
    # 1. the handle is NULL -- whatever else is wrong
    for r, o in ((0.25, out), (-1.0, none4), (nan, out)):
        assert _call(nbx, name, None, r, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. radius NaN or negative -- before the range, also where nothing is asked for
    for r in (nan, -1e-300, -1.0, -float("inf")):
        for o in (out, none4, [out[0], None, None, None], [None, None, None, out[3]]):
            assert _call(nbx, name, handle, r, o, -1, 5) == nbx.NBX_ERR_ARG
            assert err() == name + ": radius is NaN or negative"
    if name != "nbx_fof":
        # 3. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for r in (0.0, 0.25, float("inf")):
                assert _call(nbx, name, handle, r, out, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 7. count == 0 inside the range: NBX_OK, nothing written (passes included), no HIP call -- with outputs and without
        assert _call(nbx, name, handle, 0.25, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, 0.0, none4, 0, 0) == nbx.NBX_OK
    else:
        # 5. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for r, o in ((0.25, out), (0.0, none4), (1.0, [None, None, out[2], None])):
            assert _call(nbx, name, handle, r, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_fof: nbx_upload has not been called"
    assert all((a == -7).all() for a in out) and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_the_pass_guard_and_their_texts_are_in_the_source():
    """More than 2^22 bodies in one call cannot be made here without a device; the check and its three texts are read off the
    source, between the range check and the upload check.  So is the guard of n + 1 passes."""
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kFofMaxBodies = kFieldMaxPoints;" in hdr and "constexpr int kFofNone = 0x7fffffff;" in hdr
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_fof: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kFofMaxBodies" in src and "range_bodies(o, first, count) > kFofMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_fof("):]
    order = [batch.index(w) for w in ("is NULL", "bad_radius(", "check_range(", "kFofMaxBodies", "check_uploaded(", "no_output(a)", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_fof("):]
    order = [ctx.index(w) for w in ("is NULL", "bad_radius(", "kFofMaxBodies", "->uploaded", "pending_commit", "no_output(a)", "use_device(")]
    assert order == sorted(order)
    assert "if (passes > n_max) return fail(NBX_ERR_INTERNAL" in src and "did not settle in n + 1 passes" in src
    # one synchronisation per pass, on a 4-byte word, and one for the results: the pass loop is the call's own flow, not the shared
    # read-back skeleton
    assert len(re.findall(r"hipStreamSynchronize\(o->stream\)", src)) == 3 and "sizeof(int), hipMemcpyDeviceToHost" in src
    assert "read_back(" not in src


def test_python_methods_keys_and_the_helper_are_as_specified(nbx):
    p = inspect.signature(nbx.Context.fof).parameters
    assert list(p) == ["self", "radius"] and p["radius"].default is inspect.Parameter.empty
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.fof).parameters
        assert list(p) == ["self", "radius", "first", "count"], cls
        assert p["radius"].default is inspect.Parameter.empty and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "fof")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "fof" in f]  # no new nbx_opts field
    p = inspect.signature(nbx.fof_catalogue).parameters
    assert list(p) == ["label", "mass", "x", "y", "z", "min_members"] and p["min_members"].default == 2
    with pytest.raises(nbx.NbxError):
        nbx.fof_catalogue(np.zeros(4, dtype=np.int32), np.ones(3), np.ones(4), np.ones(4), np.ones(4))


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_fof\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_fof\.o: \$\(CSRC\)/nbx_fof\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    knn = re.search(r"^\$\(PKG\)/nbx_knn\.o: \$\(CSRC\)/nbx_knn\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == knn.group(1).replace("knn", "fof")  # the same dependency list
    for dep in (KERNELS, "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_diag_shape.hpp", "nbx_pair.hpp", "include/nbx_fof.h",
                "include/nbx_ensemble.h", "include/nbx_ragged.h", "include/nbx.h", "include/nbx_diag.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_fof.hip", "include/nbx_fof.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_reuse_the_shape_rule_and_keep_to_the_naming_rules():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_fof.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_fof.hip", KERNELS):
            assert "fof_pass_kernel" not in txt and "fof_body" not in txt and "fof_hook_kernel" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    both = re.sub(r"//.*", "", src + kern)
    for word in FORBIDDEN:
        assert word not in src + kern, word  # comments included: the other features' tests read every file
    assert not re.search(r'#include "nbx_(?!fof)\w+_kernels\.hpp"', both)  # no other feature's kernels
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern  # the field's rule, no new one
    assert "diag_splits" not in both and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)
    assert "fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())))" in kern  # r2 restated, not shared
    # atomics: the hook's two minima, the histogram's add, the info's add and max -- and none in the pair work
    assert len(re.findall(r"\batomic\w+\(", both)) == 5 and both.count("atomicMin(") == 2
    body = kern[kern.index("void fof_body("):kern.index("struct FofRange")]
    assert "atomic" not in re.sub(r"//.*", "", body) and "posm" not in re.sub(r"//.*", "", body)  # the pair work reads the staged records alone
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    assert "rec_off += (unsigned long long)padded(mem.n);" in src  # the staged records' offset is accumulated in this call's own maker
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("fof_rec", "fof_part", "fof_work", "fof_out", "fof_tab"):
        assert re.search(r"void\* %s = nullptr;" % field, obj) and "o->%s" % field in obj[obj.index("inline void batch_release"):], field


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
    out = tmp_path_factory.mktemp("isa") / "nbx_fof.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair-work kernel, (name, precision or None) of another."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)fof_pass_kernelI([fd])E", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+fof_(init|shortcut)_kernelI([fd])", name)
    if m:
        return (m.group(1), 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+fof_(hook|count|gather)_kernelE", name)
    return (m.group(1), None) if m else None


PAIR_KINDS = ("context", "ensemble", "ragged")


def test_every_kind_and_precision_is_compiled(isa):
    keys = sorted((_key(k) or ("?", k) for k in isa), key=str)
    want = [(kind, p) for kind in PAIR_KINDS + ("init",) for p in (32, 64)] + [("shortcut", p) for p in (32, 64)] * 2
    want += [(k, None) for k in ("hook", "count", "gather")]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_and_one_tile_of_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        kind, precision = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (256 * (16 if precision == 32 else 32) if kind in PAIR_KINDS else 0), (name, lds)


def test_the_pair_work_is_packed_in_fp32_reads_records_whole_and_has_no_atomics(isa):
    for name, (body, desc, meta) in isa.items():
        kind, precision = _key(name)
        c = lambda ins: len(re.findall(r"\b%s" % ins, body))
        atomics = c(r"(?:global|flat|ds|buffer)_atomic") + c(r"ds_(?:add|min|max)_")
        if kind not in PAIR_KINDS:
            assert (atomics > 0) == (kind in ("hook", "count", "gather")), (name, atomics)
            if kind == "hook":
                assert c("global_atomic_smin") + c("flat_atomic_smin") == 2, name
            continue
        assert atomics == 0, name
        # no root, no reciprocal and no packed multiply anywhere (a ragged kernel divides integers for field_shape: plain
        # multiplies may occur)
        assert c("v_rsq_") == 0 and c("v_sqrt") == 0 and c("v_rcp_f") == 0 and c("v_pk_mul_f32") == 0 and c("v_mul_f64") == 0, name
        records = c(r"ds_(?:read|load)_b128")
        if precision == 64:
            assert records >= 2 and c("v_fma_f64") + c("v_fmac_f64") >= 3 and c("v_add_f64") >= 3, name  # a record is two 16-byte reads
            assert c("v_min_i32") == records and c(r"v_cmp_\w+_f64") >= records, (name, records)
            continue
        assert records >= 1, name  # ONE tile loop: no masked variant
        # per j record the lane's two bodies, i.e. two pairs: 3 packed subtracts and 3 packed fused multiply-adds, then per pair
        # one compare, one integer minimum and one select
        assert c("v_pk_fma_f32") == 3 * records and c("v_pk_add_f32") == 3 * records, (name, records, c("v_pk_fma_f32"), c("v_pk_add_f32"))
        assert c("v_min_i32") == 2 * records, (name, records, c("v_min_i32"))
        against_h2 = c(r"v_cmp_ge_f32_e\d+ (?:vcc|s\[\d+:\d+\]), s\d+, v\d+\n")  # h2 is a scalar (a ragged kernel also compares floats to divide integers)
        assert against_h2 == 2 * records and c("v_cndmask_b32") >= 2 * records, (name, records, against_h2)
        if kind != "ragged":  # (a ragged kernel converts to divide integers for field_shape)
            assert c(r"v_cvt_\w*i32_f32") == 0 and c(r"v_cvt_f32_[iu]32") == 0, name  # the label is never converted: moved as bits
        print("%s: %d records per unrolled loop body" % (name, records))


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _state(xs, T=np.float64):
    n = len(xs)
    st = {f: np.zeros(n, dtype=T) for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
    for f, col in zip(R.POS, zip(*xs)):
        st[f] = np.array(col, dtype=T)
    st["mass"] = np.ones(n, dtype=T)
    return st


@pytest.mark.parametrize("precision", [32, 64])
def test_small_systems_give_the_closed_forms(precision):
    for f in (R.fof, R.restate):
        one = f(_state([(0.5, 0.25, -1.0)]), 3.0, precision)
        assert one["label"].tolist() == [0] and one["size"].tolist() == [1] and (one["groups"], one["largest"]) == (1, 1)
        two = _state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)])
        assert f(two, 1.99, precision)["label"].tolist() == [0, 1] and f(two, 2.0, precision)["label"].tolist() == [0, 0]  # <=: the tie is a friend
        # three on a line at 0, 1, 3 and one far away, indices mixed: {0, 2} at 1, {0, 1, 2} at 2
        line = _state([(1.0, 0.0, 0.0), (3.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 50.0, 0.0)])
        assert f(line, 1.5, precision)["label"].tolist() == [0, 1, 0, 3] and f(line, 1.5, precision)["size"].tolist() == [2, 1, 2, 1]
        got = f(line, 2.5, precision)
        assert got["label"].tolist() == [0, 0, 0, 3] and (got["groups"], got["largest"]) == (2, 3)
        # distinct bodies at one position are friends at radius 0
        same = f(_state([(1.0, 1.0, 1.0), (4.0, 1.0, 1.0), (1.0, 1.0, 1.0)]), 0.0, precision)
        assert same["label"].tolist() == [0, 1, 0]
    assert R.restate(_state([(0.5, 0.25, -1.0)]), 3.0, precision)["passes"] == 1  # the pass that changes nothing counts
    assert R.restate(_state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)]), 3.0, precision)["passes"] == 2


@pytest.mark.parametrize("precision", [32, 64])
def test_every_case_of_the_device_tests_is_unambiguous_and_the_restatement_is_the_plain_definition(precision):
    """The share of device cases left out for ambiguity is 0: every radius was chosen by pick_radius (or is a closed form far from
    every r2) and is shown here to keep every pair's r2 -- and every body's r2 to the padding records -- 64 u away from h2."""
    cases = R.reference_cases(precision)
    assert len(cases) == 2 * 7 * 3 + 8 + 4 + R.ENSEMBLE_MEMBERS + len(R.RAGGED_SIZES)
    shown = 0
    for name, st, radius, close in cases:
        assert not R.ambiguous(st, radius, precision, close), (precision, name, radius)
        shown += 1
        want = R.fof(st, radius, precision, close=close)
        got = R.restate(st, radius, precision, close=close)
        assert not R.differs(got, want, passes=False), (precision, name)
        n = len(st["mass"])
        assert (want["label"] <= np.arange(n)).all() and want["size"].sum() == (want["size"].astype(np.int64) ** 2)[want["label"] == np.arange(n)].sum()
        assert want["groups"] == len(set(want["label"].tolist())) and 1 <= got["passes"] <= 16
        print("fp%d %-28s r = %.5f: %5d groups, largest %5d, %2d passes" % (precision, name, radius, want["groups"], want["largest"], got["passes"]))
    assert shown == len(cases)  # none left out
    for k in (13, 33):  # the lattices' radii, from the geometry (33^3 has too many pairs to list)
        for r in (R.LATTICE_BELOW, R.LATTICE_ABOVE):
            assert not R.lattice_ambiguous(k, r, precision), (k, r)
        assert R.lattice_ambiguous(k, R.LATTICE_TIE, precision)  # the tie radius is the opposite: h2 IS an r2, bit for bit
    st = R.lattice(13, precision)
    assert R.ambiguous(st, R.LATTICE_TIE, precision) and not R.ambiguous(st, R.LATTICE_ABOVE, precision)
    # the three radii of the clouds are the three regimes
    for n in (2049, 4097):
        st, close, radii = R.sized(precision, "cloud", n)
        few, many, giant = (R.fof(st, r, precision, close=close) for r in radii)
        assert few["groups"] > 0.85 * n and few["largest"] <= 8
        assert 0.3 * n < many["groups"] < 0.7 * n and many["largest"] < 0.05 * n
        assert giant["largest"] > 0.7 * n and giant["groups"] > 30
    # the ambiguity measure itself: a partner 8 u from h2 is ambiguous, 256 u is not
    u = R.U[precision]
    for rel, want in ((8 * u, True), (256 * u, False)):
        d2 = (R.h2_of(0.5, precision) - EPS2) * (1 + rel)
        assert R.ambiguous(_state([(10.0, 0.0, 0.0), (10.0 + np.sqrt(d2), 0.0, 0.0)]), 0.5, precision) == want, rel
    assert (field_shape(257, 257)[2], field_shape(2049, 2049)[2:], field_shape(4097, 4097)[2:]) == (1, (2, 5), (4, 5))
    assert field_shape(33 ** 3, 33 ** 3) == (71, 141, 15, 10) and field_shape(8192, 8192)[:3] == (16, 32, 8)


@pytest.mark.parametrize("precision", [32, 64])
def test_chains_and_lattices_have_the_closed_forms_and_the_simulated_pass_counts(precision):
    n = R.CHAIN_N
    passes = {}
    for order in R.CHAIN_ORDERS:
        got = R.restate(R.chain(n, precision, order), R.CHAIN_RADIUS, precision)
        assert (got["groups"], got["largest"]) == (1, n) and (got["label"] == 0).all() and (got["size"] == n).all(), order
        passes[order] = got["passes"]
        cut = n // 3
        st = R.chain(n, precision, order, cut=cut)
        two = R.restate(st, R.CHAIN_RADIUS, precision)
        site = R.chain_order(n, order)
        low, high = int(np.nonzero(site < cut)[0].min()), int(np.nonzero(site >= cut)[0].min())
        assert two["groups"] == 2 and two["largest"] == n - cut, order
        assert np.array_equal(two["label"], np.where(site < cut, low, high)) and np.array_equal(two["size"], np.where(site < cut, cut, n - cut))
        assert not R.differs(two, R.fof(st, R.CHAIN_RADIUS, precision), passes=False)
    print("fp%d chain(%d) passes: %r" % (precision, n, passes))
    assert passes["ascending"] == passes["descending"] == 2 and passes["zigzag"] == 3 and 9 <= passes["random"] <= 10
    assert R.restate(R.chain(n, precision, "random"), R.CHAIN_RADIUS, precision, fault="no hook")["passes"] > 100  # why the hook is specified
    for k, want_passes in ((13, {False: 2, True: 4}), (33, {False: 2, True: 5})):
        for perm in (False, True):
            st = R.lattice(k, precision, perm)
            pairs = R.lattice_pairs(k, perm)
            if k == 13:  # the geometry's pairs are the computed ones
                found = R.friend_pairs(st, R.LATTICE_ABOVE, precision)
                assert sorted(map(tuple, found.tolist())) == sorted(map(tuple, pairs.tolist()))
                assert len(R.friend_pairs(st, R.LATTICE_BELOW, precision)) == 0 and len(R.friend_pairs(st, R.LATTICE_TIE, precision)) == len(pairs)
            above = R.restate(st, R.LATTICE_ABOVE, precision, pairs=pairs)
            assert (above["groups"], above["largest"], above["passes"]) == (1, k ** 3, want_passes[perm]) and (above["label"] == 0).all()
            below = R.restate(st, R.LATTICE_BELOW, precision, pairs=pairs[:0])
            assert (below["groups"], below["largest"], below["passes"]) == (k ** 3, 1, 1) and np.array_equal(below["label"], np.arange(k ** 3))


def _fault_case(precision, fault):
    """(state, radius, close, pairs, offset) of the state that catches `fault`."""
    if fault in ("no hook", "no shortcut"):
        return R.chain(R.CHAIN_N, precision, "random"), R.CHAIN_RADIUS, None, 0
    if fault == "padding label 0":
        st, close, radii = R.sized(precision, "cloud", 513)
        return st, radii[1], close, 0
    if fault == "< instead of <=":
        return R.lattice(13, precision, True), R.LATTICE_TIE, None, 0
    st, close, radii = R.sized(precision, "cloud", 2049)
    return st, radii[2], close, 257


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    planted = set()
    for fault in R.FAULTS:
        st, radius, close, offset = _fault_case(precision, fault)
        want = R.restate(st, radius, precision, close=close)
        assert not R.differs(want, dict(R.fof(st, radius, precision, close=close), passes=want["passes"]))
        got = R.restate(st, radius, precision, fault=fault, close=close, offset=offset)
        found = R.differs(got, want)
        print("fp%d %-50s: %r" % (precision, fault, found))
        assert found, (precision, fault)
        planted.add(fault)
    assert planted == set(R.FAULTS) and len(R.FAULTS) == 8
    # what each of the two iteration faults is seen by: the labels are right, the number of passes is not
    st, radius, close, _ = _fault_case(precision, "no hook")
    want = R.restate(st, radius, precision)
    for fault in ("no hook", "no shortcut"):
        got = R.restate(st, radius, precision, fault=fault)
        assert not R.differs(got, want, passes=False) and got["passes"] > want["passes"], fault


def test_fof_catalogue_agrees_with_a_plain_loop(nbx):
    st, close, radii = R.sized(64, "clustered", 513)
    for radius in radii:
        label = R.fof(st, radius, 64, close=close)["label"]
        for min_members in (1, 2, 10):
            got = nbx.fof_catalogue(label, st["mass"], st["pos_x"], st["pos_y"], st["pos_z"], min_members=min_members)
            want = R.catalogue(label, st["mass"], st["pos_x"], st["pos_y"], st["pos_z"], min_members=min_members)
            assert got["label"].tolist() == [r[0] for r in want] and got["members"].tolist() == [r[1] for r in want]
            assert got["centre"].shape == (len(want), 3) and got["mass"].shape == (len(want),)
            if want:
                assert np.allclose(got["mass"], [r[2] for r in want], rtol=1e-13, atol=0.0)
                assert np.allclose(got["centre"], [r[3] for r in want], rtol=0.0, atol=1e-12)
                assert (np.diff(got["members"]) <= 0).all() and got["members"].min() >= min_members
        assert nbx.fof_catalogue(label, st["mass"], st["pos_x"], st["pos_y"], st["pos_z"], min_members=1)["members"].sum() == 513
    empty = nbx.fof_catalogue(np.arange(4), np.ones(4), np.zeros(4), np.zeros(4), np.zeros(4))  # four singletons, min_members = 2
    assert empty["label"].shape == (0,) and empty["centre"].shape == (0, 3)
