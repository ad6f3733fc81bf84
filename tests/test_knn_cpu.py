"""The k nearest neighbours of every body (include/nbx_knn.h), the parts that need no GPU: the header and its three exported
symbols, the argument checks that come before the first HIP call, the Python methods and the density helpers, the build files,
an audit of the cross-compiled gfx950 code of nbx_knn.hip, and the numpy reference tests/knn_ref.py, which must show by itself
what the device tests then ask of the library.

Which state catches which planted fault (both precisions; "caught" = knn_ref.differs, the comparison of the device tests):
    box(257), k = 6: self not masked, padding record not masked (record 257 sits at the origin, inside the box)
    box(2049), k = 6: last tile of the last split skipped (it holds body 2048 alone), displaced K-th entry lost, row not sorted
        after merge (two splits: most rows draw from both)
    lattice(13), both orders, k = 6 and 16, every index compared: equal r2 displaces, merge prefers the later split on ties (two
        splits meeting at j = 1280, equal candidates from both)
    member(5), k = 6: no fill when n - 1 < k
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import knn_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2
from field_ref import field_shape

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_knn.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_knn_kernels.hpp"
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h", "nbx_field.h", "nbx_neighbours.h", "nbx_paircount.h", "nbx_tracers.h")
ENTRY_POINTS = ("nbx_knn", "nbx_ensemble_knn", "nbx_ragged_knn")
NOUN = {"nbx_knn": "ctx", "nbx_ensemble_knn": "ensemble", "nbx_ragged_knn": "ragged ensemble"}
OTHER_TUPLES = ("SYMBOLS", "DIAG_SYMBOLS", "ENSEMBLE_SYMBOLS", "ENSEMBLE_DIAG_SYMBOLS", "RAGGED_SYMBOLS", "RAGGED_DIAG_SYMBOLS",
                "BATCH_ACCEL_SYMBOLS", "KICK_SYMBOLS", "TIMESCALE_SYMBOLS", "FIELD_SYMBOLS", "NEIGHBOUR_SYMBOLS", "PAIRCOUNT_SYMBOLS",
                "TRACER_SYMBOLS")
FORBIDDEN = ("neighbour_kernel", "nb_body", "field_kernel", "field_body", "timescale_kernel", "tracer_kernel", "tracer_body",
             "tracer_update_kernel")
CAPACITIES = (4, 8, 16)


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


OUT2 = "int32_t*, void*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_knn.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, int32_t, %s) = nbx_knn; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, int32_t, %s) = nbx_ensemble_knn; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, int32_t, %s) = nbx_ragged_knn; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL && NBX_KNN_MAX == 16) ? NBX_ABI_VERSION - 1 : 1; }\n'
           % (OUT2, OUT2, OUT2))
PARAMS = "int32_t k, int32_t* i, void* d"
UNUSED = "(void)k; (void)i; (void)d;"
STUBS = ('#include "nbx_knn.h"\n'
         'int nbx_knn(nbx_ctx* h, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_knn(nbx_ensemble* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_knn(nbx_ragged* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "knn_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_three_symbols_exported_and_apart_from_every_other_tuple(nbx):
    declared = _declared("nbx_knn.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.KNN_SYMBOLS) == ENTRY_POINTS and len(nbx.KNN_SYMBOLS) == 3
    assert nbx.KNN_KEYS == ("index", "r2") == R.KEYS and nbx.KNN_MAX == 16 == R.KNN_MAX
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "_knn" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in OTHER_TUPLES:
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (4 if s == "nbx_knn" else 6)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = open(os.path.join(ROOT, "include", "nbx_knn.h")).read()
    assert "#define NBX_KNN_MAX 16" in doc
    for word in ("Why:", "Definition", "Per-pair arithmetic", "Consequences", "Semantics", "Status, in this order", "Unspecified results",
                 "Deliberately not here", "lexicographic order (r2 bits, j)", "body-major", "index = -1, r2 = +infinity", "all fill",
                 "by a mask", "padding record sits at", "r2 = eps^2", "fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))",
                 "bit for bit nbx_neighbours' index and r2", "the first k columns of the result for any k' > k", "non-decreasing in r2",
                 "strictly increasing in j among equal r2", "#(r2[i, :] <= h2) == min(within[i], k)", "Nothing is summed in floating point",
                 "the same bits", "compiled list capacity", "a NULL array is never written", "k is checked always", "member-major", "end to end",
                 "sliced context", "nbx_commit", "synchronises once", "One pair-work launch, one finish launch and one read-back", "no atomics",
                 "steps_done", "*_timed / *_ms_total", "kinetic-energy partials", "the state of graph", "k < 1 or k > NBX_KNN_MAX",
                 "checked even when both outputs are NULL", "checked in 64 bits", "2^22", "scaled by the row width", "1M bodies: k <= 4",
                 "names the first such member", "before the first HIP call", "NBX_ERR_ALLOC", "not finite", "k ln(n / k)", "decreasing distance",
                 "groups", "device pointers", "k > 16", "variable-length neighbour lists", "an i range for a", "a radius cut-off",
                 "mass-weighted selection", "hipGraph", "nbody.x"):
        assert word in doc, word
    old = open(os.path.join(ROOT, "include", "nbx_neighbours.h")).read()
    assert "k > 1 neighbours" in old  # the gap this header fills, named by the one it extends


def _call(nbx, name, handle, k, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    args = [k] + [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in out]
    return f(handle, *args) if name == "nbx_knn" else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    out = [np.full(64, -7, dtype=np.int32), np.full(64, -7.25, dtype=np.float64)]
    none2 = [None] * 2
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for k, o in ((6, out), (0, none2), (17, out)):
        assert _call(nbx, name, None, k, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. k outside [1, NBX_KNN_MAX] -- before the range, also where nothing is asked for
    for k in (0, -1, 17, 2 ** 31 - 1, -2 ** 31):
        for o in (out, none2, [out[0], None]):
            assert _call(nbx, name, handle, k, o, -1, 5) == nbx.NBX_ERR_ARG
            assert err() == name + ": k is outside [1, 16]"
    if name != "nbx_knn":
        # 3. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for k in (1, 6, 16):
                assert _call(nbx, name, handle, k, out, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 7. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with outputs and without
        assert _call(nbx, name, handle, 6, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, 16, none2, 0, 0) == nbx.NBX_OK
    else:
        # 5. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for k, o in ((6, out), (1, none2), (16, [None, out[1]])):
            assert _call(nbx, name, handle, k, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_knn: nbx_upload has not been called"
    assert (out[0] == -7).all() and (out[1] == -7.25).all() and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_is_the_fields_scaled_by_k_and_its_texts_are_in_the_source():
    """More than 2^22 entries in one call cannot be made here without a device; the check and its three texts are read off the
    source, between the range check and the upload check."""
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kKnnMaxEntries = kFieldMaxPoints;" in hdr and "constexpr int kKnnMax = 16;" in hdr
    assert "kKnnMax == NBX_KNN_MAX" in src
    assert '"nbx_knn: n * k exceeds 4194304"' in src and '"count * n * k exceeds"' in src and '"the bodies of the range times k exceed"' in src
    assert "(long long)c->n * (long long)k > kKnnMaxEntries" in src and "range_bodies(o, first, count) * (long long)k > kKnnMaxEntries" in src
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies is the shared one; the two nouns above are this call's own
    assert "long long range_bodies(" in shared and "long long range_bodies(" not in src and "entries_noun(o)" in src
    batch = src[src.index("int batch_knn("):]
    order = [batch.index(w) for w in ("is NULL", "bad_k(", "check_range(", "kKnnMaxEntries", "check_uploaded(", "no_output(a)", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_knn("):]
    order = [ctx.index(w) for w in ("is NULL", "bad_k(", "kKnnMaxEntries", "->uploaded", "pending_commit", "no_output(a)", "use_device(")]
    assert order == sorted(order)


def test_python_methods_keys_and_helpers_are_as_specified(nbx):
    p = inspect.signature(nbx.Context.knn).parameters
    assert list(p) == ["self", "k"] and p["k"].default is inspect.Parameter.empty
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.knn).parameters
        assert list(p) == ["self", "k", "first", "count"], cls
        assert p["k"].default is inspect.Parameter.empty and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "knn")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "knn" in f]  # no new nbx_opts field
    assert list(inspect.signature(nbx.local_density).parameters) == ["knn", "mass"]
    assert list(inspect.signature(nbx.density_centre).parameters) == ["x", "y", "z", "rho"]
    one = {"index": np.zeros((4, 1), dtype=np.int32), "r2": np.ones((4, 1))}
    with pytest.raises(nbx.NbxError):
        nbx.local_density(one, np.ones(4))  # needs k >= 2


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_knn\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_knn\.o: \$\(CSRC\)/nbx_knn\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    assert rule
    for dep in (KERNELS, "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_diag_shape.hpp", "nbx_pair.hpp", "include/nbx_knn.h",
                "include/nbx_ensemble.h", "include/nbx_ragged.h", "include/nbx.h", "include/nbx_diag.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_knn.hip", "include/nbx_knn.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_reuse_the_shape_rule_and_keep_to_the_naming_rules():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_knn.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_knn.hip", KERNELS):
            assert "knn_kernel" not in txt and "knn_body" not in txt and "knn_insert" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    both = re.sub(r"//.*", "", src + kern)
    for word in FORBIDDEN:
        assert word not in both, word
    assert not re.search(r'#include "nbx_(?!knn)\w+_kernels\.hpp"', both)  # no other feature's kernels
    assert "atomic" not in both
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern  # the field's rule, no new one
    assert "diag_splits" not in both and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)
    assert "fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())))" in kern  # r2 restated, not shared
    assert "__any(" in kern  # the wave-uniform branch around the insertion
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("knn_part", "knn_out", "knn_tab"):
        assert re.search(r"void\* %s = nullptr;" % field, obj) and "o->%s" % field in obj[obj.index("inline void batch_release"):], field
    assert sorted(set(R.capacity(k) for k in range(1, 17))) == list(CAPACITIES)
    assert "return k <= 4 ? 4 : k <= 8 ? 8 : 16;" in kern  # knn_ref.capacity is the kernels' rule


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
    out = tmp_path_factory.mktemp("isa") / "nbx_knn.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision, capacity) of a kernel; kind "finish" for the finish kernel."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)knn_kernelI([fd])Li(\d+)EEE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64, int(m.group(3)))
    m = re.search(r"^_ZN3nbx\d+knn_finish_kernelI([fd])Li(\d+)EEE", name)
    if m:
        return ("finish", 32 if m.group(1) == "f" else 64, int(m.group(2)))
    return None


def test_every_kind_precision_and_capacity_is_compiled(isa):
    keys = sorted((_key(k) or ("?", k, None) for k in isa), key=str)
    want = [(kind, p, c) for kind in ("context", "ensemble", "ragged", "finish") for p in (32, 64) for c in CAPACITIES]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_and_one_tile_of_position_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name  # the lists never leave the registers
        kind, precision, _ = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (0 if kind == "finish" else 256 * (16 if precision == 32 else 32)), (name, lds)


def test_the_pair_work_is_packed_in_fp32_reads_records_whole_and_branches_uniformly_around_the_insertion(isa):
    for name, (body, desc, meta) in isa.items():
        kind, precision, cap = _key(name)
        if kind == "finish":
            continue
        c = lambda ins: len(re.findall(r"\b%s" % ins, body))
        # no root and no packed multiply anywhere (a ragged kernel divides integers for field_shape: plain multiplies may occur)
        assert c("v_rsq_") == 0 and c("v_sqrt") == 0 and c("v_pk_mul_f32") == 0 and c("v_mul_f64") == 0, name
        if precision == 64:
            assert c("v_fma_f64") >= 3 and c("v_add_f64") >= 3, name
            continue
        records = c(r"ds_(?:read|load)_b128")
        assert records >= 2, name  # the masked tile loop and the one without the mask compares
        # per j record the lane's two bodies, i.e. two pairs: 3 packed subtracts and 3 packed fused multiply-adds
        assert c("v_pk_fma_f32") == 3 * records and c("v_pk_add_f32") == 3 * records, (name, records, c("v_pk_fma_f32"), c("v_pk_add_f32"))
        # per j record one branch on the OR over the wave of the two bodies' compares against their K-th values
        uniform = len(re.findall(r"v_cmp_lt_f32_e64 s\[\d+:\d+\], v\d+, v\d+\n\s*v_cmp_lt_f32_e64 s\[\d+:\d+\], v\d+, v\d+\n\s*s_or_b64 vcc, s\[\d+:\d+\], "
                                 r"s\[\d+:\d+\]\n\s*s_cbranch_vccn?z ", body))
        print("%s: %d records, %d uniform branches" % (name, records, uniform))
        assert uniform >= records // 2, (name, records, uniform)  # at least the loop without the mask


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _state(xs, T):
    n = len(xs)
    st = {f: np.zeros(n, dtype=T) for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
    for f, col in zip(R.POS, zip(*xs)):
        st[f] = np.array(col, dtype=T)
    st["mass"] = np.ones(n, dtype=T)
    return st


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in R.KEYS)


@pytest.mark.parametrize("precision", [32, 64])
def test_small_systems_give_the_closed_forms_and_exact_fill(precision):
    T = R.DTYPE[precision]
    inf = np.inf
    for f in (R.knn, R.restate):
        one = f(_state([(0.5, 0.25, -1.0)], T), 3, precision)
        assert one["index"].tolist() == [[-1, -1, -1]] and one["r2"].tolist() == [[inf, inf, inf]]
        two = f(_state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)], T), 2, precision)
        assert two["index"].tolist() == [[1, -1], [0, -1]] and two["r2"].tolist() == [[4.0 + EPS2, inf]] * 2
        # a 3-4-5 triangle in the plane z = 2: 0 -(3)- 1 -(4)- 2, 0 -(5)- 2
        tri = f(_state([(0.0, 0.0, 2.0), (3.0, 0.0, 2.0), (3.0, 4.0, 2.0)], T), 2, precision)
        assert tri["index"].tolist() == [[1, 2], [0, 2], [1, 0]]
        assert tri["r2"].tolist() == [[9.0 + EPS2, 25.0 + EPS2], [9.0 + EPS2, 16.0 + EPS2], [16.0 + EPS2, 25.0 + EPS2]]
        # distinct bodies at one position count, with r2 = eps^2; equal r2 in ascending j
        same = f(_state([(1.0, 1.0, 1.0), (4.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)], T), 3, precision)
        assert same["index"].tolist() == [[2, 3, 1], [0, 2, 3], [0, 3, 1], [0, 2, 1]]
        assert same["r2"][0].tolist() == [EPS2, EPS2, 9.0 + EPS2]
        for n in (1, 2, 5, 17):
            st = R.member(n, precision)
            got = f(st, 16, precision)
            have = min(16, n - 1)
            assert (got["index"][:, have:] == -1).all() and np.isposinf(got["r2"][:, have:]).all()
            assert (got["index"][:, :have] >= 0).all() and np.isfinite(got["r2"][:, :have]).all()


@pytest.mark.parametrize("precision", [32, 64])
def test_the_restatement_is_the_plain_definition_and_the_states_are_as_unambiguous_as_stated(precision):
    """restate without a fault equals knn on every state of the device tests, at k = 16 and -- through another capacity -- at
    k = 6; a result for k is the prefix of the result for 16.  Ambiguous bodies: none for k in {1, 6, 8} anywhere, none for k = 16
    except one on shifted(4097) in fp32, the state the device test holds to (a) and (b) only at k = 16."""
    states = [(make.__name__, n, make(n, precision)) for n in R.SIZES for make in (R.box, R.shifted)]
    states += [("member", n, R.member(n, precision)) for n in R.RAGGED_SIZES]
    states += [("lattice perm=%d" % perm, R.N.LATTICE_K ** 3, R.lattice(R.N.LATTICE_K, precision, perm)) for perm in (False, True)]
    for name, n, st in states:
        want = R.knn(st, 16, precision)
        assert _same(R.restate(st, 16, precision), want), (precision, name, n)
        six = R.restate(st, 6, precision)  # through another capacity: the prefix of the result for 16
        assert np.array_equal(six["index"], want["index"][:, :6]) and np.array_equal(six["r2"], want["r2"][:, :6]), (precision, name, n)
        if n <= 513:
            for k in (1, 6, 8):
                pre = R.knn(st, k, precision)
                assert np.array_equal(pre["index"], want["index"][:, :k]) and np.array_equal(pre["r2"], want["r2"][:, :k]), (name, n, k)
        fin = np.isfinite(want["r2"])
        assert (np.diff(np.where(fin, want["r2"], 1e300), axis=1) >= 0).all()  # rows ascend
        if name.startswith("lattice"):
            assert not R.differs(want, want, st, precision, exact=True)
            continue
        gap = R.first_gap(st, precision)
        amb = {k: R.ambiguous(st, k, precision, gap) for k in R.KS}
        print("fp%d %s(%d): ambiguous bodies %r" % (precision, name, n, amb))
        assert [amb[k] for k in (1, 6, 8)] == [0, 0, 0], (precision, name, n, amb)
        assert amb[16] == (1 if (precision, name, n) == (32, "shifted", 4097) else 0), (precision, name, n, amb)
        assert not R.differs(want, want, st, precision, gap=gap)
    for n in (257, 2049, 4097):
        assert R.ambiguous(R.reversed_box(n, precision), 16, precision) == 0, n  # none at 16: none at any smaller k
    assert (field_shape(257, 257)[2], field_shape(2049, 2049)[2:], field_shape(4097, 4097)[2:]) == (1, (2, 5), (4, 5))
    assert field_shape(33 ** 3, 33 ** 3) == (71, 141, 15, 10)  # lattice(33): 71 columns x 15 splits
    # the ambiguity measure itself: two partners at distances that differ by 8 u are ambiguous, by 64 u are not -- at every gap
    u = R.U[precision]
    for rel, want in ((8 * u, 1), (64 * u, 0)):
        st = _state([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (-(1.0 + rel), 0.0, 0.0), (0.0, 30.0, 0.0), (0.0, 33.0, 0.0), (0.0, 37.0, 0.0)],
                    np.float64)
        assert int(R.ambiguous_mask(st, 2, precision)[0]) == want, rel  # the gap between the 2nd and the 3rd: k + 1 values count
        assert int(R.ambiguous_mask(st, 1, precision)[0]) == 0, rel


FAULT_CASES = (
    (("box", 257, False), 6, False, ("self not masked", "padding record not masked")),
    (("box", 2049, False), 6, False, ("last tile of the last split skipped", "displaced K-th entry lost", "row not sorted after merge")),
    (("lattice", R.N.LATTICE_K, False), 6, True, ("equal r2 displaces", "merge prefers the later split on ties")),
    (("lattice", R.N.LATTICE_K, True), 16, True, ("equal r2 displaces", "merge prefers the later split on ties", "displaced K-th entry lost")),
    (("member", 5, False), 6, False, ("no fill when n - 1 < k",)),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    planted = set()
    for (family, size, perm), k, exact, faults in FAULT_CASES:
        st = R.lattice(size, precision, perm) if family == "lattice" else R.box(size, precision) if family == "box" else R.member(size, precision)
        want = R.knn(st, k, precision)
        assert not R.differs(R.restate(st, k, precision), want, st, precision, exact=exact)
        for fault in faults:
            got = R.restate(st, k, precision, fault=fault)
            found = R.differs(got, want, st, precision, exact=exact)
            print("fp%d %s(%d%s) k = %d, %-40s: %r" % (precision, family, size, ", permuted" if perm else "", k, fault, found))
            assert found, (precision, family, size, perm, fault)
            planted.add(fault)
    assert planted == set(R.FAULTS)
    # what each fault is seen by
    st = R.box(257, precision)
    own = R.restate(st, 6, precision, fault="self not masked")
    assert (own["index"][:, 0] == np.arange(257)).all() and (own["r2"][:, 0] == EPS2).all()
    assert (R.restate(st, 6, precision, fault="padding record not masked")["index"] == 257).any()  # the origin is somebody's neighbour
    assert _same(R.restate(st, 6, precision, fault="equal r2 displaces"), R.knn(st, 6, precision))  # no ties in the box: the lattice is needed


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattices_closed_form_is_the_plain_definition(precision, perm):
    kk = R.N.LATTICE_K
    st = R.lattice(kk, precision, perm)
    for k in (6, 8, 16):
        want = R.knn(st, k, precision)
        exp = R.lattice_expected(kk, k, precision, perm)
        assert np.array_equal(exp["index"], want["index"]), (k, np.nonzero((exp["index"] != want["index"]).any(axis=1))[0][:8])
        assert np.array_equal(exp["d2"] / 64.0 + EPS2, want["r2"])  # fp64 holds d^2 / 64 + eps2 as the reference adds it
        assert (np.abs(exp["r2"] - want["r2"]) <= 3 * R.U[precision] * want["r2"]).all()  # the class's bits in T: three fma, a rounding of at most u each
    assert R.lattice_expected(kk, 16, precision, perm)["d2"].max() == 5  # the corners: 3 + 3 + 1 + 3 + 6 partners
    # every offset of [-2, 2]^3 gives its class's bits, whatever coordinate holds which component
    for a in range(-2, 3):
        for b in range(-2, 3):
            for c in range(-2, 3):
                d2 = a * a + b * b + c * c
                if 0 < d2 <= 5:
                    assert R.lattice_r2_of_offset((a, b, c), precision) == R.lattice_class_r2(d2, precision), (a, b, c)
    assert len({R.lattice_class_r2(d, precision) for d in range(1, 6)}) == 5


# ---------------------------------------------------------------------------------------------------------------------------
# the host helpers
# ---------------------------------------------------------------------------------------------------------------------------
def test_local_density_and_density_centre_agree_with_a_plain_loop(nbx):
    st = R.box(257, 64)
    for k in (2, 6, 16):
        res = R.knn(st, k, 64)
        rho = nbx.local_density(res, st["mass"])
        want = R.local_density(res, st["mass"])
        assert rho.dtype == np.float64 and rho.shape == (257,) and (rho > 0).all()
        assert np.allclose(rho, want, rtol=1e-13, atol=0.0)
        centre, core = nbx.density_centre(st["pos_x"], st["pos_y"], st["pos_z"], rho)
        wc, wr = R.density_centre(st["pos_x"], st["pos_y"], st["pos_z"], want)
        assert centre.shape == (3,) and np.allclose(centre, wc, rtol=0, atol=1e-13) and abs(core - wr) <= 1e-13 * wr
    few = R.knn(R.member(5, 64), 6, 64)  # rows with fill give 0
    assert nbx.local_density(few, np.ones(5)).tolist() == [0.0] * 5 == R.local_density(few, np.ones(5)).tolist()
    twin = R.knn(_state([(1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (2.0, 1.0, 1.0)], np.float64), 2, 64)
    assert nbx.local_density(twin, np.ones(4)).tolist()[:3] == [0.0] * 3  # the k-th neighbour sits on the body: d_k = 0


def test_the_lattice_interior_has_the_closed_form_density_and_the_helpers_are_translation_covariant(nbx):
    kk = R.N.LATTICE_K
    st = R.lattice(kk, 64)
    n = kk ** 3
    m = 0.375
    mass = np.full(n, m)
    res = R.knn(st, 6, 64)
    rho = nbx.local_density(res, mass)
    site = np.arange(n)
    interior = np.ones(n, dtype=bool)
    for c in (site // (kk * kk), (site // kk) % kk, site % kk):
        interior &= (c > 0) & (c < kk - 1)
    assert interior.sum() == (kk - 2) ** 3
    want = 5 * m / (4.0 / 3.0 * np.pi * (1.0 / 8) ** 3)  # (k - 1) m / (4/3 pi d_6^3), d_6 = 1/8: the six face neighbours
    assert np.allclose(rho[interior], want, rtol=1e-12, atol=0.0)
    assert (rho[~interior] < want).all()  # a face, edge or corner site reaches further for its sixth partner
    centre, core = nbx.density_centre(st["pos_x"], st["pos_y"], st["pos_z"], rho)
    assert np.abs(centre).max() <= 1e-13 and core > 0  # the lattice is symmetric about the origin
    shift = (8.0, -16.0, 4.0)  # exact in the lattice's coordinates: the same r2 bits
    moved = dict(st)
    for f, s in zip(R.POS, shift):
        moved[f] = st[f] + s
    res2 = R.knn(moved, 6, 64)
    assert np.array_equal(res2["index"], res["index"])
    rho2 = nbx.local_density(res2, mass)
    assert np.allclose(rho2, rho, rtol=1e-9, atol=0.0)
    c2, core2 = nbx.density_centre(moved["pos_x"], moved["pos_y"], moved["pos_z"], rho2)
    assert np.allclose(c2 - np.array(shift), centre, rtol=0, atol=1e-9) and abs(core2 - core) <= 1e-9 * core
