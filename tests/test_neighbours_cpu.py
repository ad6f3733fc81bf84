"""Nearest neighbour and radius count of every body (include/nbx_neighbours.h), the parts that need no GPU: the header and its
three exported symbols, the argument checks that come before the first HIP call, the Python methods and mutual_pairs, the build
files, an audit of the cross-compiled gfx950 code of nbx_neighbours.hip, and the numpy reference tests/neighbours_ref.py, which
must show by itself what the device tests then ask of the library.

Which state catches which planted fault (both precisions; "caught" = neighbours_ref.differs, the comparison of the device tests):
    box(257), radius 0.25: self not masked, padding record not masked (record 257 sits at the origin, inside the box), count
        includes self
    box(2049), radius 0.25: last tile of the last split skipped (it holds body 2048 alone)
    lattice(13), both orders, radius 0.15: ties to the highest j, finish takes the last split on ties (two splits meeting at
        j = 1280, equal candidates from both), last tile of the last split skipped
    lattice(13), radius 0.125, where h2 is bit for bit the face neighbours' r2: < instead of <=
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import neighbours_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_neighbours.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_neighbours_kernels.hpp"
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h", "nbx_field.h")
ENTRY_POINTS = ("nbx_neighbours", "nbx_ensemble_neighbours", "nbx_ragged_neighbours")
NOUN = {"nbx_neighbours": "ctx", "nbx_ensemble_neighbours": "ensemble", "nbx_ragged_neighbours": "ragged ensemble"}


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


OUT3 = "int32_t*, void*, int32_t*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_neighbours.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, double, %s) = nbx_neighbours; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, double, %s) = nbx_ensemble_neighbours; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, double, %s) = nbx_ragged_neighbours; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n' % (OUT3, OUT3, OUT3))
PARAMS = "double r, int32_t* i, void* d, int32_t* w"
UNUSED = "(void)r; (void)i; (void)d; (void)w;"
STUBS = ('#include "nbx_neighbours.h"\n'
         'int nbx_neighbours(nbx_ctx* h, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_neighbours(nbx_ensemble* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_neighbours(nbx_ragged* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "neighbours_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_three_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_neighbours.h")
    assert declared == sorted(ENTRY_POINTS) and set(declared) == set(nbx.NEIGHBOUR_SYMBOLS) and len(nbx.NEIGHBOUR_SYMBOLS) == 3
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "_neighbours" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS) |
                                set(nbx.RAGGED_SYMBOLS) | set(nbx.RAGGED_DIAG_SYMBOLS) | set(nbx.BATCH_ACCEL_SYMBOLS) | set(nbx.KICK_SYMBOLS) |
                                set(nbx.TIMESCALE_SYMBOLS) | set(nbx.FIELD_SYMBOLS))
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (5 if s == "nbx_neighbours" else 7)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = open(os.path.join(ROOT, "include", "nbx_neighbours.h")).read()
    for word in ("Why:", "Definition", "Per-pair arithmetic", "Semantics", "Status, in this order", "Unspecified results", "Deliberately not here",
                 "LOWEST j", "h2 = fma(rT, rT, eps2)", "index = -1", "by a mask", "padding record sits at", "r2 = eps^2",
                 "r2(i, j) and r2(j, i) are the", "if index[i] == j then r2[j] <= r2[i]", "nbx_timescale_t.min_r2",
                 "identifies a mutual pair", "a NULL array is never written", "checked always", "member-major", "end to end", "sliced context",
                 "nbx_commit", "synchronises once", "no atomics", "steps_done", "the state of graph", "2^22", "checked in 64 bits",
                 "before the first HIP call", "NBX_ERR_ALLOC", "groups", "device pointers", "k > 1 neighbours", "neighbour list",
                 "relative velocities", "merging bodies", "hipGraph", "nbody.x", "the same bits", "not finite"):
        assert word in doc, word


def _call(nbx, name, handle, radius, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    args = [radius] + [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in out]
    return f(handle, *args) if name == "nbx_neighbours" else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    out = [np.full(8, -7, dtype=np.int32), np.full(8, -7.25, dtype=np.float64), np.full(8, -7, dtype=np.int32)]
    none3 = [None] * 3
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for radius, o in ((0.25, out), (-1.0, none3), (float("nan"), out)):
        assert _call(nbx, name, None, radius, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. the radius is NaN or negative -- before the range, also where within is not asked for
    for radius in (float("nan"), -1.0, -1e-300, float("-inf")):
        for o in (out, none3, [out[0], out[1], None]):
            assert _call(nbx, name, handle, radius, o, -1, 5) == nbx.NBX_ERR_ARG
            assert err() == name + ": radius is NaN or negative"
    if name != "nbx_neighbours":
        # 3. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for radius in (0.25, 0.0, float("inf")):
                assert _call(nbx, name, handle, radius, out, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 7. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with outputs and without
        assert _call(nbx, name, handle, 0.25, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, 0.0, none3, 0, 0) == nbx.NBX_OK
    else:
        # 5. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for radius, o in ((0.25, out), (0.0, none3), (float("inf"), [None, out[1], None])):
            assert _call(nbx, name, handle, radius, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_neighbours: nbx_upload has not been called"
    assert (out[0] == -7).all() and (out[1] == -7.25).all() and (out[2] == -7).all() and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_is_the_fields_and_its_texts_are_in_the_source():
    """More than 2^22 bodies in one call cannot be made here without a device; the check and its three texts are read off the
    source, between the range check and the upload check."""
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kNbMaxBodies = kFieldMaxPoints;" in hdr
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_neighbours: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kNbMaxBodies" in src and "range_bodies(o, first, count) > kNbMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_neighbours("):]
    order = [batch.index(w) for w in ("is NULL", "bad_radius(", "check_range(", "kNbMaxBodies", "check_uploaded(", "no_output(a)", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_neighbours("):]
    order = [ctx.index(w) for w in ("is NULL", "bad_radius(", "kNbMaxBodies", "->uploaded", "pending_commit", "no_output(a)", "use_device(")]
    assert order == sorted(order)


def test_python_methods_keys_and_mutual_pairs(nbx):
    p = inspect.signature(nbx.Context.neighbours).parameters
    assert list(p) == ["self", "radius"] and p["radius"].default is None
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.neighbours).parameters
        assert list(p) == ["self", "radius", "first", "count"], cls
        assert p["radius"].default is None and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "neighbours")  # groups: deliberately not here
    assert nbx.NEIGHBOUR_KEYS == ("index", "r2", "within") == R.KEYS
    assert not [f for f, _ in nbx.Opts._fields_ if "neighbour" in f or "radius" in f]  # no new nbx_opts field
    for index, want in (([1, 0], [(0, 1)]), ([1, 0, 1], [(0, 1)]), ([1, 2, 0], []), ([-1], []), ([3, 2, 1, 0], [(0, 3), (1, 2)]),
                        ([2, 2, 1, 2, 5, 4], [(1, 2), (4, 5)]), ([], [])):
        got = nbx.mutual_pairs(np.array(index, dtype=np.int32))
        assert got.shape == (len(want), 2) and got.dtype.kind == "i" and [tuple(r) for r in got.tolist()] == want, (index, got)
        assert np.array_equal(got, R.mutual_pairs(np.array(index, dtype=np.int32)))


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_neighbours\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_neighbours\.o: \$\(CSRC\)/nbx_neighbours\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    assert rule
    for dep in (KERNELS, "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_diag_shape.hpp", "nbx_pair.hpp", "include/nbx_neighbours.h",
                "include/nbx_ensemble.h", "include/nbx_ragged.h", "include/nbx.h", "include/nbx_diag.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_neighbours.hip", "include/nbx_neighbours.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_and_reuse_the_shape_rule_and_the_shared_helpers():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_neighbours.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_neighbours.hip", KERNELS):
            assert "neighbour_kernel" not in txt and "nb_body" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    both = re.sub(r"//.*", "", src + kern)
    assert "atomic" not in both
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern  # the field's rule, no new one
    assert "diag_splits" not in both and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("nb_part", "nb_out", "nb_tab"):
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
    out = tmp_path_factory.mktemp("isa") / "nbx_neighbours.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision, with count) of a pair-work kernel, ("finish", precision, None) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)neighbour_kernelI([fd])Lb([01])EEE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64, m.group(3) == "1")
    m = re.search(r"^_ZN3nbx\d+neighbour_finish_kernelI([fd])EE", name)
    if m:
        return ("finish", 32 if m.group(1) == "f" else 64, None)
    return None


def _pair_loops(body, ins):
    """The innermost loop bodies (label ... backward branch) that hold `ins`."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_the_kernels_are_three_kinds_in_two_precisions_with_and_without_the_count_and_the_finish(isa):
    keys = sorted((_key(k) or ("?", k, None) for k in isa), key=str)
    want = [(kind, p, c) for kind in ("context", "ensemble", "ragged") for p in (32, 64) for c in (False, True)] + [("finish", p, None) for p in (32, 64)]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_and_one_tile_of_position_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        kind, precision, _ = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (0 if kind == "finish" else 256 * (16 if precision == 32 else 32)), (name, lds)


def test_the_fp32_pair_loops_are_packed_read_lds_records_whole_and_hold_no_root_and_no_multiply(isa):
    for name, (body, desc, meta) in isa.items():
        kind, precision, count = _key(name)
        if kind == "finish":
            continue
        if precision == 64:
            assert re.search(r"\bv_fma_f64", body) and re.search(r"\bv_add_f64", body) and not re.search(r"\bv_rsq_f64|\bv_mul_f64", body), name
            continue
        loops = _pair_loops(body, "v_pk_fma_f32")
        assert len(loops) == 2, (name, len(loops))  # the masked tile loop and the one without the mask compares
        n_cmp = []
        for loop in loops:
            c = lambda ins: len(re.findall(r"\b%s" % ins, loop))
            records = c(r"ds_(?:read|load)_b128")
            assert records >= 1, name  # one whole record per j
            # per j record the lane's two bodies, i.e. two pairs: 3 packed subtracts and 3 packed fused multiply-adds
            assert c("v_pk_fma_f32") == 3 * records and c("v_pk_add_f32") == 3 * records, (name, records, c("v_pk_fma_f32"), c("v_pk_add_f32"))
            assert c("v_rsq_f32") == 0 and c("v_pk_mul_f32") == 0 and c("v_mul_f32") == 0 and c("v_sqrt") == 0 and c("v_div_") == 0, name
            assert c("v_cndmask_b32") >= 4 * records, name  # per pair a select of the minimum and one of the index
            n_cmp.append(c("v_cmp_") / records)
        # the loop without the mask: one float compare per pair, two with the count; the masked loop has more
        assert min(n_cmp) == (4 if count else 2), (name, n_cmp)
        assert max(n_cmp) > min(n_cmp), (name, n_cmp)


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


@pytest.mark.parametrize("precision", [32, 64])
def test_one_two_and_three_bodies_give_the_closed_forms(precision):
    T = R.DTYPE[precision]
    for f in (R.neighbours, R.restate):
        one = f(_state([(0.5, 0.25, -1.0)], T), 10.0, precision)
        assert one["index"].tolist() == [-1] and one["r2"].tolist() == [np.inf] and one["within"].tolist() == [0]
        two = f(_state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)], T), 2.0, precision)  # 2 apart: h2 = 4 + eps2 is their r2 exactly
        assert two["index"].tolist() == [1, 0] and two["r2"].tolist() == [4.0 + EPS2] * 2 and two["within"].tolist() == [1, 1]
        assert f(_state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)], T), 1.5, precision)["within"].tolist() == [0, 0]
        # a 3-4-5 triangle in the plane z = 2: 0 -(3)- 1 -(4)- 2, 0 -(5)- 2; and a body on top of body 0
        tri = f(_state([(0.0, 0.0, 2.0), (3.0, 0.0, 2.0), (3.0, 4.0, 2.0)], T), 4.5, precision)
        assert tri["index"].tolist() == [1, 0, 1] and tri["r2"].tolist() == [9.0 + EPS2, 9.0 + EPS2, 16.0 + EPS2]
        assert tri["within"].tolist() == [1, 2, 1]
        same = f(_state([(1.0, 1.0, 1.0), (4.0, 1.0, 1.0), (1.0, 1.0, 1.0)], T), 0.0, precision)
        assert same["index"].tolist() == [2, 0, 0] and same["r2"].tolist() == [EPS2, 9.0 + EPS2, EPS2]  # distinct bodies at one position count
        assert same["within"].tolist() == [1, 0, 1]  # h2 == eps2 == their r2
        assert R.mutual_pairs(same["index"]).tolist() == [[0, 2]] and R.mutual_pairs(tri["index"]).tolist() == [[0, 1]]


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_follows_the_lowest_index_rule_in_both_orders(precision, perm):
    k = R.LATTICE_K
    st = R.lattice(k, precision, perm)
    for c in R.POS:
        assert np.array_equal(st[c].astype(np.float32).astype(np.float64), st[c].astype(np.float64))  # exact in fp32
    index, faces = R.lattice_expected(k, perm)
    assert sorted(set(faces.tolist())) == [3, 4, 5, 6] and (faces == 6).sum() == (k - 2) ** 3
    for f in (R.neighbours, R.restate):
        got = f(st, R.LATTICE_RADIUS, precision)
        assert np.array_equal(got["index"], index) and np.array_equal(got["within"], faces)
        assert (got["r2"] == 1.0 / 64 + EPS2).all()  # the same bits for every body
        assert np.array_equal(f(st, R.LATTICE_TIE_RADIUS, precision)["within"], faces)  # <= at the exact tie
    assert R.h2_of(R.LATTICE_TIE_RADIUS, precision) == 1.0 / 64 + EPS2
    if not perm:
        assert index[0] == 1 and index[1] == 0 and index[k * k * k - 1] == k * k * k - 1 - k * k and index[1300] == 1131
        assert field_splits(k ** 3) == (2, 1280)


def field_splits(n):
    """(splits, first record of the second split) of field_shape(n, n)."""
    from field_ref import field_shape
    _, _, splits, per = field_shape(n, n)
    return splits, per * R.TILE


@pytest.mark.parametrize("precision", [32, 64])
def test_the_states_of_the_device_tests_have_no_ambiguous_body_and_the_restatement_is_the_plain_argmin(precision):
    mean = {}
    for n in R.SIZES:
        for make in (R.box, R.shifted):
            st = make(n, precision)
            bad = R.ambiguity(st, R.RADIUS, precision)
            ref = R.neighbours(st, R.RADIUS, precision)
            print("fp%d %s(%d): ambiguous nearest neighbours %d, ambiguous counts %d, mean count %.1f, mutual pairs %d"
                  % (precision, make.__name__, n, bad[0], bad[1], ref["within"].mean(), len(R.mutual_pairs(ref["index"]))))
            assert bad == (0, 0), (precision, make.__name__, n, bad)
            got = R.restate(st, R.RADIUS, precision)
            assert all(np.array_equal(got[k], ref[k]) for k in R.KEYS), (precision, make.__name__, n)
            assert (ref["r2"][ref["index"]] <= ref["r2"]).all()  # if index[i] == j then r2[j] <= r2[i]
            mean[make.__name__, n] = ref["within"].mean()
        assert abs(mean["box", n] - mean["shifted", n]) < 0.5
    for st in [R.member(n, precision) for n in R.RAGGED_SIZES] + [R.reversed_box(n, precision) for n in (257, 2049)]:  # the batch tests' other states
        assert R.ambiguity(st, R.RADIUS, precision) == (0, 0), len(st["mass"])
    assert 1.0 < mean["box", 257] < 3.0 and 12.0 < mean["box", 2049] < 17.0 and 25.0 < mean["box", 4097] < 33.0
    assert (field_splits(257)[0], field_splits(2049), field_splits(4097)) == (1, (2, 1280), (4, 1280))  # the shapes the sizes stand for
    # the ambiguity measure itself: two partners at distances that differ by 8 u are ambiguous, by 64 u are not
    u = R.U[precision]
    for rel, want in ((8 * u, 1), (64 * u, 0)):
        st = _state([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-(1.0 + rel), 0.0, 0.0), (0.0, 30.0, 0.0), (0.0, 33.0, 0.0)], np.float64)
        assert R.ambiguity(st, 0.1, precision)[0] == want, rel
    st = _state([(0.0, 0.0, 0.0), (0.25 * (1 + 2 * u), 0.0, 0.0)], np.float64)
    assert R.ambiguity(st, 0.25, precision)[1] == 2 and R.ambiguity(st, 0.3, precision)[1] == 0


FAULT_CASES = (
    (("box", 257, False), R.RADIUS, ("self not masked", "padding record not masked", "count includes self")),
    (("box", 2049, False), R.RADIUS, ("last tile of the last split skipped",)),  # body 2048 alone: within 0.25 of some fifteen others
    (("lattice", R.LATTICE_K, False), R.LATTICE_RADIUS, ("ties to the highest j", "finish takes the last split on ties",
                                                         "last tile of the last split skipped")),
    (("lattice", R.LATTICE_K, True), R.LATTICE_RADIUS, ("ties to the highest j", "finish takes the last split on ties")),
    (("lattice", R.LATTICE_K, False), R.LATTICE_TIE_RADIUS, ("< instead of <=",)),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    planted = set()
    for (family, size, perm), radius, faults in FAULT_CASES:
        st = R.box(size, precision) if family == "box" else R.lattice(size, precision, perm)
        want = R.neighbours(st, radius, precision)
        assert not R.differs(R.restate(st, radius, precision), want, precision)
        for fault in faults:
            got = R.restate(st, radius, precision, fault=fault)
            print("fp%d %s(%d%s) radius %g, %-38s: %d indices, %d counts differ" % (precision, family, size, ", permuted" if perm else "", radius, fault,
                  (got["index"] != want["index"]).sum(), (got["within"] != want["within"]).sum()))
            assert R.differs(got, want, precision), (precision, family, size, perm, fault)
            planted.add(fault)
    assert planted == set(R.FAULTS)
    # what each fault is seen by
    st = R.box(257, precision)
    want = R.neighbours(st, R.RADIUS, precision)
    pad = R.restate(st, R.RADIUS, precision, fault="padding record not masked")
    assert (pad["index"] == 257).any() and (pad["within"] > want["within"]).any()  # the origin is somebody's nearest neighbour
    own = R.restate(st, R.RADIUS, precision, fault="self not masked")
    assert (own["index"] == np.arange(257)).all() and (own["r2"] == EPS2).all()
    assert not (R.restate(st, R.RADIUS, precision, fault="ties to the highest j")["index"] != want["index"]).any()  # no ties in the box: the lattice is needed
