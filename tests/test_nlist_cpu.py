"""The neighbour lists (include/nbx_nlist.h) without a device: the header and its symbols, every status that comes before the first
HIP call, the scan's sizes through a C++ driver, the compiled gfx950 code of the translation unit, and the reference
tests/nlist_ref.py on its own -- the restatement of the scheme is the plain definition on the case table of the device tests, no
case of that table is ambiguous under the 8 u window, and every fault the restatement can plant is caught by the comparison the
device tests use (nlist_ref.differs)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import nlist_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_nlist.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_nlist_kernels.hpp"
SHAPE = "nbx_nlist_shape.hpp"
ENTRY_POINTS = ("nbx_nlist", "nbx_ensemble_nlist", "nbx_ragged_nlist")
NOUN = {"nbx_nlist": "ctx", "nbx_ensemble_nlist": "ensemble", "nbx_ragged_nlist": "ragged ensemble"}
OTHER_TUPLES = ("SYMBOLS", "DIAG_SYMBOLS", "ENSEMBLE_SYMBOLS", "ENSEMBLE_DIAG_SYMBOLS", "RAGGED_SYMBOLS", "RAGGED_DIAG_SYMBOLS",
                "BATCH_ACCEL_SYMBOLS", "KICK_SYMBOLS", "TIMESCALE_SYMBOLS", "FIELD_SYMBOLS", "NEIGHBOUR_SYMBOLS", "PAIRCOUNT_SYMBOLS",
                "TRACER_SYMBOLS", "KNN_SYMBOLS", "FOF_SYMBOLS", "BINARIES_SYMBOLS", "TIDAL_SYMBOLS", "CLUMPS_SYMBOLS")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


OUT = "int64_t, int64_t*, int32_t*, void*, int64_t*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_nlist.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, double, %s) = nbx_nlist; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, double, %s) = nbx_ensemble_nlist; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, double, %s) = nbx_ragged_nlist; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n' % (OUT, OUT, OUT))
PARAMS = "double r, int64_t cap, int64_t* o, int32_t* i, void* d, int64_t* t"
UNUSED = "(void)r; (void)cap; (void)o; (void)i; (void)d; (void)t;"
STUBS = ('#include "nbx_nlist.h"\n'
         'int nbx_nlist(nbx_ctx* h, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_nlist(nbx_ensemble* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_nlist(nbx_ragged* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "nlist_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_three_symbols_exported_and_the_header_carries_the_contract(nbx):
    declared = _declared("nbx_nlist.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.NLIST_SYMBOLS) == ENTRY_POINTS and nbx.NLIST_KEYS == R.KEYS
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "nbx_nlist.h":
            assert not set(declared) & set(_declared(h)), h
            assert "_nlist" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in OTHER_TUPLES:
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (7 if s == "nbx_nlist" else 9)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_nlist.h")).read())  # the comment as running text
    # the definition
    for word in ("Why:", "Definition", "r2 = fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))", "h2        = fma(rT, rT, eps2)", "j != i with r2(i, j) <= h2",
                 "ASCENDING j", "by a mask", "Two DISTINCT bodies at one position count", "r2 = eps^2", "MEMBER-LOCAL", "member-major", "end to end",
                 "offsets[0] = 0", "offsets[bodies] = *total", "offsets run across the members"):
        assert word in doc, word
    # the protocol
    for word in ("ALWAYS written", "if and only if *total <= capacity", "are not touched", "returns NBX_OK", "calls again",
                 "capacity == 0 with index and r2 both NULL is the counting call", "a NULL array is never written"):
        assert word in doc, word
    # the consequences
    for word in ("equals nbx_neighbours' within[b]", "twice nbx_paircount", "i in list(j), with the same r2 bits", "smallest (r2, j)",
                 "first within[i] columns of nbx_knn(k)", "nbx_fof's partition", "Nothing is summed in floating point", "the same bits",
                 "sliced context", "returns the whole context's lists"):
        assert word in doc, word
    # the status order
    order = [doc.index(w) for w in ("Status, in this order", "the handle is NULL", "radius is NaN or negative", "capacity < 0 or capacity > 2^28",
                                    "at or below 3 GiB", "capacity > 0 with index and r2 both NULL, or offsets or total NULL", "leave [0, members)",
                                    "exceed 2^22", "not uploaded", "awaiting nbx_commit", "count == 0: offsets[0] = 0 and *total = 0", "NBX_ERR_ALLOC",
                                    "Every check but the last comes before the first HIP call")]
    assert order == sorted(order)
    # semantics and what is not there
    for word in ("ordered on the object's stream", "reads the current position buffer only", "never by capacity", "freed with the object",
                 "No atomics", "no kernel waits for another workgroup", "steps_done", "the state of graph", "Deliberately not here", "groups",
                 "device pointers", "a radius per body", "half lists", "velocities in the list", "merging bodies", "not finite"):
        assert word in doc, word
    # the gap, named by the three headers this one answers
    assert "a neighbour list (variable length)" in open(os.path.join(ROOT, "include", "nbx_neighbours.h")).read()
    assert "variable-length neighbour lists" in re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_knn.h")).read())


def _call(nbx, name, handle, radius, capacity, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    args = [radius, capacity] + [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in out]
    return f(handle, *args) if name == "nbx_nlist" else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    offsets, total = np.full(8, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
    index, r2 = np.full(8, -7, dtype=np.int32), np.full(8, -7.25, dtype=np.float64)
    full = [offsets, index, r2, total]
    counting = [offsets, None, None, total]
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for radius, cap, o in ((0.25, 8, full), (-1.0, -1, [None] * 4), (float("nan"), 2 ** 40, counting)):
        assert _call(nbx, name, None, radius, cap, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. the radius is NaN or negative -- before the capacity and the arrays
    for radius in (float("nan"), -1.0, -1e-300, float("-inf")):
        for cap, o in ((8, full), (-1, full), (8, [None] * 4)):
            assert _call(nbx, name, handle, radius, cap, o, -1, 5) == nbx.NBX_ERR_ARG
            assert err() == name + ": radius is NaN or negative"
    # 3. the capacity is negative or above 2^28 -- before the arrays
    for cap in (-1, -2 ** 62, 2 ** 28 + 1, 2 ** 62):
        for o in (full, [None] * 4):
            assert _call(nbx, name, handle, 0.25, cap, o, -1, 5) == nbx.NBX_ERR_ARG
            assert err() == name + ": capacity is negative or exceeds 268435456 (3 GiB of device lists in fp64)"
    # 4. capacity > 0 with both lists NULL; offsets or total NULL -- before the range and the state
    for cap in (1, 8, 2 ** 28):
        assert _call(nbx, name, handle, 0.25, cap, counting, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == name + ": capacity > 0 but index and r2 are both NULL"
    for cap, o in ((8, [None, index, r2, total]), (8, [offsets, index, r2, None]), (0, [None, None, None, total]), (0, [offsets, None, None, None])):
        assert _call(nbx, name, handle, float("inf"), cap, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == name + ": offsets or total is NULL"
    assert (offsets == -7).all() and total[0] == -7
    if name != "nbx_nlist":
        # 5. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for cap, o in ((8, full), (0, counting), (8, [offsets, index, None, total]), (8, [offsets, None, r2, total])):
                assert _call(nbx, name, handle, 0.25, cap, o, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        assert (offsets == -7).all() and total[0] == -7
        # 8. count == 0 inside the range: NBX_OK, offsets[0] = 0 and *total = 0 and nothing else, no HIP call
        for cap, o in ((8, full), (0, counting)):
            offsets[:], total[:] = -7, -7
            assert _call(nbx, name, handle, 0.25, cap, o, 0, 0) == nbx.NBX_OK
            assert offsets[0] == 0 and total[0] == 0 and (offsets[1:] == -7).all()
    else:
        # 7. the state: the zeroed context has not been uploaded
        for radius, cap, o in ((0.25, 8, full), (0.0, 0, counting), (float("inf"), 2 ** 28, [offsets, None, r2, total])):
            assert _call(nbx, name, handle, radius, cap, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_nlist: nbx_upload has not been called"
        assert (offsets == -7).all() and total[0] == -7
    assert (index == -7).all() and (r2 == -7.25).all() and zeroed.raw == bytes(1 << 16)


def test_the_bounds_and_the_order_of_the_checks_are_in_the_source():
    """More than 2^22 bodies in one call cannot be made here without a device; the check and its texts are read off the source,
    between the range check and the upload check.  So are the launches and synchronisations a call makes."""
    src = re.sub(r"//.*", "", open(SRC).read())
    shape = re.sub(r"//.*", "", open(os.path.join(CSRC, SHAPE)).read())
    assert "constexpr long long kNlMaxBodies = 1ll << 22;" in shape and "constexpr long long kNlMaxCapacity = 1ll << 28;" in shape
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_nlist: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kNlMaxBodies" in src and "range_bodies(o, first, count) > kNlMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_nlist("):]
    order = [batch.index(w) for w in ("is NULL", "check_args(", "check_range(", "kNlMaxBodies", "check_uploaded(", "count == 0", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_nlist("):]
    order = [ctx.index(w) for w in ("is NULL", "check_args(", "kNlMaxBodies", "->uploaded", "pending_commit", "use_device(")]
    assert order == sorted(order)
    args = src[src.index("int check_args("):src.index("template <typename T>\nT radius2")]
    order = [args.index(w) for w in ("bad_radius(", "a.capacity < 0 || a.capacity > kNlMaxCapacity", "a.capacity > 0 && !a.index && !a.r2",
                                     "!a.offsets || !a.total")]
    assert order == sorted(order) and "hip" not in args
    run = src[src.index("int run_nlist("):src.index("int nlist_ctx_t(")]
    # a counting call: the pair work, the finish, three launches of the scan, one read-back, one synchronisation; a filling call adds
    # the pair work again, the read-back of the lists asked for and a second synchronisation
    order = [run.index(w) for w in ("count_pass(seg)", "nlist_finish_kernel", "nlist_scan_sums_kernel", "nlist_scan_blocks_kernel",
                                    "nlist_scan_apply_kernel", "hipMemcpyAsync(a.offsets", "hipStreamSynchronize", "total > a.capacity",
                                    "sizeof(int) * (size_t)total", "sizeof(T) * (size_t)total", "fill_pass(seg, lists)", "if (a.index) HIP_TRY(hipMemcpyAsync(",
                                    "if (a.r2) HIP_TRY(hipMemcpyAsync(")]
    assert order == sorted(order)
    assert len(re.findall(r"HIP_TRY\(hipStreamSynchronize\(", run)) == 2 and len(re.findall(r"hipLaunchKernelGGL\(", run)) == 4
    assert run.count("capacity") == 1  # the one compare: the device lists are sized by the total, never by the capacity


def test_python_methods_and_nlist_pairs(nbx):
    p = inspect.signature(nbx.Context.nlist).parameters
    assert list(p) == ["self", "radius", "capacity"] and p["capacity"].default is None
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.nlist).parameters
        assert list(p) == ["self", "radius", "capacity", "first", "count"], cls
        assert p["capacity"].default is None and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "nlist")  # groups: deliberately not there
    assert not [f for f, _ in nbx.Opts._fields_ if "nlist" in f or "capacity" in f]  # no new nbx_opts field
    assert nbx.NLIST_MAX_CAPACITY == 2 ** 28 and nbx.NLIST_FIRST_GUESS == 16
    assert list(inspect.signature(nbx.nlist_pairs).parameters) == ["nl", "n"]
    # a context's result
    st = R.cloud(257, 64)
    nl = R.nlist(st, R.cases(64, 257)[1][2], 64)
    pairs, r2 = nbx.nlist_pairs(nl)
    want = sorted((i, int(j)) for i in range(257) for j in nl["index"][nl["offsets"][i]:nl["offsets"][i + 1]] if i < j)
    assert pairs.dtype == np.int64 and pairs.shape == (nl["total"] // 2, 2) and [tuple(p) for p in pairs.tolist()] == want and len(want) > 100
    e = R.body_of_entry(nl["offsets"])
    assert np.array_equal(r2, nl["r2"][e < nl["index"]])
    # batch results: per member, member-local
    both = R.concat([nl, nl])
    for arg in (257, [257, 257]):
        per = nbx.nlist_pairs(both, arg)
        assert len(per) == 2 and all(np.array_equal(q[0], pairs) and np.array_equal(q[1], r2) for q in per)
    for bad in (256, [257, 256]):
        with pytest.raises(nbx.NbxError):
            nbx.nlist_pairs(both, bad)
    with pytest.raises(nbx.NbxError):
        nbx.nlist_pairs({"offsets": nl["offsets"], "index": None, "r2": None, "total": nl["total"]})


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_nlist\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_nlist\.o: \$\(CSRC\)/nbx_nlist\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    other = re.search(r"^\$\(PKG\)/nbx_neighbours\.o: \$\(CSRC\)/nbx_neighbours\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == other.group(1).replace("neighbours", "nlist").replace("nbx_field_shape.hpp", "nbx_field_shape.hpp $(CSRC)/" + SHAPE)
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_nlist.hip", "include/nbx_nlist.h"):
        assert word in sh, word
    for doc, words in (("README.md", ("nbx_nlist", "nbx_nlist_shape.hpp")), ("DESIGN.md", ("nbx_nlist", "prefix sum", "second pass")),
                       ("INTEGRATION.md", ("nbx_nlist", "capacity")), (os.path.join("profiles", "README.md"), ("nlist_cost.json",))):
        txt = open(os.path.join(ROOT, doc)).read()
        for word in words:
            assert word in txt, (doc, word)


def test_the_kernels_live_in_their_own_translation_unit_reuse_the_shape_rule_and_wait_for_nobody():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_nlist.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_nlist.hip", KERNELS):
            assert "nlist_kernel" not in txt and "nl_body" not in txt and "nlist_scan" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    shape = open(os.path.join(CSRC, SHAPE)).read()
    both = re.sub(r"//.*", "", src + kern)
    assert not re.search(r"nbx_(?!nlist)\w+_kernels\.hpp", both)  # no other feature's kernels
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern and '#include "nbx_nlist_shape.hpp"' in kern
    assert "diag_splits" not in both and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)  # the field's rule, no new one
    assert "#include" not in re.sub(r"//.*", "", shape) and "__device__" not in shape and "hip" not in re.sub(r"//.*", "", shape)  # host-only constexpr
    assert "static_assert(nl_scan_blocks(kNlMaxBodies) <= kNlScanBlock" in shape
    # no atomics, and no kernel waits for another workgroup: no flag is polled, nothing is volatile, no fence, no cooperative launch
    for word in ("atomic", "volatile(", "volatile ", "__threadfence", "cooperative", "while (", "__builtin_amdgcn_s_sleep"):
        assert word not in both, word
    # the whole-record read and the finish kernel's binary search over the member table live in the shared device layer
    shared = re.sub(r"//.*", "", open(os.path.join(CSRC, "nbx_tilewalk.hpp")).read())
    assert "whole_record(tile, j)" in kern and "member_at(table, first, count, n_all, idx)" in kern
    assert shared.count('asm volatile("" ::"v"(r.w));') == 1 and shared.count("while (") == 1 and "while (lo < hi)" in shared
    for word in ("atomic", "volatile ", "__threadfence", "cooperative", "__builtin_amdgcn_s_sleep"):
        assert word not in shared.replace('asm volatile("" ::"v"(r.w));', ""), word
    # one pair function decides for both passes, and every store of the fill is behind the wave-wide branch and the segment's end
    assert both.count("r2 <= h2") == 1 and both.count("nl_in<") == 3
    assert "if (__any(in0 || in1)) {" in kern and "if (__any(some)) {" in kern and "if (pos < end) {" in kern
    assert kern.count("out.index[") == 1 and kern.count("out.r2[") == 1
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents("):
        assert fn in src, fn
    shared = open(os.path.join(CSRC, "nbx_analysis.hpp")).read()  # device_alloc and device_table are reached through the two helpers
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    assert "read_back(" not in src  # the scan and the two lists are the call's own flow, not the shared read-back skeleton
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("nl_seg", "nl_scan", "nl_index", "nl_r2", "nl_tab"):
        assert re.search(r"void\* %s = nullptr;" % field, obj) and "o->%s" % field in obj[obj.index("inline void batch_release"):], field


def test_the_scan_shape_is_two_levels_of_2048_and_serves_exactly_the_largest_call(tmp_path):
    exe = str(tmp_path / "nlist_shape_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "nlist_shape_driver.cpp"), "-o", exe])
    bodies = [1, 2, 2047, 2048, 2049, 4095, 4096, 4097, 6147, 531441, 2 ** 22 - 1, 2 ** 22]
    lines = subprocess.run([exe] + [str(b) for b in bodies], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1] == "block 2048 threads 256 items 8 max_bodies 4194304 max_capacity 268435456 first_guess 16"
    got = [tuple(int(v) for v in line.split()) for line in lines[:-1]]
    assert got == [(b, -(-b // R.SCAN_BLOCK), (b - 1) // R.SCAN_BLOCK, (b - 1) % R.SCAN_BLOCK) for b in bodies]
    blocks = {b: k for b, k, _, _ in got}
    assert (blocks[2048], blocks[2049], blocks[4096], blocks[4097], blocks[531441]) == (1, 2, 2, 3, 260)  # the seams, and the large lattice
    assert blocks[2 ** 22] == 2048 == R.SCAN_BLOCK  # one workgroup scans the block sums of the largest call
    # the restatement's scan against the plain prefix sum across the seams
    rng = np.random.default_rng(3)
    for b in (1, 2047, 2048, 2049, 4096, 4097, 6147):
        w = rng.integers(0, 50, b)
        assert np.array_equal(R.scan(w), np.concatenate([[0], np.cumsum(w)])), b
    big = np.full(4097, 2 ** 31, dtype=np.int64)  # the sums are 64-bit
    assert R.scan(big)[-1] == 4097 * 2 ** 31


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
    out = tmp_path_factory.mktemp("isa") / "nbx_nlist.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision, fill) of a pair-work kernel, (name, None, None) of the finish and the scan's three."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)nlist_kernelI([fd])Lb([01])EEE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64, m.group(3) == "1")
    m = re.search(r"^_ZN3nbx\d+nlist_(finish|scan_sums|scan_blocks|scan_apply)_kernelE", name)
    return (m.group(1), None, None) if m else None


def _segments(body, ins):
    """The straight-line pieces (label ... branch back or on) that hold `ins`: the innermost loop bodies, and for the fill pass
    the pieces of its unrolled loop between the wave-wide branches."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_every_kind_precision_and_pass_is_compiled_and_the_finish_and_the_scan(isa):
    keys = sorted((_key(k) or ("?", k, None) for k in isa), key=str)
    want = [(kind, p, f) for kind in ("context", "ensemble", "ragged") for p in (32, 64) for f in (False, True)]
    want += [(k, None, None) for k in ("finish", "scan_sums", "scan_blocks", "scan_apply")]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_no_atomics_and_one_tile_of_position_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        assert not re.search(r"(?:global|flat|ds|buffer)_atomic|ds_(?:add|min|max)_", body), name
        kind, precision, _ = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        want = {"finish": 0, "scan_sums": 256 * 8, "scan_blocks": 256 * 8, "scan_apply": 256 * 8}.get(kind, 256 * (16 if precision == 32 else 32))
        assert lds == want, (name, lds)


def test_the_fp32_count_loop_is_packed_and_one_compare_and_one_add_per_pair_and_the_fill_runs_it_between_its_branches(isa):
    """Per j record the lane's two bodies, i.e. two pairs: one whole 16-byte LDS read, 3 packed subtracts and 3 packed fused
    multiply-adds; no root, no reciprocal, no multiply.  The count pass without the mask adds to that 2 float compares and the two
    counts' select and add-with-carry (the compiler's form of two 0/1 adds: one select, one v_addc that takes the other compare's
    bit as its carry) and nothing else; the masked loop has more compares.  The fill pass's unrolled loop falls into pieces at its
    wave-wide branches: every piece that computes pairs has the same packed work and the same compares and holds no store."""
    for name, (body, desc, meta) in isa.items():
        kind, precision, fill = _key(name)
        if precision is None:
            continue
        c = lambda ins, text: len(re.findall(r"\b%s" % ins, text))
        if precision == 64:
            assert c("v_fma_f64", body) + c("v_fmac_f64", body) > 0 and c("v_add_f64", body) > 0 and c(r"v_mul_f64", body) == 0, name
            continue
        segs = _segments(body, "v_pk_fma_f32")
        assert len(segs) == (8 if fill else 2), (name, len(segs))  # masked and unmasked; the fill's unroll of 4 in pieces
        n_cmp = []
        for seg in segs:
            records = c(r"ds_(?:read|load)_b128", seg)
            assert records == (1 if fill else 4) and c(r"ds_(?:read|load)_b(?:32|64|96)\b", seg) == 0, (name, records)  # whole records only
            assert c("v_pk_fma_f32", seg) == 3 * records and c("v_pk_add_f32", seg) == 3 * records, (name, records)
            assert c(r"v_(?:add|sub|mul|fma|fmac)_f32", seg) == 0 and c("v_pk_mul_f32", seg) == 0, name  # nothing unpacked, no multiply
            assert c(r"(?:global|flat)_(?:store|load)", seg) == 0, name  # the stores sit behind the branch
            assert c(r"v_rsq_|v_sqrt_|v_rcp_|v_div_", seg) == 0, name  # no root, no reciprocal
            n_cmp.append(c("v_cmp_", seg) / records)
            if not fill:
                assert c("v_cndmask_b32", seg) == records and c("v_addc_co_u32", seg) == records, (name, c("v_cndmask_b32", seg))
                assert c(r"v_(?:add|sub|subrev|subb)_(?:co_)?[ui]32", seg) == 0 and c(r"v_(?:min|max)_", seg) == 0, name  # there is no minimum
        assert min(n_cmp) == 2 and max(n_cmp) > 2, (name, n_cmp)  # one float compare per pair; the mask's on top
        if fill:
            assert c(r"global_store_dword\b", body) >= 4, name  # (j, r2) for each of the lane's two bodies


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_two_and_three_bodies_give_the_closed_forms():
    def state(xs):
        z = np.zeros(len(xs))
        return {"pos_x": np.array(xs, dtype=np.float64), "pos_y": z, "pos_z": z}
    one = R.nlist(state([0.5]), 10.0, 64)
    assert one["offsets"].tolist() == [0, 0] and one["total"] == 0 and one["index"].size == 0
    three = R.nlist(state([0.0, 1.0, 3.0]), 1.5, 64)
    assert three["offsets"].tolist() == [0, 1, 2, 2] and three["index"].tolist() == [1, 0] and three["r2"].tolist() == [1.0 + EPS2] * 2
    three = R.nlist(state([0.0, 1.0, 3.0]), 2.0, 64)
    assert three["offsets"].tolist() == [0, 1, 3, 4] and three["index"].tolist() == [1, 0, 2, 1]
    every = R.nlist(state([0.0, 1.0, 3.0]), float("inf"), 64)
    assert every["offsets"].tolist() == [0, 2, 4, 6] and every["index"].tolist() == [1, 2, 0, 2, 0, 1]
    same = R.nlist(state([2.0, 7.0, 2.0]), 0.0, 32)  # two distinct bodies at one position, radius 0: h2 == eps2 == their r2
    assert same["offsets"].tolist() == [0, 1, 1, 2] and same["index"].tolist() == [2, 0] and same["r2"].tolist() == [EPS2, EPS2]
    for xs, radius, precision in (([0.0, 1.0, 3.0], 2.0, 64), ([0.0, 1.0, 3.0], float("inf"), 64), ([2.0, 7.0, 2.0], 0.0, 32), ([0.5], 1.0, 32)):
        assert not R.differs(R.restate(state(xs), radius, precision), R.nlist(state(xs), radius, precision), 64), (xs, radius)


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("precision", [32, 64])
def test_no_case_of_the_device_tests_is_ambiguous_and_the_restatement_is_the_plain_definition(precision, n):
    splits = R.field_shape(n, n)[2]
    assert splits == {2049: 2, 4097: 4}.get(n, 1)
    for name, st, radius in R.cases(precision, n):
        assert not R.ambiguous(st, radius, precision), (n, name, radius)
        want = R.nlist(st, radius, precision)
        got = R.restate(st, radius, precision)
        assert not R.differs(got, want, 64) and np.array_equal(got["r2"], want["r2"]), (n, name)
        if name == "inf":
            assert want["total"] == n * (n - 1)
        if name == "zero":
            assert want["total"] == (2 if n >= 2 else 0) and (want["r2"] == EPS2).all()
            assert want["index"].tolist() == ([n - 1, 0] if n >= 2 else [])
    if n >= 1025:
        per = [np.diff(R.nlist(st, radius, precision)["offsets"]).mean() for _, st, radius in R.cases(precision, n)[:3]]
        assert per[0] < 1.0 and 4.0 < per[1] < 8.0 and 28.0 < per[2] < 50.0, per  # sparse, about 6, about 40 (the box's faces cost some)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_batch_cases_are_unambiguous_and_their_restatement_is_the_members_lists_end_to_end(precision):
    for states, radius in (R.ensemble_states(precision), R.ragged_states(precision)):
        for st in states:
            assert not R.ambiguous(st, radius, precision)
        want = R.concat([R.nlist(st, radius, precision) for st in states])
        assert not R.differs(R.restate(states, radius, precision), want, 64)
        assert want["offsets"].shape == (sum(len(st["mass"]) for st in states) + 1,) and want["total"] > 1000


FAULT_CASES = {
    "self not masked": "r1", "padding record not masked": "inf", "< instead of <=": "zero", "split starts in the wrong order": "r2",
    "a scan block's carry dropped": "r1", "inclusive scan": "r1", "global j in a batch": "ensemble", "offsets restarted per member": "ragged",
    "the lane's second body writes at the first body's position": "r1",
}


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    """On the named case of the device tests' table (n = 4097 for a context's) the comparison the device tests apply rejects the
    faulty scheme; without a fault it accepts it (the tests above)."""
    assert set(FAULT_CASES) == set(R.FAULTS)
    table = {name: (st, radius) for name, st, radius in R.cases(precision, 4097)}
    table["ensemble"] = R.ensemble_states(precision)
    table["ragged"] = R.ragged_states(precision)
    wants = {}
    for fault in R.FAULTS:
        name = FAULT_CASES[fault]
        st, radius = table[name]
        if name not in wants:
            wants[name] = R.concat([R.nlist(s, radius, precision) for s in st]) if isinstance(st, list) else R.nlist(st, radius, precision)
        found = R.differs(R.restate(st, radius, precision, fault=fault), wants[name], precision)
        assert found, fault
