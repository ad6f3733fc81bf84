"""Clumps under a caller-supplied label (include/nbx_clumps.h), the parts that need no GPU: the header and its three exported
symbols, the argument checks that come before the first HIP call, the Python methods, clump_catalogue and unbind, the build
files, an audit of the cross-compiled gfx950 code of nbx_clumps.hip, and the numpy reference tests/clumps_ref.py, which must show
by itself what the device tests then ask of the library: closed forms for 1, 2 and 3 bodies, that its restatement of the split
and finish scheme is the plain definition within the gate on the states of the device tests, that every planted fault is caught
by the comparison of the device tests, and that the planted unbinding case is decided outside the gate's window of 0.

Which case catches which planted fault (both precisions):
    stripes(2049): the self term kept in phi, self left out of gm, negative labels matching each other, a split dropped (two
        splits), the lane's second body using the first one's label (256 % 7 != 0), the scale not undone, an unweighted mean
        velocity, v in place of v - V
    stripes(257): padding counted (255 padding records)
    huge(513): labels compared after conversion to float32 (2^31 - 1 - i % 5 are one float32)
    fof(2049): the one-body case missing (hundreds of bodies alone)
"""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import clumps_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_clumps.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_clumps_kernels.hpp"
ENTRY_POINTS = ("nbx_clumps", "nbx_ensemble_clumps", "nbx_ragged_clumps")
NOUN = {"nbx_clumps": "ctx", "nbx_ensemble_clumps": "ensemble", "nbx_ragged_clumps": "ragged ensemble"}
OTHER_TUPLES = ("SYMBOLS", "DIAG_SYMBOLS", "ENSEMBLE_SYMBOLS", "ENSEMBLE_DIAG_SYMBOLS", "RAGGED_SYMBOLS", "RAGGED_DIAG_SYMBOLS",
                "BATCH_ACCEL_SYMBOLS", "KICK_SYMBOLS", "TIMESCALE_SYMBOLS", "FIELD_SYMBOLS", "NEIGHBOUR_SYMBOLS", "PAIRCOUNT_SYMBOLS",
                "TRACER_SYMBOLS", "KNN_SYMBOLS", "FOF_SYMBOLS", "BINARIES_SYMBOLS", "TIDAL_SYMBOLS")
FORBIDDEN = ("neighbour_kernel", "nb_body", "field_kernel", "field_body", "timescale_kernel", "tracer_kernel", "tracer_body",
             "tracer_update_kernel", "knn_kernel", "knn_body", "knn_insert", "fof_pass_kernel", "fof_body", "fof_hook_kernel", "JLANE_EPI",
             "bound_kernel", "bound_body", "bound_finish_kernel", "tidal_kernel", "tidal_body")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


def _other_headers():
    return sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h != "nbx_clumps.h")


PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_clumps.h"\n'
           'int main(void) { '
           'nbx_clumps_out_t o = {0}; '
           'int (*a)(nbx_ctx*, const int32_t*, const nbx_clumps_out_t*) = nbx_clumps; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, const int32_t*, const nbx_clumps_out_t*) = nbx_ensemble_clumps; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, const int32_t*, const nbx_clumps_out_t*) = nbx_ragged_clumps; '
           'o.centre[2] = o.velocity[2] = o.phi = o.energy = o.gm = NULL; o.members = NULL; '
           'printf("ok %d\\n", (int)(sizeof(o) / sizeof(void*))); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')
STUBS = ('#include "nbx_clumps.h"\n'
         'int nbx_clumps(nbx_ctx* h, const int32_t* l, const nbx_clumps_out_t* o) { (void)h; (void)l; (void)o; return 0; }\n'
         'int nbx_ensemble_clumps(nbx_ensemble* h, int32_t f, int32_t n, const int32_t* l, const nbx_clumps_out_t* o) '
         '{ (void)h; (void)f; (void)n; (void)l; (void)o; return 0; }\n'
         'int nbx_ragged_clumps(nbx_ragged* h, int32_t f, int32_t n, const int32_t* l, const nbx_clumps_out_t* o) '
         '{ (void)h; (void)f; (void)n; (void)l; (void)o; return 0; }\n')


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "clumps_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok 10\n"  # ten pointers, nothing else


def test_declared_set_is_the_three_symbols_exported_and_apart_from_every_other_tuple(nbx):
    declared = _declared("nbx_clumps.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.CLUMPS_SYMBOLS) == ENTRY_POINTS and len(nbx.CLUMPS_SYMBOLS) == 3
    assert nbx.CLUMPS_KEYS == R.KEYS and ctypes.sizeof(nbx.ClumpsOut) == 10 * ctypes.sizeof(ctypes.c_void_p)
    for h in _other_headers():
        assert not set(declared) & set(_declared(h)), h
        assert "_clumps" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in OTHER_TUPLES:
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (3 if s == "nbx_clumps" else 5)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_clumps.h")).read())  # the comment as running text
    for word in ("Why:", "Definition", "Arithmetic", "Error of one term", "Arrays:", "Contexts:", "Semantics", "Status, in this order",
                 "Unspecified results", "Deliberately not here", "fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))", "AS INTEGERS",
                 "never pass through a floating-point value", "above 2^24", 'means "in no clump"', "j == i is never formed in phi",
                 "Records at or beyond n never count", "negative labels do not match each other", "phi = 0 and energy = 0",
                 "centre and velocity are 0", "UNROUNDED quotients", "SAME BITS", "bijective renaming", "No atomics, no sort, no second pass",
                 "4.5u in fp32", "53.5u in fp64", "a NULL array is never written", "member-major", "end to end", "member-local",
                 "sliced context", "is refused", "nbx_commit", "synchronises once", "One label upload", "steps_done", "*_timed / *_ms_total",
                 "kinetic-energy partials", "the state of graph", "label or out is NULL", "checked in 64 bits", "2^22",
                 "names the first such member", "the velocities of the others are not resident", "before the first HIP call",
                 "NBX_ERR_ALLOC", "not finite", "groups and sliced contexts", "nbx.unbind", "device pointers", "hipGraph", "nbody.x",
                 'what nbx_fof.h lists under "Deliberately not here" as bound or unbound tests'):
        assert word in doc, word
    assert "bound or unbound" in re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_fof.h")).read())  # the gap, named there


def _call(nbx, name, handle, label, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    lab = None if label is None else label.ctypes.data_as(ctypes.c_void_p)
    o = None if out is None else ctypes.byref(out)
    return f(handle, lab, o) if name == "nbx_clumps" else f(handle, first, count, lab, o)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    arrays = {k: np.full(8, -7, dtype=np.int32 if k == "members" else np.float64) for k in R.KEYS}
    a = [arrays[k].ctypes.data for k in R.KEYS]
    out = nbx.ClumpsOut(a[0], a[1], (ctypes.c_void_p * 3)(*a[2:5]), (ctypes.c_void_p * 3)(*a[5:8]), a[8], a[9])
    none = nbx.ClumpsOut()
    label = np.zeros(8, dtype=np.int32)
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for lab, o in ((label, out), (None, None), (label, none)):
        assert _call(nbx, name, None, lab, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. label or out is NULL -- before the range and the state
    for lab, o in ((None, out), (label, None), (None, None)):
        assert _call(nbx, name, handle, lab, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == name + ": label or out is NULL"
    if name != "nbx_clumps":
        # 3. the range leaves [0, members): the zeroed object has none -- also where nothing is asked for
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for o in (out, none):
                assert _call(nbx, name, handle, label, o, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 8. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with outputs and without
        assert _call(nbx, name, handle, label, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, label, none, 0, 0) == nbx.NBX_OK
    else:
        # 5. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for o in (out, none):
            assert _call(nbx, name, handle, label, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_clumps: nbx_upload has not been called"
    assert all((v == -7).all() for v in arrays.values()) and (label == 0).all() and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_and_the_refusal_of_a_sliced_context_are_in_the_source_in_the_stated_order():
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kClumpMaxBodies = kFieldMaxPoints;" in hdr
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_clumps: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kClumpMaxBodies" in src and "range_bodies(o, first, count) > kClumpMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_clumps("):]
    order = [batch.index(w) for w in ("is NULL", "label or out is NULL", "check_range(", "kClumpMaxBodies", "check_uploaded(", "no_output(*out)",
                                      "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_clumps("):]
    order = [ctx.index(w) for w in ("is NULL", "label or out is NULL", "kClumpMaxBodies", "->uploaded", "pending_commit",
                                    "c->i_begin != 0 || c->i_count != c->n", "no_output(*out)", "use_device(")]
    assert order == sorted(order)
    text = "the context owns a slice of the bodies (the velocities of the others are not resident)"
    assert 'fail(NBX_ERR_STATE, "nbx_clumps: %s")' % text in ctx and '"nbx_clumps: a local step awaits nbx_commit"' in ctx
    # the read-back is the shared skeleton's: one use of the helper, and in the helper's body one copy, one synchronisation and
    # the one of the failure path; the call's own source keeps the label upload and the ragged table's guard, which runs only when
    # an exception leaves the call
    assert len(re.findall(r"\bread_back\(", src)) == 1 and "hipStreamSynchronize(o->stream)" not in src
    helper = shared[shared.index("int read_back("):]
    helper = helper[:helper.index("\n}\n")]
    assert len(re.findall(r"hipStreamSynchronize\(o->stream\)", helper)) == 2 and len(re.findall(r"hipStreamSynchronize\(", helper)) == 2
    assert len(re.findall(r"hipStreamSynchronize\(", src)) == 1 and "~Drain() { if (armed) (void)hipStreamSynchronize(stream); }" in src
    assert len(re.findall(r"hipMemcpyAsync\(", src)) == 1 and "hipMemcpyHostToDevice" in src  # an upload
    assert len(re.findall(r"hipMemcpyAsync\(", helper)) == 1 and "hipMemcpyDeviceToHost" in helper  # a read-back
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == 4  # three kinds, one finish


def test_python_methods_and_the_helpers_are_as_specified(nbx):
    assert list(inspect.signature(nbx.Context.clumps).parameters) == ["self", "label"]
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.clumps).parameters
        assert list(p) == ["self", "label", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "clumps")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "clump" in f]  # no new nbx_opts field
    p = inspect.signature(nbx.clump_catalogue).parameters
    assert list(p) == ["label", "result", "mass", "min_members"] and p["min_members"].default == 2
    p = inspect.signature(nbx.unbind).parameters
    assert list(p) == ["obj", "label", "max_iter"] and p["max_iter"].default == 32
    with pytest.raises(nbx.NbxError):
        nbx.unbind(object(), np.zeros(4, dtype=np.int32))
    with pytest.raises(nbx.NbxError):
        nbx.clump_catalogue(np.zeros(4, dtype=np.int32), {k: np.zeros(3) for k in R.KEYS}, np.ones(4))


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_clumps\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_clumps\.o: \$\(CSRC\)/nbx_clumps\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    other = re.search(r"^\$\(PKG\)/nbx_binaries\.o: \$\(CSRC\)/nbx_binaries\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == other.group(1).replace("binaries", "clumps")  # the same dependency list
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_clumps.hip", "include/nbx_clumps.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_reuse_the_shape_rule_and_keep_to_the_naming_rules():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_clumps.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_clumps.hip", KERNELS):
            assert "clump_kernel" not in txt and "clump_body" not in txt and "clump_finish_kernel" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    both = re.sub(r"//.*", "", src + kern)
    for word in FORBIDDEN:
        assert word not in src + kern, word  # comments included: the other features' tests read every file
    assert not re.search(r"nbx_(?!clumps)\w+_kernels\.hpp", src + kern)  # no other feature's kernels, not even by name
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern  # the field's rule, no new one
    assert "diag_splits" not in src + kern and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)
    assert "fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())))" in kern  # r2 restated, not shared
    assert "atomic" not in both
    assert "__shared__ T4 ptile[kTile];" in kern and "__shared__ T4 vtile[kTile];" in kern  # two arrays per tile
    assert re.sub(r"//.*", "", kern).count("velm[j]") == 2 and re.sub(r"//.*", "", kern).count("lab[j]") == 2  # only below n
    assert "(float)l" not in both and "(T)l" not in both and "__int2float" not in both  # a label is never converted
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("clump_lab", "clump_part", "clump_out", "clump_tab"):
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
    out = tmp_path_factory.mktemp("isa") / "nbx_clumps.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair-work kernel, ("finish", precision) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)clump_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+clump_finish_kernelI([fd])EE", name)
    return ("finish", 32 if m.group(1) == "f" else 64) if m else None


def _pair_loops(body, ins):
    """The innermost loop bodies (label ... backward branch) that hold `ins`."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_every_kind_and_precision_is_compiled_and_the_finish(isa):
    keys = sorted((_key(k) or ("?", k) for k in isa), key=str)
    assert keys == sorted([(kind, p) for kind in ("context", "ensemble", "ragged", "finish") for p in (32, 64)], key=str), keys


def test_no_scratch_no_spills_and_one_tile_of_position_and_velocity_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        kind, precision = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (0 if kind == "finish" else 256 * (32 if precision == 32 else 64)), (name, lds)  # exactly its tiles'


def test_the_pair_loops_have_the_specified_operations_per_record_packed_in_fp32_and_no_atomics(isa):
    """Per j record, relative to the 16-byte LDS reads (two per fp32 record: the position and the velocity, both read whole): 4
    packed adds (three subtracts, the mass), 10 packed fma (3 r2, phi, 3 momentum, 3 moment), 2 v_rsq_f32, no packed multiply
    and nothing unpacked; in the loop without the self mask 2 integer compares and, for the lane's two bodies, 2 selects of g and
    the count's select and add-with-carry (the compiler's form of two counts: one 0/1 select, one v_addc that takes the other
    compare's bit as its carry)."""
    for name, (body, desc, meta) in isa.items():
        kind, precision = _key(name)
        c = lambda ins, text=body: len(re.findall(r"\b%s" % ins, text))
        assert c(r"(?:global|flat|ds|buffer)_atomic") + c(r"ds_(?:add|min|max)_") == 0, name
        assert c("v_sqrt") == 0, name
        if kind == "finish":
            assert c("v_rsq_") == 0, name
            continue
        if precision == 64:
            loops = _pair_loops(body, "v_rsq_f64")
            assert len(loops) == 2, (name, len(loops))
            for loop in loops:
                pairs = c("v_rsq_f64", loop)  # one seed per pair; a record serves the lane's two bodies
                assert pairs >= 2 and c(r"ds_(?:read|load)_b128", loop) == 2 * pairs, name  # a 32-byte record is two reads; two records per two pairs
                assert c("v_fma_f64", loop) + c("v_fmac_f64", loop) == 11 * pairs and c("v_add_f64", loop) == 4 * pairs, name  # 3 + 7 + the Newton step's; 3 + 1
                assert c("v_mul_f64", loop) == 2 * pairs, name  # the Newton step's
            continue
        loops = _pair_loops(body, "v_pk_fma_f32")
        assert len(loops) == 2, (name, len(loops))  # the loop with the self mask and the one without
        extra = []
        for loop in loops:
            reads = c(r"ds_(?:read|load)_b128", loop)
            assert reads >= 2 and reads % 2 == 0 and c(r"ds_(?:read|load)_b(?:32|64|96)\b", loop) == 0, (name, reads)  # whole records only
            records = reads // 2
            got = (c("v_pk_add_f32", loop), c("v_pk_fma_f32", loop), c("v_pk_mul_f32", loop), c("v_rsq_f32", loop))
            assert got == (4 * records, 10 * records, 0, 2 * records), (name, records, got)
            assert c(r"v_(?:add|sub|mul|fma|fmac)_f32", loop) == 0, name  # nothing unpacked
            assert records == 4, (name, records)  # the unroll the counts below are stated for
            extra.append((c("v_cmp_", loop), c("v_cmp_eq_u32", loop), c("v_cndmask_b32", loop), c("v_addc_co_u32", loop),
                          c(r"v_(?:add|sub|subrev|subb)_(?:co_)?[ui]32", loop)))
        # Pinned as built, per four records.  Without the self mask, per record: 2 label compares, 2 selects of g,
        # and for the two counts 1 select of 0/1 and 1 add-with-carry -- no other integer arithmetic.  With it, per four records:
        # 15 compares (8 of them the labels'), 20 selects, the 4 add-with-carry and 2 plain integer adds.
        assert sorted(extra) == [(8, 8, 12, 4, 0), (15, 8, 20, 4, 2)], (name, extra)


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _state(rows, T=np.float64):
    """rows of (x, y, z, vx, vy, vz, G m)."""
    st = {f: np.array(col, dtype=np.float64) for f, col in zip(R.FIELDS, zip(*rows))}
    st["mass"] = st["mass"] / R.G
    return {k: v.astype(T) for k, v in st.items()}


def _values(f, st, label, precision):
    if f is R.truth:
        tr = R.truth(st, label, precision)
        return dict({k: tr[k][0].astype(np.float64) for k in R.FLOAT_KEYS}, members=tr["members"])
    return {k: np.asarray(v, dtype=np.float64) for k, v in f(st, label, precision).items()}


@pytest.mark.parametrize("precision", [32, 64])
def test_one_two_and_three_bodies_give_the_closed_forms(precision):
    T = R.DTYPE[precision]
    tol = 8 * R.U[32]  # G m is rounded once when it is stored: the closed forms hold to that
    for f in (R.truth, R.restate):
        st = _state([(0.5, 0.25, -1.0, 1.0, 2.0, 3.0, 1.0)], T)
        one = _values(f, st, [7], precision)
        assert one["members"].tolist() == [1] and abs(one["gm"][0] - 1.0) <= tol and one["phi"][0] == 0 and one["energy"][0] == 0
        assert [one[k][0] for k in R.CENTRE + R.VELOCITY] == [0.5, 0.25, -1.0, 1.0, 2.0, 3.0]  # the body itself, exactly
        none = _values(f, st, [-3], precision)
        assert all(none[k][0] == 0 for k in R.KEYS)
        # two bodies 2 apart along x, G m = 1 and 3: centre at +0.5, phi_0 = -3 / sqrt(4 + eps2), phi_1 = -1 / sqrt(4 + eps2)
        st = _state([(-1.0, 0.5, 0.25, 0.0, 4.0, 0.0, 1.0), (1.0, 0.5, 0.25, 0.0, 0.0, 0.0, 3.0)], T)
        two = _values(f, st, [2 ** 31 - 1, 2 ** 31 - 1], precision)
        d = math.sqrt(4.0 + EPS2)
        assert two["members"].tolist() == [2, 2] and np.allclose(two["gm"], 4.0, rtol=tol, atol=0)
        assert np.allclose(two["centre_x"], 0.5, atol=tol) and np.allclose(two["velocity_y"], 1.0, atol=tol)
        assert np.allclose(two["phi"], [-3.0 / d, -1.0 / d], rtol=4 * tol) and np.allclose(two["energy"], [4.5 - 3.0 / d, 0.5 - 1.0 / d], atol=8 * tol)
        apart = _values(f, st, [5, 6], precision)  # two names: two clumps of one
        assert apart["members"].tolist() == [1, 1] and apart["phi"].tolist() == [0, 0] and apart["centre_x"].tolist() == [-1.0, 1.0]
        # three bodies, the third in no clump: it changes nothing for the two and gets zeros
        st3 = {k: np.concatenate([v, np.array([9.0 if k != "mass" else 1.0 / R.G], dtype=T)]) for k, v in st.items()}
        three = _values(f, st3, [4, 4, -1], precision)
        assert all(np.array_equal(three[k][:2], two[k]) for k in R.KEYS) and all(three[k][2] == 0 for k in R.KEYS)
        # massless members: gm == 0 with several members gives centre and velocity 0 and the kinetic term of the body's own velocity
        ghosts = _values(f, _state([(1.0, 2.0, 3.0, 1.0, 2.0, 2.0, 0.0), (5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)], T), [0, 0], precision)
        assert ghosts["members"].tolist() == [2, 2] and all(ghosts[k].tolist() == [0, 0] for k in R.CENTRE + R.VELOCITY + ("gm", "phi"))
        assert ghosts["energy"].tolist() == [4.5, 0.0]


def _device_cases(precision):
    """Every (name, case) the device tests compare with the reference: the contexts' (the ensemble's and the ragged members' states
    are among them) and the lattice with its sampled rows."""
    cases = [("%s(%d)" % (fam, n), R.case(precision, n, fam)) for n, fam in R.context_cases()]
    assert {(R.ENSEMBLE[1], f) for f in ("stripes", "fof", "blocks")} <= set(R.context_cases())
    assert {(n, "stripes") for n in R.NB.RAGGED_SIZES} <= set(R.context_cases())
    n = R.LATTICE_K ** 3
    return cases + [("lattice blocks(%d)" % n, R.case(precision, n, "blocks", state=R.lattice(precision), rows=R.lattice_rows(), name="lattice"))]


@pytest.mark.parametrize("precision", [32, 64])
def test_the_restatement_is_the_plain_definition_within_the_gate_on_the_states_of_the_device_tests(precision):
    shown = 0
    cases = _device_cases(precision)
    for name, c in cases:
        rows = c["truth"]["rows"] if name.startswith("lattice") else None
        got = R.restate(c["state"], c["label"], precision, rows=rows)
        problems, ks = R.compare(got, c["truth"], c["gates"], c["state"], c["label"], precision)
        print("fp%d %s: K_ref %s" % (precision, name, {k: round(v, 1) for k, v in c["kref"].items()}))
        assert not problems, (precision, name, problems)
        assert all(c["gates"][k] >= R.F.M * R.F.K_TERM for k in R.FLOAT_KEYS)
        assert c["gates"]["phi"] >= R.F.M * R.FLOOR["phi"][precision]
        if len(c["label"]) <= 2049:
            renamed = R.restate(c["state"], R.renamed(c["label"]), precision)
            assert all(np.array_equal(renamed[k], got[k]) for k in R.KEYS), (precision, name)  # a renaming changes nothing
        shown += 1
    assert shown == len(cases) == len(R.context_cases()) + 1  # none left out
    assert (R.FR.field_shape(257, 257)[2], R.FR.field_shape(513, 513)[0], R.FR.field_shape(2049, 2049)[2:]) == (1, 2, (2, 5))
    fof = R.case(precision, 2049, "fof")["truth"]["members"]
    assert (fof == 1).sum() > 100 and fof.max() >= 3  # singletons and groups


FAULT_CASES = (
    (2049, "stripes", ("the self term kept in phi", "self left out of gm", "negative labels matching each other", "a split dropped",
                       "the lane's second body using the first one's label", "the scale not undone", "an unweighted mean velocity",
                       "v in place of v - V")),
    (257, "stripes", ("padding counted",)),
    (513, "huge", ("labels compared after conversion to float32",)),
    (2049, "fof", ("the one-body case missing",)),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    planted = set()
    for n, fam, faults in FAULT_CASES:
        c = R.case(precision, n, fam)
        assert not R.compare(R.restate(c["state"], c["label"], precision), c["truth"], c["gates"], c["state"], c["label"], precision)[0]
        for fault in faults:
            got = R.restate(c["state"], c["label"], precision, fault=fault)
            problems, _ = R.compare(got, c["truth"], c["gates"], c["state"], c["label"], precision)
            print("fp%d %s(%d) %-52s: %s" % (precision, fam, n, fault, "; ".join(problems)))
            assert problems, (precision, n, fam, fault)
            planted.add(fault)
    assert planted == set(R.FAULTS) and len(R.FAULTS) == 11


@pytest.mark.parametrize("precision", [32, 64])
def test_the_planted_unbinding_case_is_decided_outside_the_gates_window_of_zero(precision):
    st = R.unbind_state(precision)
    n = R.UNBIND_N
    first = R.truth(st, np.zeros(n, dtype=np.int32), precision)["energy"][0]
    assert first[n - 2] > 0 and first[n - 1] < 0  # the interloper leaves at once; its companion is bound while it counts
    label, iterations, margin = R.unbind(st, np.zeros(n, dtype=np.int32), precision)
    print("fp%d: %d iterations, %d bodies left, margin %.3g gates" % (precision, iterations, (label >= 0).sum(), margin))
    assert iterations >= 3 and label[n - 2] == label[n - 1] == -1 and (label[:64] == 0).sum() >= 32
    assert margin > 1.0  # no reference energy lies within the gate's window of 0 in any iteration


class _Fake:
    """A Context-like object whose clumps() is the reference's truth."""

    def __init__(self, st, precision):
        self.st, self.precision, self.calls = st, precision, 0

    def clumps(self, label):
        self.calls += 1
        tr = R.truth(self.st, label, self.precision)
        return dict({k: tr[k][0].astype(np.float64) for k in R.FLOAT_KEYS}, members=tr["members"].astype(np.int32))


def test_clump_catalogue_and_unbind_agree_with_plain_loops(nbx, monkeypatch):
    c = R.case(64, 513, "fof")
    st, label = c["state"], c["label"]
    res = _Fake(st, 64).clumps(label)
    got = nbx.clump_catalogue(label, res, st["mass"])
    want = R.catalogue(label, res, st["mass"])
    assert len(want) >= 10 and got["label"].tolist() == [r[0] for r in want] and got["members"].tolist() == [r[1] for r in want]
    assert np.allclose(got["gm"], [r[2] for r in want], rtol=1e-15) and np.allclose(got["centre"], [r[3] for r in want], rtol=1e-15)
    assert np.allclose(got["velocity"], [r[4] for r in want], rtol=1e-15) and got["bound"].tolist() == [r[8] for r in want]
    for k, key in ((5, "kinetic"), (6, "potential"), (7, "virial")):
        assert np.allclose(got[key], [r[k] for r in want], rtol=1e-12), key
    assert (np.diff(got["members"]) <= 0).all() and (got["members"] >= 2).all() and (got["kinetic"] >= 0).all() and (got["potential"] < 0).all()
    alone = nbx.clump_catalogue(label, res, st["mass"], min_members=1)
    assert len(alone["label"]) == len(set(label.tolist())) and alone["virial"][alone["members"] == 1].tolist() == [np.inf] * int((alone["members"] == 1).sum())
    # unbind: a fake object that answers with the truth goes through the reference's iterations
    monkeypatch.setattr(nbx, "Context", _Fake)
    st = R.unbind_state(64)
    start = np.zeros(R.UNBIND_N, dtype=np.int32)
    want, iterations, _ = R.unbind(st, start, 64)
    fake = _Fake(st, 64)
    label, result, its = nbx.unbind(fake, start)
    assert np.array_equal(label, want) and its == iterations == fake.calls and (start == 0).all()  # the caller's labels are not written
    assert (result["energy"][label >= 0] < 0).all()
    label, _, its = nbx.unbind(_Fake(st, 64), start, max_iter=1)
    assert its == 1 and (label == -1).sum() >= 1 and label[R.UNBIND_N - 1] == 0  # the companion is still in after one call
