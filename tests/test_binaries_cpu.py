"""Most bound partner and bound count of every body (include/nbx_binaries.h), the parts that need no GPU: the header and its
three exported symbols, the argument checks that come before the first HIP call, the Python methods and binary_catalogue, the
build files, an audit of the cross-compiled gfx950 code of nbx_binaries.hip, and the numpy reference tests/binaries_ref.py,
which must show by itself what the device tests then ask of the library: that its restatement of the split and finish scheme is
the plain definition, that EVERY (state, precision) the device tests compare with it has no ambiguous partner, and that every
planted fault is caught.

Which state catches which planted fault (both precisions; "caught" = binaries_ref.differs, the comparison of the device tests):
    cloud(257): self not masked, padding record not masked, padding velocity read (255 padding records at the origin, inside the
        cloud), m_j alone instead of m_i + m_j
    cloud(2049): a split row dropped (two splits), indices offset by the member's place
    clustered(513): <= instead of < in the count (the two massless bodies that move as one: their pair energy is 0 exactly)
    lattice(13), both orders: ties to the highest j, finish takes a later split on ties (two splits meeting at j = 1280, equal
        candidates from both)
"""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import binaries_ref as R
import neighbours_ref as NB
from conftest import ROOT, PKG
from energy_ref import EPS2
from field_ref import field_shape

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_binaries.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_binaries_kernels.hpp"
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h", "nbx_field.h", "nbx_neighbours.h", "nbx_paircount.h", "nbx_tracers.h", "nbx_knn.h",
                 "nbx_fof.h")
ENTRY_POINTS = ("nbx_binaries", "nbx_ensemble_binaries", "nbx_ragged_binaries")
NOUN = {"nbx_binaries": "ctx", "nbx_ensemble_binaries": "ensemble", "nbx_ragged_binaries": "ragged ensemble"}
OTHER_TUPLES = ("SYMBOLS", "DIAG_SYMBOLS", "ENSEMBLE_SYMBOLS", "ENSEMBLE_DIAG_SYMBOLS", "RAGGED_SYMBOLS", "RAGGED_DIAG_SYMBOLS",
                "BATCH_ACCEL_SYMBOLS", "KICK_SYMBOLS", "TIMESCALE_SYMBOLS", "FIELD_SYMBOLS", "NEIGHBOUR_SYMBOLS", "PAIRCOUNT_SYMBOLS",
                "TRACER_SYMBOLS", "KNN_SYMBOLS", "FOF_SYMBOLS")
FORBIDDEN = ("neighbour_kernel", "nb_body", "field_kernel", "field_body", "timescale_kernel", "tracer_kernel", "tracer_body",
             "tracer_update_kernel", "knn_kernel", "knn_body", "knn_insert", "fof_pass_kernel", "fof_body", "fof_hook_kernel", "JLANE_EPI")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


OUT3 = "int32_t*, void*, int32_t*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_binaries.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, %s) = nbx_binaries; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, %s) = nbx_ensemble_binaries; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, %s) = nbx_ragged_binaries; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n' % (OUT3, OUT3, OUT3))
PARAMS = "int32_t* p, void* e, int32_t* b"
UNUSED = "(void)p; (void)e; (void)b;"
STUBS = ('#include "nbx_binaries.h"\n'
         'int nbx_binaries(nbx_ctx* h, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_binaries(nbx_ensemble* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_binaries(nbx_ragged* h, int32_t f, int32_t n, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "binaries_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_three_symbols_exported_and_apart_from_every_other_tuple(nbx):
    declared = _declared("nbx_binaries.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.BINARIES_SYMBOLS) == ENTRY_POINTS and len(nbx.BINARIES_SYMBOLS) == 3
    assert nbx.BINARIES_KEYS == ("partner", "energy", "bound") == R.KEYS
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "_binaries" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in OTHER_TUPLES:
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (4 if s == "nbx_binaries" else 6)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_binaries.h")).read())  # the comment as running text
    for word in ("Why:", "Definition", "Per-pair arithmetic", "Consequences", "Arrays:", "Contexts:", "Semantics", "Status, in this order",
                 "Unspecified results", "Deliberately not here", "fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))", "fma(ux,ux, fma(uy,uy, uz*uz))",
                 "s = add_rn(gm_i, gm_j)", "e = fma(-s, inv, w/2)", "the LOWEST j", "partner = -1, energy = +infinity, bound = 0", "by a mask",
                 "never read", "w/2 is exact", "power-of-two scale", "e(i, j) and e(j, i) are the same bits",
                 "partner[i] == j && partner[j] == i && energy[i] < 0", "if partner[i] == j then energy[j] <= energy[i]",
                 "(bound[i] > 0) == (energy[i] < 0)", "the sum of bound over a system is even", "6.5u (A + B)", "55.5u (A + B)",
                 "gives the same bits", "a NULL array is never written", "do not pay for the count", "member-major", "end to end",
                 "member-local", "sliced context", "is refused", "nbx_commit", "synchronises once", "no atomics", "steps_done",
                 "*_timed / *_ms_total", "kinetic-energy partials", "the state of graph", "checked in 64 bits", "2^22",
                 "names the first such member", "the velocities of the others are not resident", "before the first HIP call", "NBX_ERR_ALLOC",
                 "not finite", "groups and sliced contexts", "triples and hierarchies", "orbital elements on the device", '"hard" and "soft"',
                 "device pointers", "hipGraph", "nbody.x"):
        assert word in doc, word
    for h in ("nbx_neighbours.h", "nbx_fof.h"):  # the gap this header fills, named by the ones it follows
        assert "bound or unbound" in re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", h)).read()), h
    assert "a value per body" in re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_timescale.h")).read())


def _call(nbx, name, handle, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    args = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in out]
    return f(handle, *args) if name == "nbx_binaries" else f(handle, first, count, *args)


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
    for o in (out, none3, [None, out[1], None]):
        assert _call(nbx, name, None, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    if name != "nbx_binaries":
        # 2. the range leaves [0, members): the zeroed object has none -- also where nothing is asked for
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for o in (out, none3):
                assert _call(nbx, name, handle, o, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 7. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with outputs and without
        assert _call(nbx, name, handle, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, none3, 0, 0) == nbx.NBX_OK
    else:
        # 4. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for o in (out, none3, [None, out[1], None]):
            assert _call(nbx, name, handle, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_binaries: nbx_upload has not been called"
    assert (out[0] == -7).all() and (out[1] == -7.25).all() and (out[2] == -7).all() and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_and_the_refusal_of_a_sliced_context_are_in_the_source_in_the_stated_order():
    """More than 2^22 bodies in one call, a pending commit and a sliced context cannot be made here without a device; the checks
    and their texts are read off the source, in the header's order and before the first HIP call."""
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kBoundMaxBodies = kFieldMaxPoints;" in hdr
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_binaries: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kBoundMaxBodies" in src and "range_bodies(o, first, count) > kBoundMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_binaries("):]
    order = [batch.index(w) for w in ("is NULL", "check_range(", "kBoundMaxBodies", "check_uploaded(", "no_output(a)", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_binaries("):]
    order = [ctx.index(w) for w in ("is NULL", "kBoundMaxBodies", "->uploaded", "pending_commit", "c->i_begin != 0 || c->i_count != c->n",
                                    "no_output(a)", "use_device(")]
    assert order == sorted(order)
    # nbx_timescale's text, for its reason
    text = "the context owns a slice of the bodies (the velocities of the others are not resident)"
    assert 'fail(NBX_ERR_STATE, "nbx_binaries: %s")' % text in ctx
    assert '"nbx_timescale: %s"' % text in open(os.path.join(CSRC, "nbx_timescale.hip")).read()
    assert '"nbx_binaries: a local step awaits nbx_commit"' in ctx
    # the read-back is the shared skeleton's: no synchronisation of the call's own, one use of the helper, and in the helper's body
    # one synchronisation and the one of the failure path
    assert "hipStreamSynchronize" not in src and len(re.findall(r"\bread_back\(", src)) == 1
    helper = shared[shared.index("int read_back("):]
    helper = helper[:helper.index("\n}\n")]
    assert len(re.findall(r"hipStreamSynchronize\(o->stream\)", helper)) == 2 and len(re.findall(r"hipStreamSynchronize\(", helper)) == 2


def test_python_methods_keys_and_the_helper_are_as_specified(nbx):
    p = inspect.signature(nbx.Context.binaries).parameters
    assert list(p) == ["self", "bound"] and p["bound"].default is True
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.binaries).parameters
        assert list(p) == ["self", "bound", "first", "count"], cls
        assert p["bound"].default is True and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "binaries")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "binar" in f or "bound" in f]  # no new nbx_opts field
    p = inspect.signature(nbx.binary_catalogue).parameters
    assert list(p) == ["partner", "energy", "mass", "x", "y", "z", "vx", "vy", "vz"]
    assert "IGNORE THE SOFTENING" in nbx.binary_catalogue.__doc__
    with pytest.raises(nbx.NbxError):
        nbx.binary_catalogue(np.zeros(4, dtype=np.int32), np.ones(4), np.ones(3), *[np.ones(4)] * 6)


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_binaries\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_binaries\.o: \$\(CSRC\)/nbx_binaries\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    knn = re.search(r"^\$\(PKG\)/nbx_knn\.o: \$\(CSRC\)/nbx_knn\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == knn.group(1).replace("knn", "binaries")  # the same dependency list
    for dep in (KERNELS, "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_diag_shape.hpp", "nbx_pair.hpp", "include/nbx_binaries.h",
                "include/nbx_ensemble.h", "include/nbx_ragged.h", "include/nbx.h", "include/nbx_diag.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_binaries.hip", "include/nbx_binaries.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_reuse_the_shape_rule_and_keep_to_the_naming_rules():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_binaries.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_binaries.hip", KERNELS):
            assert "bound_kernel" not in txt and "bound_body" not in txt and "bound_finish_kernel" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    both = re.sub(r"//.*", "", src + kern)
    for word in FORBIDDEN:
        assert word not in src + kern, word  # comments included: the other features' tests read every file
    assert not re.search(r"nbx_(?!binaries)\w+_kernels\.hpp", src + kern)  # no other feature's kernels, not even by name
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern  # the field's rule, no new one
    assert "diag_splits" not in src + kern and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)
    assert "fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<T>())))" in kern  # r2 restated, not shared
    assert "fmaT(ux, ux, fmaT(uy, uy, mul_rn(uz, uz)))" in kern and "add_rn(gmi, gmj)" in kern and "fmaT(-s, inv, w)" in kern
    assert "atomic" not in both
    assert "__shared__ T4 ptile[kTile];" in kern and "__shared__ T4 vtile[kTile];" in kern  # two arrays per tile
    assert "if (j < n) next_v = velm[j];" in kern and re.sub(r"//.*", "", kern).count("velm[") == 3  # a velocity is loaded only below n
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("bin_part", "bin_out", "bin_tab"):
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
    out = tmp_path_factory.mktemp("isa") / "nbx_binaries.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision, with count) of a pair-work kernel, ("finish", precision, None) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)bound_kernelI([fd])Lb([01])EEE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64, m.group(3) == "1")
    m = re.search(r"^_ZN3nbx\d+bound_finish_kernelI([fd])EE", name)
    if m:
        return ("finish", 32 if m.group(1) == "f" else 64, None)
    return None


def _pair_loops(body, ins):
    """The innermost loop bodies (label ... backward branch) that hold `ins`."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_every_kind_precision_and_count_form_is_compiled_and_the_finish(isa):
    keys = sorted((_key(k) or ("?", k, None) for k in isa), key=str)
    want = [(kind, p, c) for kind in ("context", "ensemble", "ragged") for p in (32, 64) for c in (False, True)] + [("finish", p, None) for p in (32, 64)]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_and_one_tile_of_position_and_velocity_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        kind, precision, _ = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (0 if kind == "finish" else 256 * (32 if precision == 32 else 64)), (name, lds)


def test_the_pair_loops_have_the_specified_operations_per_record_packed_in_fp32_and_no_atomics(isa):
    """Per j record, relative to the 16-byte LDS reads (two per fp32 record: the position and the velocity, both read whole): 6
    packed subtracts and 1 packed add, 5 + 1 packed fma, 1 packed multiply, 2 v_rsq_f32; per pair a compare and two selects, and
    with the count a second compare."""
    for name, (body, desc, meta) in isa.items():
        kind, precision, count = _key(name)
        c = lambda ins, text=body: len(re.findall(r"\b%s" % ins, text))
        assert c(r"(?:global|flat|ds|buffer)_atomic") + c(r"ds_(?:add|min|max)_") == 0, name
        assert c("v_sqrt") == 0 and c("v_rcp_f") == 0, name  # (a ragged kernel divides integers for field_shape: v_rcp_iflag may occur)
        if kind == "finish":
            assert c("v_rsq_") == 0, name
            continue
        if precision == 64:
            loops = _pair_loops(body, "v_rsq_f64")
            assert len(loops) == 2, (name, len(loops))
            for loop in loops:
                pairs = c("v_rsq_f64", loop)  # one seed per pair; a record serves the lane's two bodies
                assert pairs >= 2 and c(r"ds_(?:read|load)_b128", loop) >= pairs, name
                assert c("v_fma_f64", loop) + c("v_fmac_f64", loop) >= 7 * pairs and c("v_add_f64", loop) >= 7 * pairs, name  # 5 + 1 + the Newton step's; 6 + 1
            continue
        loops = _pair_loops(body, "v_pk_fma_f32")
        assert len(loops) == 2, (name, len(loops))  # the masked tile loop and the one without the mask compares
        n_cmp = []
        for loop in loops:
            reads = c(r"ds_(?:read|load)_b128", loop)
            assert reads >= 2 and reads % 2 == 0 and c(r"ds_(?:read|load)_b(?:32|64|96)\b", loop) == 0, (name, reads)  # whole records only
            records = reads // 2
            got = (c("v_pk_add_f32", loop), c("v_pk_fma_f32", loop), c("v_pk_mul_f32", loop), c("v_rsq_f32", loop))
            assert got == (7 * records, 6 * records, records, 2 * records), (name, records, got)
            assert c(r"v_(?:add|sub|mul|fma|fmac)_f32", loop) == 0, name  # nothing unpacked
            assert c("v_cndmask_b32", loop) >= 4 * records, name  # per pair a select of the minimum and one of the index
            n_cmp.append(c("v_cmp_", loop) / records)
        # the loop without the mask: one float compare per pair, two with the count; the masked loop has more
        assert min(n_cmp) == (4 if count else 2), (name, n_cmp)
        assert max(n_cmp) > min(n_cmp), (name, n_cmp)


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _state(rows, T=np.float64):
    """rows of (x, y, z, vx, vy, vz, G m)."""
    cols = list(zip(*rows))
    st = {f: np.array(col, dtype=np.float64) for f, col in zip(R.K.FIELDS, cols)}
    st["mass"] = st["mass"] / R.G
    return {k: v.astype(T) for k, v in st.items()}


@pytest.mark.parametrize("precision", [32, 64])
def test_one_two_and_three_bodies_give_the_closed_forms(precision):
    T = R.DTYPE[precision]
    tol = 8 * R.U[32]  # G m is rounded once when it is stored: the closed forms hold to that
    for f in (R.binaries, R.restate):
        one = f(_state([(0.5, 0.25, -1.0, 1.0, 2.0, 3.0, 1.0)], T), precision)
        assert one["partner"].tolist() == [-1] and one["energy"].tolist() == [np.inf] and one["bound"].tolist() == [0]
        # two bodies 2 apart, G (m_1 + m_2) = 2: B = 2 / sqrt(4 + eps2); at rest bound, at relative speed 2 (A = 2) not
        for speed, bound in ((0.0, 1), (1.0, 1), (2.0, 0)):
            two = f(_state([(-1.0, 0.5, 0.25, 0.0, 0.0, 0.0, 1.0), (1.0, 0.5, 0.25, 0.0, speed, 0.0, 1.0)], T), precision)
            e = 0.5 * speed * speed - 2.0 / math.sqrt(4.0 + EPS2)
            assert two["partner"].tolist() == [1, 0] and two["bound"].tolist() == [bound, bound]
            assert two["energy"][0] == two["energy"][1] and abs(two["energy"][0] - e) <= tol * (0.5 * speed * speed + 1.0)
        # a circular binary of semi-major axis a: e = -G M / (2 a) up to the softening, which is known: G M (1/(2a) - 1/sqrt(a^2 + eps2))
        for a in (0.25, 1.0, 4.0):
            st = {k: np.zeros(2) for k in R.K.FIELDS}
            st["mass"] = np.array([1.0, 3.0]) / R.G
            st["vel_z"][:] = 0.5  # a common velocity does not show
            R.circular_pair(st, 0, 1, a, axis=1)
            got = f({k: v.astype(T) for k, v in st.items()}, precision)
            gm = 4.0
            assert got["partner"].tolist() == [1, 0] and got["bound"].tolist() == [1, 1]
            assert abs(got["energy"][0] - gm * (0.5 / a - 1.0 / math.sqrt(a * a + EPS2))) <= tol * gm / a
            assert abs(got["energy"][0] + gm / (2 * a)) <= gm / a * EPS2 / (2 * a * a)  # -G M / (2 a) up to the softening
        # the hierarchical triple: b close to a, c far out on a circle about a
        st = {k: np.zeros(3) for k in R.K.FIELDS}
        st["mass"] = np.array([2.0, 1.0, 0.25]) / R.G
        R.circular_pair(st, 0, 1, 0.25, axis=0)
        R.circular_pair(st, 0, 2, 4.0, axis=2)
        tri = f({k: v.astype(T) for k, v in st.items()}, precision)
        assert tri["partner"].tolist() == [1, 0, 0] and tri["bound"].tolist() == [2, 1, 1]  # c is bound to a, not to the fast b
        assert abs(tri["energy"][2] - 2.25 * (0.125 - 1.0 / math.sqrt(16.0 + EPS2))) <= tol * 2.25 / 4
        assert tri["energy"][0] == tri["energy"][1] < tri["energy"][2] < 0 and not R.identities(tri)
        # distinct bodies at one position count, with r2 = eps^2; massless bodies moving as one have energy 0 exactly: not bound
        same = f(_state([(1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.5), (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.5)], T), precision)
        assert same["partner"].tolist() == [1, 0] and abs(same["energy"][0] + 1.0 / math.sqrt(EPS2)) <= tol / math.sqrt(EPS2)
        ghosts = f(_state([(0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0), (5.0, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0)], T), precision)
        assert ghosts["partner"].tolist() == [1, 0] and ghosts["energy"].tolist() == [0.0, 0.0] and ghosts["bound"].tolist() == [0, 0]


def device_cases(precision):
    """Every (name, state) the device tests compare with the reference's partner."""
    cases = [("cloud(%d)" % n, R.cloud(n, precision)) for n in R.CONTEXT_SIZES]
    assert set(R.RAGGED_SIZES) <= set(R.CONTEXT_SIZES)  # the ragged members are the contexts' states
    cases += [("reversed_cloud(%d)" % R.ENSEMBLE_N, R.reversed_cloud(R.ENSEMBLE_N, precision))]
    cases += [("clustered(%d)" % n, R.clustered(n, precision)) for n in sorted(R.CLUSTERED_SEEDS)]
    cases += [("encounter", R.encounter(precision))]
    return cases


@pytest.mark.parametrize("precision", [32, 64])
def test_every_state_of_the_device_tests_has_no_ambiguous_partner_and_the_restatement_is_the_plain_definition(precision):
    """The share of device cases left out for ambiguity is 0.  (The lattice is tied exactly and on purpose: the device tests
    hold it to the geometry's closed form, not to the reference's argmin.)"""
    cases = device_cases(precision)
    assert len(cases) == len(R.CONTEXT_SIZES) + 1 + 2 + 1
    shown = 0
    for name, st in cases:
        n = len(st["mass"])
        bad = R.ambiguity(st, precision)
        want = R.binaries(st, precision)
        loose = int((want["bound_lo"] != want["bound_hi"]).sum())
        print("fp%d %-22s: %d ambiguous partners, %d bodies with a pair inside the window around 0, mean bound %.1f of %d, %d unbound bodies"
              % (precision, name, bad, loose, want["bound"].mean(), n - 1, (want["bound"] == 0).sum()))
        assert bad == 0, (precision, name, bad)
        shown += 1
        got = R.restate(st, precision)
        assert all(np.array_equal(got[k], want[k]) for k in R.KEYS), (precision, name)
        assert not R.differs(got, want, st, precision) and not R.identities(want), (precision, name)
        assert ((want["bound_lo"] <= want["bound"]) & (want["bound"] <= want["bound_hi"])).all()
        if n >= 255 and name != "encounter":  # the states are about something: bound and unbound partners, the count nearly always exact
            assert 0.02 * n < want["bound"].mean() < 0.98 * n and loose <= n // 50, (precision, name, loose)
    assert shown == len(cases)  # none left out
    for n in sorted(R.CLUSTERED_SEEDS):  # what was planted is found
        st = R.clustered(n, precision)
        want = R.binaries(st, precision)
        p = R.planted(n)
        for i, j in p["binaries"] + [p["triple"][:2]]:
            assert want["partner"][i] == j and want["partner"][j] == i and want["energy"][i] < -1.0, (n, i, j)
        a, b, c = p["triple"]
        assert R.pair_energy(st, [c], [a])[0][0] < 0 and want["bound"][a] >= 2 and want["bound"][c] >= 1  # a is bound to b and to c
        i, j = p["massless"]
        assert R.pair_energy(st, [i], [j])[0][0] == 0.0 and R.pair_energy(st, [i], [j])[1][0] == 0.0
        assert (want["bound"][list(p["escapers"])] == 0).all() and (want["energy"][list(p["escapers"])] > 100.0).all()
    # the ambiguity measure itself: a runner-up 8 u (A + B) behind is ambiguous, 4 GATE u (A + B) behind is not
    u = R.U[precision]
    for rel, bad in ((8 * u, 1), (4 * R.GATE[precision] * u, 0)):
        far = 1.0 / (1.0 / math.sqrt(1.0 + EPS2) - rel) ** 2 - EPS2  # B smaller by 2 rel (A = 0, s = 2)
        st = _state([(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (-math.sqrt(far), 0.0, 0.0, 0.0, 0.0, 0.0, 1.0),
                     (0.0, 90.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.0, 99.0, 0.0, 0.0, 0.0, 0.0, 1.0)])
        assert R.ambiguity(st, precision) >= bad and (R.ambiguity(st, precision) == 0) == (bad == 0), rel
    assert (field_shape(257, 257)[2], field_shape(513, 513)[0], field_shape(2049, 2049)[2:], field_shape(4097, 4097)) == (1, 2, (2, 5), (9, 17, 4, 5))


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_follows_the_lowest_index_rule_in_both_orders(precision, perm):
    st = R.lattice(precision, perm)
    n = R.LATTICE_K ** 3
    index, _ = NB.lattice_expected(R.LATTICE_K, perm)
    for f in (R.binaries, R.restate):
        got = f(st, precision)
        assert np.array_equal(got["partner"], index) and (got["bound"] == n - 1).all()
        assert len(set(got["energy"].tolist())) == 1  # one distance class, one value
    assert R.ambiguity(st, precision) == n  # tied exactly, by construction: held to the geometry, not to the argmin


FAULT_CASES = (
    ("cloud", 257, ("self not masked", "padding record not masked", "padding velocity read", "m_j alone instead of m_i + m_j")),
    ("cloud", 2049, ("a split row dropped", "indices offset by the member's place")),
    ("clustered", 513, ("<= instead of < in the count",)),
    ("lattice", False, ("ties to the highest j", "finish takes a later split on ties")),
    ("lattice", True, ("ties to the highest j", "finish takes a later split on ties")),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    planted = set()
    for family, arg, faults in FAULT_CASES:
        st = R.lattice(precision, arg) if family == "lattice" else getattr(R, family)(arg, precision)
        want = R.binaries(st, precision)
        if family == "lattice":
            want["partner"] = NB.lattice_expected(R.LATTICE_K, arg)[0]  # what the device test of the lattice holds partner to
        assert not R.differs(R.restate(st, precision), want, st, precision)
        for fault in faults:
            got = R.restate(st, precision, fault=fault, offset=257)
            problems, _ = R.compare(got, want, st, precision)
            print("fp%d %s(%s) %-40s: %s" % (precision, family, arg, fault, "; ".join(problems)))
            assert problems and R.differs(got, want, st, precision), (precision, family, arg, fault)
            planted.add(fault)
    assert planted == set(R.FAULTS) and len(R.FAULTS) == 9
    # what some of the faults are seen by
    st = R.cloud(257, precision)
    want = R.binaries(st, precision)
    own = R.restate(st, precision, fault="self not masked")
    assert (own["partner"] == np.arange(257)).all() and (own["bound"] == want["bound"] + 1).all()
    pad = R.restate(st, precision, fault="padding record not masked")
    assert (pad["bound"] >= want["bound"]).all() and ((pad["bound"] - want["bound"]) % 255 == 0).all() and (pad["bound"] > want["bound"]).any()
    st = R.clustered(513, precision)
    le = R.restate(st, precision, fault="<= instead of < in the count")
    i, j = R.planted(513)["massless"]
    assert np.nonzero(le["bound"] != R.binaries(st, precision)["bound"])[0].tolist() == sorted((i, j))


def test_binary_catalogue_agrees_with_a_plain_loop(nbx):
    for n in sorted(R.CLUSTERED_SEEDS):
        st = R.clustered(n, 64)
        ref = R.binaries(st, 64)
        args = (ref["partner"], ref["energy"], st["mass"]) + tuple(st[k] for k in R.POS + R.VEL)
        got = nbx.binary_catalogue(*args)
        want = R.catalogue(*args)
        assert len(want) >= 4 and got["i"].tolist() == [r[0] for r in want] and got["j"].tolist() == [r[1] for r in want]
        for k, key in enumerate(("energy", "a", "ecc", "period", "binding"), start=2):
            # (a circular orbit's eccentricity is the root of a rounding error: no relative agreement there)
            assert got[key].shape == (len(want),) and np.allclose(got[key], [r[k] for r in want], rtol=1e-12, atol=1e-6 if key == "ecc" else 0.0), key
        assert (np.diff(got["binding"]) <= 0).all() and (got["energy"] < 0).all() and (got["a"] > 0).all() and ((got["ecc"] >= 0) & (got["ecc"] < 1)).all()
        p = R.planted(n)
        for i, j in p["binaries"]:  # planted on circular orbits of the unsoftened problem: a = the separation, ecc = 0
            row = [r for r in want if (r[0], r[1]) == (min(i, j), max(i, j))]
            assert len(row) == 1 and abs(row[0][3] - R.BINARY_SEP) < 1e-9 and row[0][4] < 1e-6, (i, j, row)
    none = nbx.binary_catalogue(np.array([1, 0]), np.array([0.5, 0.5]), np.ones(2), *[np.arange(2.0)] * 6)  # mutual, not bound
    assert none["i"].shape == (0,) and none["binding"].shape == (0,)
