"""The acceleration of every body and its time derivative (include/nbx_jerk.h), the parts that need no GPU: the header and its
three exported symbols, the argument checks that come before the first HIP call, the Python methods, jerk_dt and hermite, the
build files, an audit of the cross-compiled gfx950 code of nbx_jerk.hip, and the numpy reference tests/jerk_ref.py, which must
show by itself what the device tests then ask of the library: closed forms for 2 and 3 bodies, adot = Omega x a on a rigid
rotation, the central difference of the reference acceleration, that its restatement of the split and finish scheme is the
plain definition within the gate on the states of the device tests, that every planted fault is caught by the comparison of
the device tests, and that a Hermite P(EC) built on the reference jerk is of fourth order where a wrong factor is not.

Which state catches which planted fault:
    cloud(2049), both precisions: the factor 3, the sign of the second term, r2^(-3/2) used for r2^(-5/2), u taken from the
        wrong j record, the lane's second body using the first one's velocity (2049 > 256), a split dropped (two splits)
    cloud(2049), fp64: the fp64 scale not undone, 1/r2 left at the raw seed in fp64
    cloud(257), both precisions: padding velocities read as the next system's (255 padding records)
    the lattice in H x + Omega x x: u taken from the wrong j record and the lane's second body using the first one's velocity,
        at the sampled rows
"""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import jerk_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_jerk.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_jerk_kernels.hpp"
ENTRY_POINTS = ("nbx_jerk", "nbx_ensemble_jerk", "nbx_ragged_jerk")
NOUN = {"nbx_jerk": "ctx", "nbx_ensemble_jerk": "ensemble", "nbx_ragged_jerk": "ragged ensemble"}
OTHER_TUPLES = ("SYMBOLS", "DIAG_SYMBOLS", "ENSEMBLE_SYMBOLS", "ENSEMBLE_DIAG_SYMBOLS", "RAGGED_SYMBOLS", "RAGGED_DIAG_SYMBOLS",
                "BATCH_ACCEL_SYMBOLS", "KICK_SYMBOLS", "TIMESCALE_SYMBOLS", "FIELD_SYMBOLS", "NEIGHBOUR_SYMBOLS", "PAIRCOUNT_SYMBOLS",
                "TRACER_SYMBOLS", "KNN_SYMBOLS", "FOF_SYMBOLS", "BINARIES_SYMBOLS", "TIDAL_SYMBOLS", "CLUMPS_SYMBOLS", "NLIST_SYMBOLS")
HEADER_FORBIDDEN = ("nbx_field", "nbx_tidal", "nbx_timescale", "_neighbours", "_binaries", "_clumps", "_fof", "_knn", "_nlist", "tracers_")
FORBIDDEN = ("neighbour_kernel", "nb_body", "field_kernel", "field_body", "timescale_kernel", "tracer_kernel", "tracer_body",
             "tracer_update_kernel", "knn_kernel", "knn_body", "knn_insert", "fof_pass_kernel", "fof_body", "fof_hook_kernel", "JLANE_EPI",
             "bound_kernel", "bound_body", "bound_finish_kernel", "tidal_kernel", "tidal_body", "clump_kernel", "clump_body",
             "clump_finish_kernel", "nlist_kernel", "nl_body", "nlist_scan")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_jerk.h"\n'
           'int main(void) { '
           'nbx_jerk_out_t o = {{0}, {0}}; '
           'int (*a)(nbx_ctx*, const nbx_jerk_out_t*) = nbx_jerk; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, const nbx_jerk_out_t*) = nbx_ensemble_jerk; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, const nbx_jerk_out_t*) = nbx_ragged_jerk; '
           'o.acc[2] = o.jerk[2] = NULL; '
           'printf("ok %d\\n", (int)(sizeof(o) / sizeof(void*))); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')
STUBS = ('#include "nbx_jerk.h"\n'
         'int nbx_jerk(nbx_ctx* h, const nbx_jerk_out_t* o) { (void)h; (void)o; return 0; }\n'
         'int nbx_ensemble_jerk(nbx_ensemble* h, int32_t f, int32_t n, const nbx_jerk_out_t* o) { (void)h; (void)f; (void)n; (void)o; return 0; }\n'
         'int nbx_ragged_jerk(nbx_ragged* h, int32_t f, int32_t n, const nbx_jerk_out_t* o) { (void)h; (void)f; (void)n; (void)o; return 0; }\n')


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "jerk_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok 6\n"  # six pointers, nothing else


def test_declared_set_is_the_three_symbols_exported_and_apart_from_every_other_tuple(nbx):
    declared = _declared("nbx_jerk.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.JERK_SYMBOLS) == ENTRY_POINTS and len(nbx.JERK_SYMBOLS) == 3
    assert nbx.JERK_KEYS == R.KEYS == ("acc_x", "acc_y", "acc_z", "jerk_x", "jerk_y", "jerk_z")
    assert ctypes.sizeof(nbx.JerkOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    for h in sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h != "nbx_jerk.h"):
        assert not set(declared) & set(_declared(h)), h
        assert "_jerk" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    for t in OTHER_TUPLES:
        assert not set(declared) & set(getattr(nbx, t)), t
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (2 if s == "nbx_jerk" else 4)
    assert sorted(re.findall(r" T (nbx_\w*jerk\w*)$", out, flags=re.M)) == declared  # exactly three new exported symbols
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()


def test_the_header_has_its_contract_words_and_none_of_the_forbidden_strings():
    raw = open(os.path.join(ROOT, "include", "nbx_jerk.h")).read()
    for word in HEADER_FORBIDDEN:
        assert word not in raw, word
    doc = re.sub(r"\n \*\s*", " ", raw)  # the comment as running text
    for word in ("Why:", "Definition", "Masks:", "Per-pair arithmetic in fp32", "Per-pair arithmetic in fp64", "Sums and finish",
                 "Error of one term", "Operation count", "Contracts:", "Arrays:", "Contexts:", "Semantics", "Status, in this order",
                 "Unspecified results", "Deliberately not here", "fma(dx,dx, fma(dy,dy, fma(dz,dz, eps2)))",
                 "a_i    = sum over j < n of gm_j d / r2^(3/2)", "adot_i = sum over j < n of gm_j [ u / r2^(3/2) - 3 (d.u) d / r2^(5/2) ]",
                 "j == i is NOT masked", "exact zeros", "A velocity is loaded only where j < n", "never read",
                 "inv = rsq(r2);  inv2 = inv*inv;  s = (gm*inv)*inv2;  a += d*s  (fma)",
                 "rv = fma(dx,ux, fma(dy,uy, dz*uz));  c = (rv*inv2)*(-3);  t_a = fma(c, d_a, u_a);  adot_a += t_a*s  (fma)",
                 "two separately rounded multiplies", "mul_rn / add_rn", "fma(h, fma(h, 15, 12), 8)", "inv2 = fma(y2, fma(h, h, h), y2)",
                 "G*m/8", "j ascending within a split", "in fp64 in split order and rounds once", "17.5u", "35.5u", "13.5u", "29.5u",
                 "26 packed VALU and 2 v_rsq_f32", "against 13 and 2", "the same bits on every call", "bit for bit what nbx_jerk returns",
                 "acc is bit for bit the acceleration the field call returns", "m = n", "a NULL array is never written", "member-major",
                 "end to end", "sliced context", "is refused", "nbx_commit", "synchronises once", "one finish launch", "one read-back",
                 "no atomics", "steps_done", "*_timed / *_ms_total", "kinetic-energy partials", "the state of graph replay", "out is NULL",
                 "checked in 64 bits", "2^22", "names the first such member", "the velocities of the others are not resident",
                 "all six pointers NULL", "before the first HIP call", "NBX_ERR_ALLOC", "not finite", "of that system alone",
                 "groups and sliced contexts", "caller-supplied points", "snap and crackle", "per-body maxima", "resident Hermite stepper",
                 "device pointers", "hipGraph", "nbody.x"):
        assert word in doc, word
    # the gap, named where the issue found it
    for other in ("nbx_field.h", "nbx_tidal.h"):
        assert "jerk" in open(os.path.join(ROOT, "include", other)).read(), other


def _call(nbx, name, handle, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    o = None if out is None else ctypes.byref(out)
    return f(handle, o) if name == "nbx_jerk" else f(handle, first, count, o)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    arrays = {k: np.full(8, -7.0) for k in R.KEYS}
    a = [arrays[k].ctypes.data for k in R.KEYS]
    out = nbx.JerkOut((ctypes.c_void_p * 3)(*a[:3]), (ctypes.c_void_p * 3)(*a[3:]))
    none = nbx.JerkOut()
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for o in (out, None, none):
        assert _call(nbx, name, None, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. out is NULL -- before the range and the state
    assert _call(nbx, name, handle, None, -1, 5) == nbx.NBX_ERR_ARG
    assert err() == name + ": out is NULL"
    if name != "nbx_jerk":
        # 3. the range leaves [0, members): the zeroed object has none -- also where nothing is asked for
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            for o in (out, none):
                assert _call(nbx, name, handle, o, first, count) == nbx.NBX_ERR_ARG, (first, count)
                assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 8. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with outputs and without
        assert _call(nbx, name, handle, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, none, 0, 0) == nbx.NBX_OK
    else:
        # 5. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for o in (out, none):
            assert _call(nbx, name, handle, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_jerk: nbx_upload has not been called"
    assert all((v == -7).all() for v in arrays.values()) and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_and_the_refusals_are_in_the_source_in_the_stated_order():
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    assert "constexpr long long kJerkMaxBodies = kFieldMaxPoints;" in hdr
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_jerk: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kJerkMaxBodies" in src and "range_bodies(o, first, count) > kJerkMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_jerk("):]
    order = [batch.index(w) for w in ("is NULL", "out is NULL", "check_range(", "kJerkMaxBodies", "check_uploaded(", "no_output(*out)", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_jerk("):]
    order = [ctx.index(w) for w in ("ctx is NULL", "out is NULL", "kJerkMaxBodies", "->uploaded", "pending_commit",
                                    "c->i_begin != 0 || c->i_count != c->n", "no_output(*out)", "use_device(")]
    assert order == sorted(order)
    text = "the context owns a slice of the bodies (the velocities of the others are not resident)"
    assert 'fail(NBX_ERR_STATE, "nbx_jerk: %s")' % text in ctx and '"nbx_jerk: a local step awaits nbx_commit"' in ctx
    # the read-back is the shared skeleton's: no synchronisation and no copy of the call's own, one use of the helper, and in the
    # helper's body one copy, one synchronisation and the one of the failure path
    assert "hipStreamSynchronize" not in src and "hipMemcpy" not in src and len(re.findall(r"\bread_back\(", src)) == 1
    helper = shared[shared.index("int read_back("):]
    helper = helper[:helper.index("\n}\n")]
    assert len(re.findall(r"hipStreamSynchronize\(o->stream\)", helper)) == 2 and len(re.findall(r"hipStreamSynchronize\(", helper)) == 2
    assert len(re.findall(r"hipMemcpyAsync\(", helper)) == 1 and "hipMemcpyDeviceToHost" in helper  # one read-back
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == 4  # three kinds, one finish


class _Fake:
    pass


def test_python_methods_jerk_dt_and_hermite_are_as_specified(nbx):
    assert list(inspect.signature(nbx.Context.jerk).parameters) == ["self"]
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.jerk).parameters
        assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "jerk")  # groups: deliberately not here
    assert not [f for f, _ in nbx.Opts._fields_ if "jerk" in f]  # no new nbx_opts field
    assert list(inspect.signature(nbx.jerk_dt).parameters) == ["result", "eta"]
    assert list(inspect.signature(nbx.hermite).parameters) == ["obj", "dt", "nsteps"]
    res = {"acc_x": np.array([3.0, 0.0, 1.0, 0.0], dtype=np.float32), "acc_y": np.array([4.0, 0.0, 2.0, 0.0], dtype=np.float32),
           "acc_z": np.array([0.0, 0.0, 2.0, 0.0], dtype=np.float32), "jerk_x": np.array([0.0, 1.0, 0.0, 0.0], dtype=np.float32),
           "jerk_y": np.array([0.0, 0.0, 0.0, 0.0], dtype=np.float32), "jerk_z": np.array([10.0, 0.0, 0.0, 0.0], dtype=np.float32)}
    dt = nbx.jerk_dt(res, 0.02)
    assert dt.dtype == np.float64 and dt.tolist() == [0.02 * 5.0 / 10.0, 0.0, math.inf, math.inf]  # |adot| = 0: +inf, also where a = 0
    assert nbx.jerk_dt({k: v.reshape(2, 2) for k, v in res.items()}, 0.02).shape == (2, 2)
    for obj in (object(), _Fake(), None, nbx.Group):
        with pytest.raises(nbx.NbxError) as e:
            nbx.hermite(obj, 0.01, 1)
        assert e.value.code == nbx.NBX_ERR_ARG
    doc = " ".join(nbx.hermite.__doc__.split())
    for word in ("one upload and one read-back of O(n) per step", "steps_done", "energies", "downloaded once at the start", "P(EC)"):
        assert word in doc, word


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_jerk\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_jerk\.o: \$\(CSRC\)/nbx_jerk\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    other = re.search(r"^\$\(PKG\)/nbx_binaries\.o: \$\(CSRC\)/nbx_binaries\.hip(.*)\n", mk, re.M)
    assert rule and rule.group(1) == other.group(1).replace("binaries", "jerk")  # the same dependency list
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_jerk.hip", "include/nbx_jerk.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_reuse_the_shape_rule_and_keep_to_the_naming_rules():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_jerk.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_jerk.hip", KERNELS):
            assert "jerk_kernel" not in txt and "jerk_body" not in txt and "jerk_finish_kernel" not in txt, f
    src = open(SRC).read()
    kern = open(os.path.join(CSRC, KERNELS)).read()
    both = re.sub(r"//.*", "", src + kern)
    for word in FORBIDDEN:
        assert word not in src + kern, word  # comments included: the other features' tests read every file
    assert not re.search(r"nbx_(?!jerk)\w+_kernels\.hpp", src + kern)  # no other feature's kernels, not even by name
    assert "field_shape(" in both and '#include "nbx_field_shape.hpp"' in kern  # the field's rule, no new one
    assert "diag_splits" not in src + kern and not re.search(r"constexpr\s+\w+\s+\w*shape\w*\s*\(", both)
    assert "fmaT(dx, dx, fmaT(dy, dy, fmaT(dz, dz, softening2<double>())))" in kern  # r2 restated, not shared
    assert "atomic" not in both
    assert "__shared__ T4 ptile[kTile];" in kern and "__shared__ T4 vtile[kTile];" in kern  # two arrays per tile
    code = re.sub(r"//.*", "", kern)
    walk = re.sub(r"//.*", "", open(os.path.join(CSRC, "nbx_tilewalk.hpp")).read())  # the two-array walk lives in the shared device layer
    assert "TileWalk2<T4> walk(posm, velm, n, split, tiles_per_split);" in code and "velm[j]" not in code
    assert walk.count("velm[j]") == 2 and len(re.findall(r"if \(j < n\) next_v = velm\[j\];", walk)) == 2  # only below n
    assert code.count("velm[li]") == 1 and "if (li < n) {\n      p = posm[li];\n      v = velm[li];" in code
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("jerk_part", "jerk_out", "jerk_tab"):
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
    out = tmp_path_factory.mktemp("isa") / "nbx_jerk.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair-work kernel, ("finish", precision) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)jerk_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+jerk_finish_kernelI([fd])EE", name)
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


def test_the_pair_loops_have_the_headers_operations_per_record_packed_in_fp32_and_no_atomics(isa):
    """Per j record, relative to the 16-byte LDS reads (two per fp32 record: the position and the velocity, both read whole): the
    header's 26 packed VALU -- 6 packed adds (the subtracts of d and u), 14 packed fma (3 r2, 2 rv, 3 a, 3 t, 3 adot) and 6
    packed multiplies (rv, inv2, the two of s, the two of c) --, 2 v_rsq_f32 and nothing unpacked.  fp64, per pair: one seed, 19
    fma (3 r2, 2 rv, the residual, 2 of the cube's polynomial, 2 of 1/r2, 3 t, 6 sums), 7 multiplies, 6 subtracts."""
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
            assert len(loops) == 1, (name, len(loops))
            pairs = c("v_rsq_f64", loops[0])  # one seed per pair; a record serves the lane's two bodies
            assert pairs >= 2 and pairs % 2 == 0, (name, pairs)
            got = (c("v_fma_f64", loops[0]) + c("v_fmac_f64", loops[0]), c("v_mul_f64", loops[0]), c("v_add_f64", loops[0]))
            assert got == (19 * pairs, 7 * pairs, 6 * pairs), (name, pairs, got)
            continue
        loops = _pair_loops(body, "v_pk_fma_f32")
        assert len(loops) == 1, (name, len(loops))  # nothing is masked: one loop
        loop = loops[0]
        reads = c(r"ds_(?:read|load)_b128", loop)
        assert reads >= 2 and reads % 2 == 0 and c(r"ds_(?:read|load)_b(?:32|64|96)\b", loop) == 0, (name, reads)  # whole records only
        records = reads // 2
        got = (c("v_pk_add_f32", loop), c("v_pk_fma_f32", loop), c("v_pk_mul_f32", loop), c("v_rsq_f32", loop))
        assert got == (6 * records, 14 * records, 6 * records, 2 * records), (name, records, got)
        assert sum(got[:3]) == 26 * records
        assert c(r"v_(?:add|sub|subrev|mul|fma|fmac|mad|mac)_f32", loop) == 0, name  # nothing unpacked


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _state(rows, T=np.float64):
    """rows of (x, y, z, vx, vy, vz, G m)."""
    st = {f: np.array(col, dtype=np.float64) for f, col in zip(R.POS + R.VEL + ("mass",), zip(*rows))}
    st["mass"] = st["mass"] / float(R.G32)
    return {k: v.astype(T) for k, v in st.items()}


def _values(f, st, precision):
    if f is R.truth:
        tr = R.truth(st, precision)
        return np.concatenate([tr["acc"][0], tr["jerk"][0]], axis=1)
    got = f(st, precision)
    return np.stack([got[k].astype(np.float64) for k in R.KEYS], axis=1)


@pytest.mark.parametrize("precision", [32, 64])
def test_two_and_three_bodies_give_the_closed_forms(precision):
    T = R.DTYPE[precision]
    tol = 64 * R.U[32]  # G m is rounded once when it is stored: the closed forms hold to that
    D, u = 2.0, (0.5, -1.0, 0.25)
    r2 = D * D + EPS2
    for f in (R.truth, R.restate):
        # two bodies D apart along x, G m = 1 and 3, relative velocity u: for body 0 d = (D, 0, 0), d.u = D u_x
        st = _state([(-1.0, 0.5, 0.25, 1.0, 2.0, 3.0, 1.0), (-1.0 + D, 0.5, 0.25, 1.0 + u[0], 2.0 + u[1], 3.0 + u[2], 3.0)], T)
        two = _values(f, st, precision)
        a0 = 3.0 * D / r2 ** 1.5
        j0 = [3.0 * (u[0] / r2 ** 1.5 - 3.0 * D * u[0] * D / r2 ** 2.5), 3.0 * u[1] / r2 ** 1.5, 3.0 * u[2] / r2 ** 1.5]
        assert np.allclose(two[0], [a0, 0.0, 0.0] + j0, rtol=tol, atol=tol)
        assert np.allclose(two[1], [-a0 / 3.0, 0.0, 0.0] + [-x / 3.0 for x in j0], rtol=tol, atol=tol)  # momentum: gm_0 a_0 = -gm_1 a_1
        # a third body H up the y axis from body 0, at rest relative to it, G m = 2: its term for body 0 is along y and adds no jerk
        H = 1.5
        st3 = _state([(-1.0, 0.5, 0.25, 1.0, 2.0, 3.0, 1.0), (-1.0 + D, 0.5, 0.25, 1.0 + u[0], 2.0 + u[1], 3.0 + u[2], 3.0),
                      (-1.0, 0.5 + H, 0.25, 1.0, 2.0, 3.0, 2.0)], T)
        three = _values(f, st3, precision)
        assert np.allclose(three[0], [a0, 2.0 * H / (H * H + EPS2) ** 1.5, 0.0] + j0, rtol=tol, atol=tol)
        # total momentum: sum gm_i a_i = 0 and sum gm_i adot_i = 0
        gm = np.array([1.0, 3.0, 2.0])
        assert np.abs((gm[:, None] * three).sum(axis=0)).max() <= 16 * tol
        # one body: nothing
        one = _values(f, _state([(0.5, 0.25, -1.0, 1.0, 2.0, 3.0, 1.0)], T), precision)
        assert (one == 0).all()


@pytest.mark.parametrize("precision", [32, 64])
def test_a_rigid_rotation_has_adot_equal_to_omega_cross_a(precision):
    for n in (513, 2049):
        c = R.case(precision, n, "rotation")
        a, j = c["truth"]["acc"][0], c["truth"]["jerk"][0]
        want = np.stack([-R.OMEGA * a[:, 1], R.OMEGA * a[:, 0], np.zeros(len(a))], axis=1)
        assert np.abs(j - want).max() <= 64 * R.U[64] * c["truth"]["jerk"][2].max()  # to rounding of the truth, relative to its scale
        assert np.abs(j).max() > 1.0


def test_the_central_difference_of_the_reference_acceleration_is_the_reference_jerk():
    for n, fam in ((257, "cloud"), (257, "clustered"), (513, "rotation")):
        st = R.make_state(64, n, fam)
        tr = R.truth(st, 64)
        h = 2.0 ** -20
        moved = []
        for sign in (1.0, -1.0):
            s = {k: v.copy() for k, v in st.items()}
            for p, v in zip(R.POS, R.VEL):
                s[p] = st[p] + sign * h * st[v]
            moved.append(R.truth(s, 64)["acc"][0])
        diff = (moved[0] - moved[1]) / (2.0 * h)
        # the difference quotient leaves h^2 / 6 of the third derivative -- (|u| / eps)^2 of the jerk at most, 2e6 for the planted
        # pair, times h^2 = 1e-12 -- and the fp64 positions' rounding over 2h, 1e-10: 1e-3 of the jerk's scale is far above both
        # (a wrong factor or sign in the (d.u) term changes the jerk by the order of its scale)
        err = np.abs(diff - tr["jerk"][0]) / tr["jerk"][2]
        print(fam, n, float(err.max()))
        assert err.max() < 1e-3, (fam, n, float(err.max()))
        for fault in R.FAULTS[:3] if fam != "rotation" else ():  # a rigid rotation has d.u = 0 in every pair
            _, bad = R.direct(st, fault)
            assert (np.abs(bad.T - diff) / tr["jerk"][2]).max() > 0.05, fault


def _device_cases(precision):
    """Every (name, case, rows) the device tests compare with the reference."""
    cases = [("%s(%d)" % (fam, n), R.case(precision, n, fam)) for n, fam in R.context_cases()]
    assert {(R.ENSEMBLE[1], f) for f in R.ENSEMBLE_FAMILIES} <= set(R.context_cases())
    assert {(n, "cloud") for n in R.RAGGED_SIZES} <= set(R.context_cases())
    return (cases + [("lattice perm=%d" % perm, R.lattice_case(precision, perm)) for perm in (False, True)] +
            [("lattice large", R.large_case(precision))])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_restatement_is_the_plain_definition_within_the_gate_on_the_states_of_the_device_tests(precision):
    cases = _device_cases(precision)
    for name, c in cases:
        rows = c["truth"]["rows"]
        got = R.restate(c["state"], precision, rows=rows if name.startswith("lattice") else None)
        problems, ks = R.compare(got, c["truth"], c["gates"], precision)
        print("fp%d %s: K_ref %s gates %s" % (precision, name, {k: round(v, 1) for k, v in c["kref"].items()}, c["gates"]))
        assert not problems, (precision, name, problems)
        assert c["gates"]["acc"] >= R.F.M * max(R.F.K_TERM, R.FLOOR["acc"][precision])
        assert c["gates"]["jerk"] >= R.F.M * max(R.F.K_TERM, R.FLOOR["jerk"][precision])
        if name != "lattice large":  # whose one split sums 531 456 terms in T one after the other
            assert c["gates"]["jerk"] <= 4 * R.F.M * R.FLOOR["jerk"][precision]  # no restatement so poor that its gate says nothing
    assert len(cases) == len(R.context_cases()) + 3
    assert R.FR.field_shape(R.LARGE_K ** 3, R.LARGE_K ** 3) == (1038, 2076, 1, 2076)
    assert (R.FR.field_shape(257, 257)[2], R.FR.field_shape(513, 513)[0], R.FR.field_shape(2049, 2049)[2:]) == (1, 2, (2, 5))
    n = R.LATTICE_K ** 3
    assert R.FR.field_shape(n, n)[0] == 71 and R.FR.field_shape(n, n)[2] == 15 and {0, n - 1, 511, 512} <= set(R.lattice_rows().tolist())
    rest = R.case(precision, 513, "rest")
    assert (rest["truth"]["jerk"][2] == 0).all() and all((R.restate(rest["state"], precision)[k] == 0).all() for k in R.JERK)


FAULT_CASES = (
    (2049, "cloud", R.FAULTS[:6], R.FP64_FAULTS),
    (257, "cloud", ("padding velocities read as the next system's",), ()),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_is_caught_by_the_comparison_of_the_device_tests(precision):
    planted = set()
    for n, fam, faults, wide in FAULT_CASES:
        c = R.case(precision, n, fam)
        assert not R.compare(R.restate(c["state"], precision), c["truth"], c["gates"], precision)[0]
        for fault in faults + (wide if precision == 64 else ()):
            problems, _ = R.compare(R.restate(c["state"], precision, fault=fault), c["truth"], c["gates"], precision)
            print("fp%d %s(%d) %-56s: %s" % (precision, fam, n, fault, "; ".join(problems)))
            assert problems, (precision, n, fam, fault)
            planted.add(fault)
    assert planted == set(R.FAULTS if precision == 64 else R.FAULTS[:7]) and len(R.FAULTS) == 9
    # the lattice's exact velocities catch the two pairing faults at the sampled rows as well
    c = R.lattice_case(precision, False)
    for fault in ("u taken from the wrong j record", "the lane's second body using the first one's velocity"):
        assert R.compare(R.restate(c["state"], precision, fault=fault, rows=c["truth"]["rows"]), c["truth"], c["gates"], precision)[0], fault


def test_a_numpy_hermite_on_the_reference_jerk_is_of_fourth_order_and_a_wrong_factor_is_not():
    """The fixed states of the device test (96 bodies, T = 0.25), dt = T / 16 against dt / 2, both measured against dt / 16: a
    fourth-order scheme gains 16 per halving and a second-order one 4; the planted factor leaves a first-order error in every
    evaluation's adot, hence second order at best."""
    for seed in R.HERMITE_SEEDS:
        s0 = R.hermite_state(seed)
        n1 = R.HERMITE_STEPS
        ref = R.hermite(s0, R.HERMITE_T / (16 * n1), 16 * n1)
        e1 = R.state_error(R.hermite(s0, R.HERMITE_T / n1, n1), ref)
        e2 = R.state_error(R.hermite(s0, R.HERMITE_T / (2 * n1), 2 * n1), ref)
        f1 = R.state_error(R.hermite(s0, R.HERMITE_T / n1, n1, fault="the factor 3"), ref)
        f2 = R.state_error(R.hermite(s0, R.HERMITE_T / (2 * n1), 2 * n1, fault="the factor 3"), ref)
        print("seed %d: errors %.3g %.3g ratio %.1f; with the factor-3 fault %.3g %.3g ratio %.1f" % (seed, e1, e2, e1 / e2, f1, f2, f1 / f2))
        assert e1 / e2 >= 12.0, (seed, e1, e2)
        assert f1 / f2 < 6.0 and f2 > e2, (seed, f1, f2)
