"""The field at caller-supplied points (include/nbx_field.h), the parts that need no GPU: the header and its three exported
symbols, the argument checks that come before the first HIP call, the Python methods, the build files, the shape rule
csrc/nbx_field_shape.hpp against its Python restatement, an audit of the cross-compiled gfx950 code of nbx_field.hip, and the
numpy reference tests/field_ref.py, which must show by itself what the device tests then ask of the library.

Which state catches which planted fault (both precisions; "outside a gate" = K of at least one point above the case's gate):
    (n, m) = (2049, 1025), points uniform in the box, two j splits of 5 and 4 tiles, three columns:
        dropped record (point 700, record 1500), doubled record (point 3, record 2048: the last tile's only body), last tile of the
        last split skipped, split partial added twice (split 1), point index shifted by one, the lane's two points swapped,
        phi without its sign
    (n, m) = (257, 513), all bodies 50 away from the origin in every coordinate, points about the origin:
        padding record with mass (record 257 sits at the origin, among the points), last tile of the last split skipped,
        the lane's two points swapped
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref as R
import force_ref as F
from conftest import ROOT, PKG
from energy_ref import EPS2, gm_as_uploaded

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_field.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h")
ENTRY_POINTS = ("nbx_field", "nbx_ensemble_field", "nbx_ragged_field")
NOUN = {"nbx_field": "ctx", "nbx_ensemble_field": "ensemble", "nbx_ragged_field": "ragged ensemble"}


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


ARGS9 = "const void*, const void*, const void*, void*, void*, void*, void*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_field.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, int32_t, %s) = nbx_field; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, int32_t, %s) = nbx_ensemble_field; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, int32_t, %s) = nbx_ragged_field; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n' % (ARGS9, ARGS9, ARGS9))
PARAMS = ("const void* x, const void* y, const void* z, void* a, void* b, void* c, void* p")
UNUSED = "(void)x; (void)y; (void)z; (void)a; (void)b; (void)c; (void)p; (void)m;"
STUBS = ('#include "nbx_field.h"\n'
         'int nbx_field(nbx_ctx* h, int32_t m, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_field(nbx_ensemble* h, int32_t f, int32_t n, int32_t m, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_field(nbx_ragged* h, int32_t f, int32_t n, int32_t m, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "field_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_three_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_field.h")
    assert declared == sorted(ENTRY_POINTS) and set(declared) == set(nbx.FIELD_SYMBOLS) and len(nbx.FIELD_SYMBOLS) == 3
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "nbx_field" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS) |
                                set(nbx.RAGGED_SYMBOLS) | set(nbx.RAGGED_DIAG_SYMBOLS) | set(nbx.BATCH_ACCEL_SYMBOLS) | set(nbx.KICK_SYMBOLS) |
                                set(nbx.TIMESCALE_SYMBOLS))
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (9 if s == "nbx_field" else 11)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = open(os.path.join(ROOT, "include", "nbx_field.h")).read()
    for word in ("Why:", "Definition", "Per-pair arithmetic", "Semantics", "Status, in this order", "Deliberately not here", "Unspecified results",
                 "no self-exclusion", "a(x_i) is body i's acceleration", "nbx_diag_t.potential", "no mask is needed", "nbx_timescale.h needs one",
                 "a NULL array is never written", "sliced context", "nbx_commit", "synchronises once", "steps_done", "graph replay", "2^22",
                 "32 bits", "1 GiB", "before the first HIP call", "NBX_ERR_ALLOC", "groups", "device pointers", "tidal tensors or jerk",
                 "self-exclusion by index", "reference summation order", "hipGraph", "nbody.x", "the same bits", "not finite"):
        assert word in doc, word


def _call(nbx, name, handle, m, p, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    args = [m] + [ptr(a) for a in p] + [ptr(a) for a in out]
    return f(handle, *args) if name == "nbx_field" else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members and nothing uploaded: it reaches the range
    check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    pts = [np.full(8, 0.25, dtype=np.float64) for _ in range(3)]
    out = [np.full(8, -7.25, dtype=np.float64) for _ in range(4)]
    none3, none4 = [None] * 3, [None] * 4
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for m, p in ((4, pts), (-1, none3)):
        assert _call(nbx, name, None, m, p, out, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. m < 0 -- before the arrays and the range
    assert _call(nbx, name, handle, -1, none3, out, -1, 5) == nbx.NBX_ERR_ARG
    assert err() == name + ": m < 0"
    # 3. m > 0 and a NULL point array -- before the range
    for k in range(3):
        p = list(pts)
        p[k] = None
        assert _call(nbx, name, handle, 4, p, out, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == name + ": NULL point array"
    if name != "nbx_field":
        # 4. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert _call(nbx, name, handle, 4, pts, out, first, count) == nbx.NBX_ERR_ARG, (first, count)
            assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 8. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with points, without, and with m == 0
        assert _call(nbx, name, handle, 4, pts, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, 0, none3, none4, 0, 0) == nbx.NBX_OK
    else:
        # 5. more than 2^22 points -- before the state (the arrays are not read)
        assert _call(nbx, name, handle, (1 << 22) + 1, pts, out) == nbx.NBX_ERR_ARG
        assert err() == "nbx_field: m exceeds 4194304"
        # 6. then the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for m, p, o in ((4, pts, out), (1 << 22, pts, none4), (0, none3, out), (4, pts, none4)):
            assert _call(nbx, name, handle, m, p, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_field: nbx_upload has not been called"
    assert all((a == -7.25).all() for a in out) and zeroed.raw == bytes(1 << 16)


def test_python_methods(nbx):
    p = inspect.signature(nbx.Context.field).parameters
    assert list(p) == ["self", "px", "py", "pz"]
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.field).parameters
        assert list(p) == ["self", "px", "py", "pz", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "field")  # groups: deliberately not here
    assert nbx.FIELD_KEYS == ("acc_x", "acc_y", "acc_z", "phi") == R.KEYS
    assert not [f for f, _ in nbx.Opts._fields_ if "field" in f or "point" in f]  # no new nbx_opts field


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_field\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_field\.o: \$\(CSRC\)/nbx_field\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    assert rule
    for dep in ("nbx_field_kernels.hpp", "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_pair.hpp", "include/nbx_field.h", "include/nbx_ensemble.h",
                "include/nbx_ragged.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_field.hip", "include/nbx_field.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_and_the_shape_rule_includes_nothing():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_field.hip":
            assert "nbx_field_kernels.hpp" not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_field.hip", "nbx_field_kernels.hpp"):
            assert "field_kernel" not in txt and "field_body" not in txt, f
    shape = re.sub(r"//.*", "", open(os.path.join(CSRC, "nbx_field_shape.hpp")).read())
    assert "#include" not in shape and "constexpr FieldShape field_shape(int m, int n)" in shape
    for word in ("multiProcessorCount", "prop", "opts", "hip"):
        assert word not in shape, word  # a function of (m, n) alone
    both = re.sub(r"//.*", "", open(SRC).read() + open(os.path.join(CSRC, "nbx_field_kernels.hpp")).read())
    assert "atomic" not in both
    src = open(SRC).read()
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc is reached through ensure_bytes
    assert "device_alloc(" in shared and "device_alloc(" not in re.sub(r"//.*", "", src)


# ---------------------------------------------------------------------------------------------------------------------------
# the shape rule against its restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_field_shape_of_the_header_is_the_python_restatement(tmp_path):
    pairs = sorted(set([(m, n) for n, m in R.SHAPES] + [(m, n) for n in R.RAGGED_SIZES for _, m in R.SHAPES] +
                       [(1, 1), (1, 1048576), (4194304, 256), (513, 16383), (512, 1024), (513, 1024), (2, 1023), (2, 1025)]))
    exe = str(tmp_path / "field_shape_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "field_shape_driver.cpp"), "-o", exe])
    lines = subprocess.run([exe] + [str(v) for mn in pairs for v in mn], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1] == "max_points %d" % R.MAX_POINTS == "max_points 4194304"
    got = [tuple(int(v) for v in line.split()) for line in lines[:-1]]
    assert got == [(m, n) + R.field_shape(m, n) for m, n in pairs]
    for m, n, columns, tiles, splits, per in got:
        assert columns == -(-m // 512) and tiles == -(-n // 256)
        assert 1 <= splits and (splits - 1) * per < tiles <= splits * per  # every split non-empty, all tiles covered
        assert splits == 1 or per >= 4
    assert R.field_shape(1, 1) == (1, 1, 1, 1) and R.field_shape(1, 1048576) == (1, 4096, 1024, 4)
    assert R.field_shape(4194304, 256) == (8192, 1, 1, 1) and R.field_shape(513, 16383) == (2, 64, 16, 4)
    assert R.field_shape(1025, 2049) == (3, 9, 2, 5) and R.field_shape(4097, 4097) == (9, 17, 4, 5)  # the GPU test's split shapes


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
    out = tmp_path_factory.mktemp("isa") / "nbx_field.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair-work kernel, ("finish", precision) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)field_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+field_finish_kernelI([fd])EE", name)
    if m:
        return ("finish", 32 if m.group(1) == "f" else 64)
    return None


def test_the_kernels_are_the_pair_work_of_three_kinds_in_two_precisions_and_the_finish(isa):
    keys = sorted(_key(k) or ("?", k) for k in isa)
    assert keys == sorted((kind, p) for kind in ("context", "ensemble", "ragged", "finish") for p in (32, 64)), keys


def test_no_scratch_and_no_spills(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name


def test_the_fp32_pair_loop_is_packed_reads_lds_records_whole_and_takes_the_raw_reciprocal_square_root(isa):
    for name, (body, desc, meta) in isa.items():
        kind, precision = _key(name)
        if kind == "finish":
            continue
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == 256 * (16 if precision == 32 else 32), (name, lds)  # one tile of position records
        if precision == 32:
            for ins in ("v_rsq_f32", "v_pk_fma_f32", "v_pk_add_f32", "v_pk_mul_f32"):
                assert re.search(r"\b%s" % ins, body), (name, ins)
            assert re.search(r"\bds_(?:read|load)_b128", body), name
            # the unrolled loop body: per two pairs 13 packed operations -- 3 differences, 7 fused multiply-adds (r2: 3, a: 3, phi: 1),
            # 3 multiplies -- and 2 reciprocal square roots
            loop = max(re.findall(r"\.LBB\d+_\d+:[^\n]*\n(.*?)s_cbranch_\w+ \.LBB", body, re.S), key=lambda b: b.count("v_pk_fma_f32"))
            n_rsq = len(re.findall(r"\bv_rsq_f32", loop))
            assert n_rsq >= 2 and n_rsq % 2 == 0, (name, n_rsq)
            for ins, per_two_pairs in (("v_pk_add_f32", 3), ("v_pk_fma_f32", 7), ("v_pk_mul_f32", 3)):
                assert len(re.findall(r"\b%s" % ins, loop)) == per_two_pairs * n_rsq // 2, (name, ins)
        else:
            assert re.search(r"\bv_rsq_f64", body) and re.search(r"\bv_fma_f64", body), name


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _state(xs, ms, T):
    st = {f: np.zeros(len(ms), dtype=T) for f in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}
    for f, col in zip(R.POS, zip(*xs)):
        st[f] = np.array(col, dtype=T)
    st["mass"] = np.array(ms, dtype=T)
    return st


def _points(ps, T):
    return tuple(np.array(c, dtype=T) for c in zip(*ps))


def _values(state, points, precision):
    """(acc (m, 3), phi (m,)) as fp64 of the truth, and the same of the restatement."""
    tr = R.truth(state, points, precision)
    r = R.restate(state, points, precision)
    return (tr["acc"][0] + tr["acc"][1], tr["phi"][0] + tr["phi"][1]), (np.stack([r[k] for k in R.KEYS[:3]], axis=1).astype(np.float64),
                                                                         r["phi"].astype(np.float64))


@pytest.mark.parametrize("precision", [32, 64])
def test_two_bodies_the_midpoint_and_a_point_on_a_body_give_the_closed_forms(precision):
    T = R.DTYPE[precision]
    st = _state([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)], [3.0e9, 5.0e9], T)  # 2 apart on the x axis, all exactly representable
    gm = gm_as_uploaded(st["mass"])
    pts = _points([(0.0, 0.5, 0.25), (-1.0, 0.5, 0.25)], T)
    f1, f2 = (1.0 + EPS2) ** -1.5, 2.0 * (4.0 + EPS2) ** -1.5
    want_a = np.array([[(gm[1] - gm[0]) * f1, 0, 0],          # the midpoint: the heavier body wins
                       [gm[1] * f2, 0, 0]])                   # on body 0: its own term is an exact zero, body 1 pulls
    want_p = np.array([-(gm[0] + gm[1]) / np.sqrt(1.0 + EPS2),
                       -gm[0] / np.sqrt(EPS2) - gm[1] / np.sqrt(4.0 + EPS2)])  # on body 0: its own term is -G m_0 / eps
    tol = 1e-15 if precision == 64 else 1e-6
    for (a, p), rel in zip(_values(st, pts, precision), (1e-15, tol)):
        assert np.abs(a - want_a).max() <= rel * np.abs(want_a).max(), (a, want_a)
        assert (np.abs(p - want_p) <= rel * np.abs(want_p)).all(), (p, want_p)
        assert (a[:, 1:] == 0).all()
    # the identities of the header: a(x_i) is body i's acceleration, phi(x_i) + G m_i / eps body i's potential
    hand = [h for h in F.hand_placed(precision) if h[0] == "n2_axis"][0]
    own = _points([(-1.0, 0.5, 0.25), (1.0, 0.5, 0.25)], T)
    (a, p), _ = _values(hand[1], own, precision)
    assert np.abs(a - hand[2]).max() <= 1e-15 * np.abs(hand[2]).max()
    body_phi = p + gm / np.sqrt(EPS2)
    assert (np.abs(body_phi - (-gm[::-1] / np.sqrt(4.0 + EPS2))) <= 1e-9 * np.abs(body_phi)).all()  # the cancellation costs digits


def test_a_point_a_thousand_box_sizes_away_sees_the_monopole():
    st = R.make_state(64, 96, "box")
    gm = gm_as_uploaded(st["mass"])
    x = np.stack([st[f] for f in R.POS], axis=1)
    com = (gm[:, None] * x).sum(axis=0) / gm.sum()
    pts = R.make_points(64, st, 5, "far")
    (a, p), (ra, rp) = _values(st, pts, 64)
    d = com[None, :] - np.stack(pts, axis=1)
    r = np.linalg.norm(d, axis=1)
    assert (r > 1.9e3).all()
    want_a, want_p = gm.sum() * d / r[:, None] ** 3, -gm.sum() / r
    for got_a, got_p in ((a, p), (ra, rp)):  # the quadrupole is (size / r)^2 ~ 3e-7 of the monopole, eps^2 / r^2 far less
        assert np.abs(got_a - want_a).max() <= 1e-6 * np.abs(want_a).max()
        assert (np.abs(got_p - want_p) <= 1e-6 * np.abs(want_p)).all()


@pytest.mark.parametrize("precision", [32, 64])
def test_on_the_gpu_tests_states_the_unfaulted_restatement_is_inside_both_gates(oracle, precision):
    for n, m, family in R.cases():
        c = R.case(oracle, precision, n, m, family)
        ka, kp = R.worst(R.restate(c["state"], c["points"], precision), c, precision)
        print("fp%d (n, m) = (%d, %d) %-6s: acc K %.2f of %.1f (K_ref %.2f), phi K %.2f of %.1f (K_ref %.2f)"
              % (precision, n, m, family, ka, c["gate_acc"], c["kref_acc"], kp, c["gate_phi"], c["kref_phi"]))
        assert ka <= c["gate_acc"] and kp <= c["gate_phi"], (precision, n, m, family, ka, kp)
        if n == 1:
            assert c["kref_acc"] == 0.0 and ka == 0.0  # A == 0: exact zeros


FAULT_CASES = (
    ((2049, 1025, "box"), (("dropped record", 700, 1500), ("doubled record", 3, 2048), ("last tile of the last split skipped", -1, -1),
                           ("split partial added twice", -1, 1), ("point index shifted by one", -1, -1),
                           ("the lane's two points swapped", -1, -1), ("phi without its sign", -1, -1))),
    ((257, 513, "origin"), (("padding record with mass", -1, -1), ("last tile of the last split skipped", -1, -1),
                            ("the lane's two points swapped", -1, -1))),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_puts_a_point_outside_a_gate(oracle, precision):
    planted = set()
    for (n, m, family), faults in FAULT_CASES:
        c = R.case(oracle, precision, n, m, family)
        for fault in faults:
            ka, kp = R.worst(R.restate(c["state"], c["points"], precision, fault=fault), c, precision)
            print("fp%d (n, m) = (%d, %d) %-6s %-36s: acc K %.3g of %.1f, phi K %.3g of %.1f"
                  % (precision, n, m, family, fault[0], ka, c["gate_acc"], kp, c["gate_phi"]))
            assert ka > c["gate_acc"] or kp > c["gate_phi"], (precision, n, m, family, fault, ka, kp)
            if fault[0] != "phi without its sign":
                assert ka > c["gate_acc"] and kp > c["gate_phi"], (precision, n, m, family, fault, ka, kp)  # both quantities see it
            planted.add(fault[0])
    assert planted == set(R.FAULTS)
