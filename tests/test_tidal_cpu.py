"""The tidal tensor at caller-supplied points and at the bodies (include/nbx_tidal.h), the parts that need no GPU: the numpy
reference tests/tidal_ref.py on its own -- truth against finite differences of the field, the two identities of the header, the
unfaulted restatement inside the gate on every case the device tests use and every planted fault outside it --, the header and
its six exported symbols, the argument checks that come before the first HIP call, the Python methods and host helpers, the build
files, and an audit of the cross-compiled gfx950 code of nbx_tidal.hip.

Which case catches which planted fault (both precisions; "outside the gate" = K of at least one point above the case's gate):
    points, (n, m) = (2049, 1025), uniform in the box, two j splits of 5 and 4 tiles, three columns:
        dropped record (point 700, record 1500), doubled record (point 3, record 2048: the last tile's only body), last tile of the
        last split skipped, split partial added twice (split 1), point index shifted by one, the lane's two points swapped,
        xy and yz exchanged, the factor 3 missing, Q not subtracted
    points, (n, m) = (257, 513), all bodies 50 away from the origin in every coordinate, points about the origin:
        padding record with mass (record 257 sits at the origin, among the points)
    bodies, n = 1025, the cloud: the self term kept in bodies mode, a neighbour masked instead of self, the lane's two points
        swapped, last tile of the last split skipped
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref as FR
import force_ref as F
import tidal_ref as R
from conftest import ROOT, PKG
from energy_ref import EPS2, gm_as_uploaded

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_tidal.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
KERNELS = "nbx_tidal_kernels.hpp"
POINT_ENTRIES = ("nbx_tidal", "nbx_ensemble_tidal", "nbx_ragged_tidal")
BODY_ENTRIES = ("nbx_tidal_bodies", "nbx_ensemble_tidal_bodies", "nbx_ragged_tidal_bodies")
ENTRY_POINTS = POINT_ENTRIES + BODY_ENTRIES
NOUN = {"nbx_tidal": "ctx", "nbx_ensemble_tidal": "ensemble", "nbx_ragged_tidal": "ragged ensemble",
        "nbx_tidal_bodies": "ctx", "nbx_ensemble_tidal_bodies": "ensemble", "nbx_ragged_tidal_bodies": "ragged ensemble"}
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h", "nbx_timescale.h", "nbx_neighbours.h", "nbx_paircount.h", "nbx_tracers.h", "nbx_knn.h", "nbx_fof.h",
                 "nbx_binaries.h")


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
def _full(tr):
    return tr[0] + tr[1]


def test_truth_is_the_central_difference_of_the_fields_acceleration():
    """T_ab = d a_a / d p_b.  f(t) = a_a(p + t e_b) of one body is G m x r^-3 along its own axis at worst, whose third derivative
    is G m (-9 r^-5 + 90 x^2 r^-7 - 105 x^4 r^-9), at most 204 G m r2^(-5/2) in magnitude; a central difference of step h is off
    by h^2 / 6 of that somewhere within h of p -- r2^(-5/2) moves by less than 5 % there, h / eps being 2.4e-4 -- plus the rounding
    of the two accelerations, each a sum of n terms in the wide type: (n + 10) eps_wide A_acc / h."""
    n, m, h = 96, 7, 2.0 ** -17
    state = FR.make_state(64, n, "box")
    points = FR.make_points(64, state, m, "box")
    wide = R._wide(64)
    T = _full(R.truth(state, points, 64))
    m3 = -R.trace_truth(state, points, 64) / (3 * EPS2)  # sum_j G m_j r2^(-5/2)
    worst = 0.0
    for b in range(3):
        plus, minus = ([np.asarray(p).astype(wide) + (h if c == b else 0) for c, p in enumerate(points)],
                       [np.asarray(p).astype(wide) - (h if c == b else 0) for c, p in enumerate(points)])
        ap, am = FR.truth_at(state, plus, 64)["acc"], FR.truth_at(state, minus, 64)["acc"]
        fd = ((ap[0] - am[0]) + (ap[1] - am[1])) / (2 * h)  # (m, 3): d a_a / d p_b for a = 0, 1, 2
        tol = h * h / 6 * 1.05 * 204 * m3 + (n + 10) * float(np.finfo(wide).eps) * np.maximum(ap[2], am[2]) / h
        for a in range(3):
            c = R.PAIRS.index((min(a, b), max(a, b)))
            err = np.abs(fd[:, a] - T[:, c])
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (a, b, err, tol)
            assert (tol <= 1e-4 * np.abs(T).max(axis=1)).all()  # the comparison means something: four digits at least
    print("largest |central difference - truth| / tolerance: %.3g" % worst)


@pytest.mark.parametrize("precision", [32, 64])
def test_the_two_identities_hold_for_truth(precision):
    n = 300
    state = R.body_state(precision, n, "cloud")
    own = R.positions(state)
    tp, tb = R.truth(state, own, precision), R.truth(state, None, precision, bodies=True)
    # the trace: -3 eps^2 sum G m r2^(-5/2) <= 0, in both modes
    for tr, bodies in ((tp, False), (tb, True)):
        want = R.trace_truth(state, own, precision, bodies=bodies)
        got = _full(tr)[:, R.DIAG].sum(axis=1)
        assert (want < 0).all() and (np.abs(got - want) <= 1e-13 * tr[2][:, R.DIAG].sum(axis=1)).all()
    # points mode at x_i = bodies mode at i - G m_i / eps^3 on the diagonal
    self_term = gm_as_uploaded(state["mass"]) / EPS2 ** 1.5
    want = _full(tb)
    want[:, R.DIAG] -= self_term[:, None]
    assert (np.abs(_full(tp) - want) <= 1e-13 * tp[2]).all()
    assert (np.abs(_full(tb)[:, 0]) < 0.1 * self_term).any()  # which is why the self term must never be formed
    # a different body at the same place counts, through its delta_ab term only
    two = {f: np.zeros(2, dtype=R.DTYPE[precision]) for f in FR.make_state(precision, 2, "box")}
    two["mass"][:] = 3.0e9
    t = _full(R.truth(two, None, precision, bodies=True))
    g = float(gm_as_uploaded(two["mass"])[0]) / EPS2 ** 1.5
    assert np.allclose(t[:, R.DIAG], -g, rtol=1e-12) and (t[:, [1, 2, 4]] == 0).all()


def test_two_bodies_on_an_axis_give_the_closed_form():
    T = np.float64
    st = {f: np.zeros(2, dtype=T) for f in FR.make_state(64, 2, "box")}
    st["pos_x"][:] = (-1.0, 1.0)
    st["mass"][:] = (3.0e9, 5.0e9)
    gm = gm_as_uploaded(st["mass"])
    r2 = 4.0 + EPS2
    for i, j in ((0, 1), (1, 0)):  # at body i, from body j alone: stretched along x, compressed across
        want = np.array([gm[j] * (12.0 * r2 ** -2.5 - r2 ** -1.5), 0, 0, -gm[j] * r2 ** -1.5, 0, -gm[j] * r2 ** -1.5])
        for got in (_full(R.truth(st, None, 64, bodies=True))[i], R.restate(st, None, 64, bodies=True)[i].astype(np.float64)):
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), (got, want)


@pytest.mark.parametrize("precision", [32, 64])
def test_on_the_gpu_tests_cases_the_unfaulted_restatement_is_inside_the_gate(precision):
    cases = [(R.case(precision, n, m, fam), "points (n, m) = (%d, %d) %s" % (n, m, fam)) for n, m, fam in R.point_cases()]
    cases += [(R.body_case(precision, n, fam), "bodies n = %d %s" % (n, fam)) for n, fam in R.body_cases()]
    for c, what in cases:
        got = R.restate(c["state"], c["points"], precision, bodies=c["bodies"])
        k = R.worst(got, c, precision)
        print("fp%d %-40s: K %.2f of %.1f (K_ref %.2f)" % (precision, what, k, c["gate"], c["kref"]))
        assert k <= c["gate"], (precision, what, k)
        assert c["gate"] == 2 * max(c["kref"], R.FLOOR[precision]) and R.FLOOR[precision] >= F.K_TERM
    one = R.body_case(precision, 1, "cloud")
    assert (R.restate(one["state"], None, precision, bodies=True) == 0).all() and (one["truth"][2] == 0).all()  # n = 1: exact zeros


FAULT_CASES = (
    (("points", 2049, 1025, "box"), (("dropped record", 700, 1500), ("doubled record", 3, 2048), ("last tile of the last split skipped", -1, -1),
                                     ("split partial added twice", -1, 1), ("point index shifted by one", -1, -1),
                                     ("the lane's two points swapped", -1, -1), ("xy and yz exchanged", -1, -1),
                                     ("the factor 3 missing", -1, -1), ("Q not subtracted", -1, -1))),
    (("points", 257, 513, "origin"), (("padding record with mass", -1, -1),)),
    (("bodies", 1025, None, "cloud"), (("the self term kept in bodies mode", -1, -1), ("a neighbour masked instead of self", -1, -1),
                                       ("the lane's two points swapped", -1, -1), ("last tile of the last split skipped", -1, -1))),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_puts_a_point_outside_the_gate(precision):
    planted = set()
    for (mode, n, m, family), faults in FAULT_CASES:
        c = R.case(precision, n, m, family) if mode == "points" else R.body_case(precision, n, family)
        for fault in faults:
            k = R.worst(R.restate(c["state"], c["points"], precision, bodies=c["bodies"], fault=fault), c, precision)
            print("fp%d %s n = %d %-6s %-36s: K %.3g of %.1f" % (precision, mode, n, family, fault[0], k, c["gate"]))
            assert k > c["gate"], (precision, mode, n, family, fault, k)
            planted.add(fault[0])
    assert planted == set(R.FAULTS)


# ---------------------------------------------------------------------------------------------------------------------------
# the header, the symbols, the checks before HIP
# ---------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


PTS = "const void*, const void*, const void*"
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_tidal.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, int32_t, %s, void*[6]) = nbx_tidal; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, int32_t, %s, void*[6]) = nbx_ensemble_tidal; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, int32_t, %s, void*[6]) = nbx_ragged_tidal; '
           'int (*d)(nbx_ctx*, void*[6]) = nbx_tidal_bodies; '
           'int (*e)(nbx_ensemble*, int32_t, int32_t, void*[6]) = nbx_ensemble_tidal_bodies; '
           'int (*f)(nbx_ragged*, int32_t, int32_t, void*[6]) = nbx_ragged_tidal_bodies; '
           'printf("ok\\n"); return (a != NULL && b != NULL && c != NULL && d != NULL && e != NULL && f != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n'
           % (PTS, PTS, PTS))
PARAMS = "const void* x, const void* y, const void* z, void* t[6]"
UNUSED = "(void)x; (void)y; (void)z; (void)t; (void)m;"
STUBS = ('#include "nbx_tidal.h"\n'
         'int nbx_tidal(nbx_ctx* h, int32_t m, %s) { (void)h; %s return 0; }\n'
         'int nbx_ensemble_tidal(nbx_ensemble* h, int32_t f, int32_t n, int32_t m, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_ragged_tidal(nbx_ragged* h, int32_t f, int32_t n, int32_t m, %s) { (void)h; (void)f; (void)n; %s return 0; }\n'
         'int nbx_tidal_bodies(nbx_ctx* h, void* t[6]) { (void)h; (void)t; return 0; }\n'
         'int nbx_ensemble_tidal_bodies(nbx_ensemble* h, int32_t f, int32_t n, void* t[6]) { (void)h; (void)f; (void)n; (void)t; return 0; }\n'
         'int nbx_ragged_tidal_bodies(nbx_ragged* h, int32_t f, int32_t n, void* t[6]) { (void)h; (void)f; (void)n; (void)t; return 0; }\n'
         % (PARAMS, UNUSED, PARAMS, UNUSED, PARAMS, UNUSED))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_against_stubs(tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "tidal_header")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok\n"


def test_declared_set_is_the_six_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_tidal.h")
    assert declared == sorted(ENTRY_POINTS) and tuple(nbx.TIDAL_SYMBOLS) == ENTRY_POINTS
    for h in OTHER_HEADERS + ("nbx_field.h",):
        assert not set(declared) & set(_declared(h)), h
    for h in OTHER_HEADERS:
        assert "nbx_tidal" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
    assert [len(getattr(L, s).argtypes) for s in ENTRY_POINTS] == [6, 8, 8, 2, 4, 4]
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_tidal.h")).read())  # the comment as running text
    for word in ("Why:", "Definition", "Points mode", "Bodies mode", "Two identities", "Per-pair arithmetic", "Error of one term", "Semantics",
                 "Status of points mode, in this order", "Status of bodies mode, in this order", "Deliberately not here", "Unspecified results",
                 "xx, xy, xz, yy, yz, zz", "never formed", "not subtracted afterwards", "delta_ab term only", "-3 eps^2", "no mask is needed",
                 "a NULL array is never written", "t itself must not be NULL", "sliced context", "all n bodies", "nbx_commit", "synchronises once",
                 "steps_done", "graph replay", "the tracers", "2^21", "two partial records", "1 GiB", "32 bits", "before the first HIP call",
                 "NBX_ERR_ALLOC", "fma(h, fma(h, 35, 20), 8)", "2^-65", "2^-24", "30.5 u", "24 u", "groups", "device pointers", "jerk",
                 "variational equation", "hipGraph", "nbody.x", "the same bits", "not finite"):
        assert word in doc, word
    field = re.sub(r"\n \*\s*", " ", open(os.path.join(ROOT, "include", "nbx_field.h")).read())
    not_here = field[field.index("Deliberately not here"):]
    assert "nbx_tidal.h" in not_here and "jerk;" in not_here and "tidal tensors or jerk;" not in not_here  # the list names jerk alone


def _call(nbx, name, handle, first, count, m, p, t):
    f = getattr(nbx.load(), name)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    args = ([m] + [ptr(a) for a in p] if name in POINT_ENTRIES else []) + [t]
    return f(handle, *args) if name in ("nbx_tidal", "nbx_tidal_bodies") else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members and nothing uploaded: it reaches the range
    check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    points = name in POINT_ENTRIES
    batch = "ensemble" in name or "ragged" in name
    pts = [np.full(8, 0.25, dtype=np.float64) for _ in range(3)]
    out = [np.full(8, -7.25, dtype=np.float64) for _ in range(6)]
    t = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in out])
    none6 = (ctypes.c_void_p * 6)()
    none3 = [None] * 3
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # the handle is NULL -- whatever else is wrong
    for m, p, tt in ((4, pts, t), (-1, none3, None)):
        assert _call(nbx, name, None, -1, 5, m, p, tt) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    if points:
        # m < 0 -- before the arrays, t and the range
        assert _call(nbx, name, handle, -1, 5, -1, none3, None) == nbx.NBX_ERR_ARG and err() == name + ": m < 0"
        # m > 0 and a NULL point array -- before t and the range
        for k in range(3):
            p = list(pts)
            p[k] = None
            assert _call(nbx, name, handle, -1, 5, 4, p, None) == nbx.NBX_ERR_ARG and err() == name + ": NULL point array"
    # t is NULL -- before the range, the size and the state
    assert _call(nbx, name, handle, -1, 5, 4, pts, None) == nbx.NBX_ERR_ARG and err() == name + ": t is NULL"
    if batch:
        # the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert _call(nbx, name, handle, first, count, 4, pts, t) == nbx.NBX_ERR_ARG, (first, count)
            assert err() == name + ": members [first, first + count) are outside [0, members)"
        # count == 0 inside the range: NBX_OK, nothing written, no HIP call
        assert _call(nbx, name, handle, 0, 0, 4, pts, t) == nbx.NBX_OK
        assert _call(nbx, name, handle, 0, 0, 0, none3, none6) == nbx.NBX_OK
    else:
        if points:
            # more than 2^21 points -- before the state (the arrays are not read)
            assert _call(nbx, name, handle, 0, 1, (1 << 21) + 1, pts, t) == nbx.NBX_ERR_ARG and err() == "nbx_tidal: m exceeds 2097152"
        # then the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for m, p, tt in ((4, pts, t), (1 << 21, pts, none6), (0, none3, t), (4, pts, none6)):
            assert _call(nbx, name, handle, 0, 1, m, p, tt) == nbx.NBX_ERR_STATE
            assert err() == name + ": nbx_upload has not been called"
    assert all((a == -7.25).all() for a in out) and zeroed.raw == bytes(1 << 16)


def test_python_methods_and_host_helpers(nbx):
    assert list(inspect.signature(nbx.Context.tidal).parameters) == ["self", "px", "py", "pz"]
    assert list(inspect.signature(nbx.Context.tidal_bodies).parameters) == ["self"]
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.tidal).parameters
        assert list(p) == ["self", "px", "py", "pz", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
        p = inspect.signature(cls.tidal_bodies).parameters
        assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
    assert not hasattr(nbx.Group, "tidal") and not hasattr(nbx.Group, "tidal_bodies")  # groups: deliberately not here
    assert nbx.TIDAL_KEYS == ("t_xx", "t_xy", "t_xz", "t_yy", "t_yz", "t_zz") == R.KEYS
    assert not [f for f, _ in nbx.Opts._fields_ if "tidal" in f]  # no new nbx_opts field
    # tidal_matrix: symmetric, (..., 3, 3), fp64; tidal_radius: (gm / lambda_max)^(1/3), inf where nothing stretches
    res = {k: np.arange(6, dtype=np.float32).reshape(2, 3) + 10 * i for i, k in enumerate(nbx.TIDAL_KEYS)}
    M = nbx.tidal_matrix(res)
    assert M.shape == (2, 3, 3, 3) and M.dtype == np.float64 and np.array_equal(M, np.swapaxes(M, -1, -2))
    assert [M[1, 2, a, b] for a, b in R.PAIRS] == [5.0 + 10 * i for i in range(6)]
    point_mass = {k: np.array([v, v]) for k, v in zip(nbx.TIDAL_KEYS, (2.0 / 8, 0, 0, -1.0 / 8, 0, -1.0 / 8))}  # G M = 1 at distance 2
    assert np.allclose(nbx.tidal_radius(point_mass, 2.0), 2.0) and np.allclose(nbx.tidal_radius(point_mass, [2.0, 16.0]), [2.0, 4.0])
    squeezed = {k: np.array([v]) for k, v in zip(nbx.TIDAL_KEYS, (-1.0, 0, 0, -2.0, 0, 0.0))}
    assert np.isinf(nbx.tidal_radius(squeezed, 1.0)).all()


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_tidal\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_tidal\.o: \$\(CSRC\)/nbx_tidal\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    assert rule
    for dep in (KERNELS, "nbx_analysis.hpp", "nbx_field_shape.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp",
                "nbx_batch.hpp", "nbx_object.hpp", "nbx_plan.hpp", "nbx_pair.hpp", "include/nbx_tidal.h", "include/nbx_ensemble.h",
                "include/nbx_ragged.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_tidal.hip", "include/nbx_tidal.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_and_use_the_fields_shape_rule_unchanged():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_tidal.hip":
            assert KERNELS not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_tidal.hip", KERNELS):
            assert "tidal_kernel" not in txt and "tidal_body" not in txt, f
    kern = re.sub(r"//.*", "", open(os.path.join(CSRC, KERNELS)).read())
    src = open(SRC).read()
    assert "atomic" not in kern + re.sub(r"//.*", "", src)
    assert '#include "nbx_field_shape.hpp"' in kern and "field_shape(" in kern and "field_shape(pts, c->n)" in src
    assert "kTidalMaxPoints = kFieldMaxPoints / 2" in kern
    for fn in ("check_range(", "check_uploaded(", "guarded(", "use_device(", "ensure_bytes(", "ragged_member_table<", "ragged_extents(", "read_back("):
        assert fn in src, fn
    shared = open(ANALYSIS).read()  # device_alloc and device_table are reached through ensure_bytes and ragged_member_table
    for fn in ("device_alloc(", "device_table("):
        assert fn in shared and fn not in re.sub(r"//.*", "", src), fn
    # the bodies-mode size bound's words are the shared ones
    assert '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "range_bodies(o, first, count) > kTidalMaxPoints" in src and "range_noun(o)" in src
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    for field in ("tidal_pts", "tidal_part", "tidal_out", "tidal_tab"):
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
    out = tmp_path_factory.mktemp("isa") / "nbx_tidal.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision, bodies mode) of a pair-work kernel, ("finish", precision, None) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)tidal_kernelI([fd])Lb([01])EEE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64, m.group(3) == "1")
    m = re.search(r"^_ZN3nbx\d+tidal_finish_kernelI([fd])EE", name)
    if m:
        return ("finish", 32 if m.group(1) == "f" else 64, None)
    return None


def _pair_loops(body, ins):
    """The innermost loop bodies (label ... backward branch) that hold `ins`."""
    return [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if re.search(r"\b%s" % ins, b)]


def test_every_kind_precision_and_mode_is_compiled_and_the_finish(isa):
    keys = sorted((_key(k) or ("?", k, None) for k in isa), key=str)
    want = [(kind, p, b) for kind in ("context", "ensemble", "ragged") for p in (32, 64) for b in (False, True)] + [("finish", p, None) for p in (32, 64)]
    assert keys == sorted(want, key=str), keys


def test_no_scratch_no_spills_and_one_tile_of_position_records_in_lds(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)", body), name
        kind, precision, _ = _key(name)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
        assert lds == (0 if kind == "finish" else 256 * (16 if precision == 32 else 32)), (name, lds)


def test_the_fp32_loops_hold_the_derived_operations_per_record_and_only_the_masked_ones_compare(isa):
    """Per j record and lane, counted against the 16-byte LDS reads (one per fp32 record, read whole): 20 packed VALU -- 4 adds (3
    differences and Q), 9 fused multiply-adds (r2: 3, S: 6), 7 multiplies (inv^2, the two of s3, s5, the three of d s5) -- and 2
    v_rsq_f32, nothing unpacked.  Points mode has that one loop.  Bodies mode has three: the unmasked one, the same, and the two
    masked tiles of a column, which add one compare and one select per record: 22."""
    for name, (body, desc, meta) in isa.items():
        kind, precision, bodies = _key(name)
        c = lambda ins, text=body: len(re.findall(r"\b%s" % ins, text))
        assert c(r"(?:global|flat|ds|buffer)_atomic") + c(r"ds_(?:add|min|max)_") == 0, name
        assert c("v_sqrt") == 0 and c("v_rcp_f") == 0, name  # (a ragged kernel divides integers for field_shape: v_rcp_iflag may occur)
        if kind == "finish":
            assert c("v_rsq_") == 0 and c("v_fma_f64") >= 3, name  # 3 S - Q on the diagonal: one fma each
            continue
        if precision == 64:
            loops = _pair_loops(body, "v_rsq_f64")
            assert len(loops) == (3 if bodies else 1), (name, len(loops))
            for loop in loops:
                pairs = c("v_rsq_f64", loop)  # one seed per pair; a record serves the lane's two points
                assert pairs >= 2 and c(r"ds_(?:read|load)_b128", loop) >= pairs, name
                assert c("v_fma_f64", loop) + c("v_fmac_f64", loop) == 14 * pairs, name  # r2: 3, h: 1, the polynomials: 4, S: 6
                assert c("v_add_f64", loop) == 4 * pairs, name                            # 3 differences and Q: a plain add
                assert c("v_mul_f64", loop) == 9 * pairs, name                            # y^2, G m y, t3, s3, t3 y^2, s5, d s5: 3
            assert sorted(c("v_cmp_", loop) > 0 for loop in loops) == ([False, True, True] if bodies else [False]), name
            continue
        loops = _pair_loops(body, "v_pk_fma_f32")
        assert len(loops) == (3 if bodies else 1), (name, len(loops))
        extra = []
        for loop in loops:
            records = c(r"ds_(?:read|load)_b128", loop)
            assert records >= 1 and c(r"ds_(?:read|load)_b(?:32|64|96)\b", loop) == 0, (name, records)  # whole records only
            got = (c("v_pk_add_f32", loop), c("v_pk_fma_f32", loop), c("v_pk_mul_f32", loop), c("v_rsq_f32", loop))
            assert got == (4 * records, 9 * records, 7 * records, 2 * records), (name, records, got)
            assert c(r"v_(?:add|sub|mul|fma|fmac)_f32", loop) == 0, name  # nothing unpacked
            assert c("v_cmp_", loop) == c("v_cndmask_b32", loop), name
            extra.append(c("v_cmp_", loop) / records)
        assert sorted(extra) == ([0, 1, 1] if bodies else [0]), (name, extra)  # 20 per record, and 22 in the two masked tiles
