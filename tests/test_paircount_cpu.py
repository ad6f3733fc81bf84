"""Pairs within each of a list of radii (include/nbx_paircount.h), the parts that need no GPU: the numpy reference
tests/paircount_ref.py, which must show by itself what the device tests then ask of the library; shell_counts; the header and
its three exported symbols; the NULL handle; and an audit of the cross-compiled gfx950 code of nbx_paircount.hip.

The ambiguity caps.  The device tests ask lo <= got <= hi of paircount_ref.bracket (the 8 u window of neighbours_ref).  That
asks something only where the window is narrow, so the reference alone is held to: on every fp32 test state hi - lo <= 8 at
every radius and hi == lo at no fewer than 8 of the 20 radii; on every fp64 test state hi == lo at all of them.  (Seen: the
largest hi - lo is 5, at fp32 box and shifted 4097; 10 of 20 are exact on the worst state; fp64 is exact throughout.)

Which state catches which planted fault: FAULT_CASES."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import paircount_ref as P
from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_paircount.hip")
ANALYSIS = os.path.join(CSRC, "nbx_analysis.hpp")  # the host layer the analysis calls share
ENTRY_POINTS = ("nbx_paircount", "nbx_ensemble_paircount", "nbx_ragged_paircount")
NOUN = {"nbx_paircount": "ctx", "nbx_ensemble_paircount": "ensemble", "nbx_ragged_paircount": "ragged ensemble"}

_r2 = {}


def r2_of(precision, family, n):
    """(state, its sorted pair r2), computed once."""
    key = (precision, family, n)
    if key not in _r2:
        st = P.lattice(n, precision) if family == "lattice" else getattr(P, family)(n, precision)
        r2 = P.pair_r2(st)
        r2.setflags(write=False)
        _r2[key] = (st, r2)
    return _r2[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy reference on its own
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_the_restatement_is_the_plain_count_and_the_passes_are_sixteen_then_the_rest(precision):
    assert len(P.RADII) == 20 and P.RADII == sorted(P.RADII)
    assert P.pass_slots(20) == [(0, 16, 16), (16, 4, 4)]
    assert [P.pass_slots(k)[-1] for k in (1, 4, 5, 8, 9, 16, 17)] == [(0, 1, 4), (0, 4, 4), (0, 5, 8), (0, 8, 8), (0, 9, 16), (0, 16, 16), (16, 1, 4)]
    for family, n in (("box", 257), ("shifted", 257), ("box", 2049), ("shifted", 2049), ("member", 1), ("member", 2), ("member", 513)):
        st, r2 = r2_of(precision, family, n)
        want = P.counts(st, P.RADII, precision, r2)
        assert want.dtype == np.uint64 and want.shape == (20,) and (np.diff(want.astype(np.int64)) >= 0).all()
        assert np.array_equal(P.restate(st, P.RADII, precision), want), (family, n)
        assert P.counts(st, [np.inf], precision, r2).tolist() == [n * (n - 1) // 2] and P.counts(st, [0.0], precision, r2).tolist() == [0]
        for k in (1, 5, 17):  # every E and the seam
            assert np.array_equal(P.restate(st, P.RADII[:k], precision), want[:k]), (family, n, k)
    st, r2 = r2_of(precision, "box", 257)
    order = [7, 0, 19, 7, 3]  # unsorted and repeated
    assert np.array_equal(P.restate(st, [P.RADII[k] for k in order], precision), P.counts(st, P.RADII, precision, r2)[order])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_ambiguity_caps_hold_on_every_state_of_the_device_tests(precision):
    states = [(f, n) for f in ("box", "shifted") for n in P.SIZES] + [("reversed_box", 257), ("reversed_box", 2049)] + \
             [("member", n) for n in P.RAGGED_SIZES]
    for family, n in states:
        st, r2 = r2_of(precision, family, n)
        lo, hi = P.bracket(st, P.RADII, precision, r2)
        plain = P.counts(st, P.RADII, precision, r2)
        assert (lo <= plain).all() and (plain <= hi).all()
        width = (hi - lo).astype(np.int64)
        print("fp%d %s(%d): largest hi - lo %d, exact at %d of 20 radii, counts %d ... %d" % (precision, family, n, width.max(), (width == 0).sum(),
                                                                                             plain[0], plain[-1]))
        if precision == 64:
            assert (width == 0).all(), (family, n)
        else:
            assert width.max() <= 8 and (width == 0).sum() >= 8, (family, n, width.tolist())
    # the radii span the system: nothing to count below the first at 257 bodies, every pair within the last
    st, r2 = r2_of(precision, "box", 4097)
    plain = P.counts(st, P.RADII, precision, r2)
    assert 0 < plain[0] < plain[10] < plain[19] < 4097 * 4096 // 2 and len(set(plain.tolist())) == 20
    assert P.counts(r2_of(precision, "shifted", 4097)[0], [3.5], precision).tolist() == [4097 * 4096 // 2]


FAULT_CASES = (
    (("box", 257), P.RADII[:17], ("self counted", "padding record counted", "not halved", "last tile of the last split skipped",
                                  "second pass reuses the first pass's radii", "unused slot counted")),
    (("box", 2049), P.RADII, ("last tile of the last split skipped", "last column dropped by the finish", "second pass reuses the first pass's radii",
                              "padding record counted")),
    (("lattice", P.LATTICE_K), [P.LATTICE_TIE_RADIUS], ("< instead of <=", "self counted", "unused slot counted")),
)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_planted_fault_changes_the_counts_of_some_test_state(precision):
    planted = set()
    for (family, n), radii, faults in FAULT_CASES:
        st, r2 = r2_of(precision, family, n)
        want = P.counts(st, radii, precision, r2)
        lo, hi = P.bracket(st, radii, precision, r2)
        assert np.array_equal(P.restate(st, radii, precision), want)
        for fault in faults:
            got = P.restate(st, radii, precision, fault=fault)
            # what the device tests see: the bracket, and on the lattice -- exact in T, h2 a tie -- the count from the geometry
            outside = (got != want) if family == "lattice" else (got < lo) | (got > hi)
            print("fp%d %s(%d), %d radii, %-42s: %d counts differ, %d leave the bracket" % (precision, family, n, len(radii), fault, (got != want).sum(),
                                                                                          outside.sum()))
            assert outside.any(), (precision, family, n, fault)
            planted.add(fault)
    assert planted == set(P.FAULTS)
    # what some faults are seen by
    st, r2 = r2_of(precision, "box", 257)
    want = P.counts(st, P.RADII, precision, r2)
    assert np.array_equal(P.restate(st, P.RADII, precision, fault="not halved"), 2 * want)
    assert (P.restate(st, P.RADII, precision, fault="self counted") - want == 128).all()  # 257 bodies themselves, halved
    assert np.array_equal(P.restate(st, P.RADII, precision, fault="unused slot counted"), want)  # twenty radii leave no slot unused
    assert np.array_equal(P.restate(st, P.RADII, precision, fault="< instead of <="), want)  # no tie in the box: the lattice is needed


@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_counts_follow_from_integer_geometry(precision):
    k = P.LATTICE_K
    st, r2 = r2_of(precision, "lattice", k)
    want = P.lattice_counts(k, 6)
    assert want.tolist() == [6084, 17316, 24228, 29805, 50397, 69405] and P.lattice_face_pairs(k) == 6084
    for f in (lambda radii: P.counts(st, radii, precision, r2), lambda radii: P.restate(st, radii, precision)):
        assert np.array_equal(f(P.LATTICE_RADII), want)
        assert f([P.LATTICE_TIE_RADIUS]).tolist() == [P.lattice_face_pairs(k)]  # <= at the exact tie
    lo, hi = P.bracket(st, P.LATTICE_RADII, precision, r2)
    assert np.array_equal(lo, want) and np.array_equal(hi, want)  # the radii lie between the shells
    assert P.lattice_counts(2, 3).tolist() == [12, 24, 28] and P.lattice_counts(3, 12)[-1] == 27 * 26 // 2


def test_shell_counts_is_the_histogram(nbx):
    c = np.array([0, 3, 3, 10, 4000000000000], dtype=np.uint64)
    got = nbx.shell_counts(c)
    assert got.dtype == np.uint64 and got.tolist() == [0, 3, 0, 7, 3999999999990]
    two = nbx.shell_counts(np.array([[1, 4, 9], [0, 0, 5]], dtype=np.uint64))
    assert two.shape == (2, 3) and two.tolist() == [[1, 3, 5], [0, 0, 5]]
    assert nbx.shell_counts(np.zeros((3, 0), dtype=np.uint64)).shape == (3, 0)
    st, r2 = r2_of(32, "box", 257)
    plain = P.counts(st, P.RADII, 32, r2)
    h2 = [P.h2_of(r, 32) for r in P.RADII]
    hist = [int(((r2 > a) & (r2 <= b)).sum()) for a, b in zip([-1.0] + h2[:-1], h2)]
    assert nbx.shell_counts(plain).tolist() == hist and int(nbx.shell_counts(plain).sum()) == int(plain[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# the header, the symbols, the checks that come before any device
# ---------------------------------------------------------------------------------------------------------------------------
PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_paircount.h"\n'
           'int main(void) { '
           'int (*a)(nbx_ctx*, int32_t, const double*, uint64_t*) = nbx_paircount; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, int32_t, const double*, uint64_t*) = nbx_ensemble_paircount; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, int32_t, const double*, uint64_t*) = nbx_ragged_paircount; '
           'printf("ok %d\\n", NBX_PAIRCOUNT_MAX_RADII); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')
STUBS = ('#include "nbx_paircount.h"\n'
         'int nbx_paircount(nbx_ctx* h, int32_t k, const double* r, uint64_t* c) { (void)h; (void)k; (void)r; (void)c; return 0; }\n'
         'int nbx_ensemble_paircount(nbx_ensemble* h, int32_t f, int32_t n, int32_t k, const double* r, uint64_t* c) '
         '{ (void)h; (void)f; (void)n; (void)k; (void)r; (void)c; return 0; }\n'
         'int nbx_ragged_paircount(nbx_ragged* h, int32_t f, int32_t n, int32_t k, const double* r, uint64_t* c) '
         '{ (void)h; (void)f; (void)n; (void)k; (void)r; (void)c; return 0; }\n')


def test_header_compiles_as_c99_against_stubs(tmp_path):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + ".c")).write_text(text)
    exe = str(tmp_path / "paircount_header")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "main.c"),
                           str(tmp_path / "stubs.c"), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == "ok 256\n"


def test_the_three_symbols_are_exported_and_kept_apart(nbx):
    assert tuple(nbx.PAIRCOUNT_SYMBOLS) == ENTRY_POINTS and nbx.PAIRCOUNT_MAX_RADII == 256
    assert not set(ENTRY_POINTS) & (set(nbx.SYMBOLS) | set(nbx.NEIGHBOUR_SYMBOLS) | set(nbx.FIELD_SYMBOLS) | set(nbx.TIMESCALE_SYMBOLS))
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in ENTRY_POINTS:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (4 if s == "nbx_paircount" else 6)
    assert L.nbx_abi_version() == 1
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged):
        assert callable(cls.paircount)
    assert not hasattr(nbx.Group, "paircount")  # groups: deliberately not here


def _call(nbx, name, handle, nradii, radii, counts, first=0, count=1):
    f = getattr(nbx.load(), name)
    args = [nradii, None if radii is None else radii.ctypes.data_as(ctypes.c_void_p), None if counts is None else counts.ctypes.data_as(ctypes.c_void_p)]
    return f(handle, *args) if name == "nbx_paircount" else f(handle, first, count, *args)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_in_the_stated_order_and_nothing_is_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members, no bodies and nothing uploaded: it reaches
    the range check (a batch kind) or the state check (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    radii = np.array(P.RADII, dtype=np.float64)
    out = np.full(32, 7, dtype=np.uint64)
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for nradii, r, o in ((20, radii, out), (0, None, None), (300, radii, out)):
        assert _call(nbx, name, None, nradii, r, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. nradii outside [1, 256], or radii NULL -- before the radii are looked at and before the range
    for nradii, r in ((0, radii), (-1, radii), (257, radii), (2 ** 31 - 1, radii), (20, None)):
        assert _call(nbx, name, handle, nradii, r, out, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == name + ": nradii is outside [1, 256] or radii is NULL"
    # 3. a radius that is NaN or negative: the first such k is named
    for bad, value in ((0, -1.0), (3, float("nan")), (19, -1e-300), (7, float("-inf"))):
        r = radii.copy()
        r[bad] = value
        r[19] = -2.0 if bad != 19 else r[19]
        for o in (out, None):
            assert _call(nbx, name, handle, 20, r, o, -1, 5) == nbx.NBX_ERR_ARG
            assert err() == "%s: radii[%d] is NaN or negative" % (name, bad)
    if name != "nbx_paircount":
        # 4. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert _call(nbx, name, handle, 20, radii, out, first, count) == nbx.NBX_ERR_ARG, (first, count)
            assert err() == name + ": members [first, first + count) are outside [0, members)"
        # 7. count == 0 inside the range: NBX_OK, nothing written, no HIP call -- with counts and without
        assert _call(nbx, name, handle, 20, radii, out, 0, 0) == nbx.NBX_OK
        assert _call(nbx, name, handle, 1, np.array([np.inf]), None, 0, 0) == nbx.NBX_OK
    else:
        # 6. the state: the zeroed context has not been uploaded -- also where nothing would be launched
        for o in (out, None):
            assert _call(nbx, name, handle, 20, radii, o) == nbx.NBX_ERR_STATE
            assert err() == "nbx_paircount: nbx_upload has not been called"
    assert (out == 7).all() and zeroed.raw == bytes(1 << 16)


def test_the_size_bound_and_the_order_of_the_checks_are_in_the_source():
    """More than 2^22 bodies in one call cannot be made here without a device: the check and its texts are read off the source."""
    src = re.sub(r"//.*", "", open(SRC).read())
    hdr = re.sub(r"//.*", "", open(os.path.join(CSRC, "nbx_paircount_kernels.hpp")).read())
    assert "constexpr long long kPcMaxBodies = kFieldMaxPoints;" in hdr and "atomic" not in src + hdr
    shared = re.sub(r"//.*", "", open(ANALYSIS).read())  # range_bodies and range_noun: one definition for every call
    assert '"nbx_paircount: n exceeds 4194304"' in src and '"count * n exceeds"' in shared and '"the bodies of the range exceed"' in shared
    assert "(long long)c->n > kPcMaxBodies" in src and "range_bodies(o, first, count) > kPcMaxBodies" in src and "range_noun(o)" in src
    batch = src[src.index("int batch_paircount("):]
    order = [batch.index(w) for w in ("is NULL", "check_radii(", "check_range(", "kPcMaxBodies", "check_uploaded(", "!counts", "use_device(")]
    assert order == sorted(order)
    ctx = src[src.index("int nbx_paircount("):]
    order = [ctx.index(w) for w in ("is NULL", "check_radii(", "kPcMaxBodies", "->uploaded", "pending_commit", "!counts", "use_device(")]
    assert order == sorted(order)
    doc = open(os.path.join(ROOT, "include", "nbx_paircount.h")).read()
    for word in ("2^22", "2^31", "by a mask", "member-major", "synchronises once", "no atomics", "before the first HIP call", "triangular half",
                 "Deliberately not here", "i < j < n", "h2_k      = fma(rT, rT, eps2)"):
        assert word in doc, word
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_paircount\.o", mk, re.M)
    assert re.search(r"^\$\(PKG\)/nbx_paircount\.o: \$\(CSRC\)/nbx_paircount\.hip .*nbx_paircount_kernels\.hpp.*include/nbx_paircount\.h\n"
                     r"\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the translation unit
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
    out = tmp_path_factory.mktemp("isa") / "nbx_paircount.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision, E, scheme) of a pair-work kernel, ("finish",) of the finish."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)paircount_kernelI([fd])Li(\d+)ELb([01])EEE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64, int(m.group(3)), "wave" if m.group(4) == "1" else "lane")
    return ("finish",) if re.search(r"^_ZN3nbx\d+paircount_finish_kernelE", name) else None


def test_every_instance_is_there_and_no_kernel_uses_scratch(isa):
    keys = sorted((_key(k) or ("?", k) for k in isa), key=str)
    want = [(kind, p, e, s) for kind in ("context", "ensemble", "ragged") for p in (32, 64) for e in (4, 8, 16) for s in ("lane", "wave")] + [("finish",)]
    assert keys == sorted(want, key=str), keys
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert "scratch_" not in body and "buffer_store" not in body and "atomic" not in body, name


def test_the_fp32_pair_loops_are_packed_and_the_wave_scheme_counts_on_the_scalar_unit(isa):
    """Per j record and lane: one whole 16-byte LDS read, 3 packed subtracts and 3 packed fma for the two pairs, 2 E compares.
    Lane counters add with carry on the vector unit; wave counters take the compare's lane mask through the scalar bit count."""
    for name, (body, desc, meta) in isa.items():
        key = _key(name)
        if key == ("finish",) or key[1] == 64:
            continue
        _, _, E, scheme = key
        loops = [b for b in re.findall(r"\.LBB\d+_\d+:[^\n]*\n((?:(?!\.LBB\d+_\d+:).)*?)s_cbranch_\w+ \.LBB", body, re.S) if "v_pk_fma_f32" in b]
        assert len(loops) == 2, (name, len(loops))  # the masked tile loop and the one without the mask
        for loop in loops:
            c = lambda ins: len(re.findall(r"\b%s" % ins, loop))
            records = c(r"ds_(?:read|load)_b128")
            assert records >= 1 and c("v_pk_fma_f32") == 3 * records and c("v_pk_add_f32") == 3 * records, (name, records)
            assert c("v_cmp_[a-z]+_f32") == 2 * E * records, (name, c("v_cmp_[a-z]+_f32"), records)
            assert c("v_rsq_f32") == 0 and c("v_mul_f32") == 0 and c("v_sqrt") == 0, name
            if scheme == "wave":
                assert c("s_bcnt1_i32_b64") == 2 * E * records, (name, c("s_bcnt1_i32_b64"))
            else:
                assert c("s_bcnt1_i32_b64") == 0 and c("v_addc_co_u32") + c("v_add3_u32") + c("v_add_u32") + c("v_add_co_u32") >= E * records, name
