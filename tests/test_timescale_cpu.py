"""Pair approach and free-fall rates (include/nbx_timescale.h), the parts that need no GPU: the header, its struct and its three
exported symbols, the argument checks that come before the first HIP call, the Python methods, suggest_dt and adaptive(), the
build files, an audit of the cross-compiled gfx950 code of nbx_timescale.hip, and the numpy restatement tests/timescale_ref.py,
which must show by itself what the device tests then ask of the library.

The adaptive figures, restatement alone, fp64, the three systems of timescale_ref.ENCOUNTER_SEEDS = (2, 4, 5) to T = 0.5 with
eta = 0.05 and dt_max = 1/16, |E - E0| / |E0| of adaptive() against plain steps of T / steps, the same number of steps:
    each system alone:   478 steps 4.811e-04 vs 3.239e-03 (6.7x);  494 steps 4.858e-04 vs 3.140e-03 (6.5x);
                         486 steps 4.255e-04 vs 3.244e-03 (7.6x)
    the three together (one dt, the smallest any asks for -- what an ensemble does): 610 steps,
                         4.052e-04 vs 2.139e-03 (5.3x);  4.074e-04 vs 2.181e-03 (5.4x);  4.118e-04 vs 2.197e-03 (5.3x)
Of seeds 1 ... 24, all have the adaptive run ahead (3.6x ... 7.6x); the three were taken for their room over 4x.  The error of
the adaptive run is not small because plain steps, read as leapfrog, kick by a(x) dt_k where a changing step would want
a(x) (dt_k-1 + dt_k) / 2: it is about eta times the pair's potential well whatever the step count.  The fixed run loses more
because its step, 1e-3, is more than twice the 4e-4 the two bodies take to pass through each other.
"""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import energy_ref as E
import kick_ref as K
import timescale_ref as R
from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
SRC = os.path.join(CSRC, "nbx_timescale.hip")
OTHER_HEADERS = ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h", "nbx_ragged.h", "nbx_ragged_diag.h", "nbx_batch_accel.h",
                 "nbx_kick.h")
ENTRY_POINTS = ("nbx_timescale", "nbx_ensemble_timescale", "nbx_ragged_timescale")
NOUN = {"nbx_timescale": "ctx", "nbx_ensemble_timescale": "ensemble", "nbx_ragged_timescale": "ragged ensemble"}
STRUCT_FIELDS = ("struct_size", "n", "steps_done", "approach_rate2", "freefall_rate2", "min_r2")


def _declared(header):
    """The functions a header declares itself (comments stripped, #include lines not followed)."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


PROGRAM = ('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_timescale.h"\n'
           'int main(void) { nbx_timescale_t t; '
           'int (*a)(nbx_ctx*, nbx_timescale_t*) = nbx_timescale; '
           'int (*b)(nbx_ensemble*, int32_t, int32_t, nbx_timescale_t*) = nbx_ensemble_timescale; '
           'int (*c)(nbx_ragged*, int32_t, int32_t, nbx_timescale_t*) = nbx_ragged_timescale; '
           'printf("%d", (int)sizeof t); '
           + "".join('printf(" %%d", (int)offsetof(nbx_timescale_t, %s)); ' % f for f in STRUCT_FIELDS) +
           'printf("\\n"); return (a != NULL && b != NULL && c != NULL) ? NBX_ABI_VERSION - 1 : 1; }\n')
STUBS = ('#include "nbx_timescale.h"\n'
         'int nbx_timescale(nbx_ctx* c, nbx_timescale_t* o) { (void)c; (void)o; return 0; }\n'
         'int nbx_ensemble_timescale(nbx_ensemble* e, int32_t f, int32_t n, nbx_timescale_t* o) { (void)e; (void)f; (void)n; (void)o; return 0; }\n'
         'int nbx_ragged_timescale(nbx_ragged* r, int32_t f, int32_t n, nbx_timescale_t* o) { (void)r; (void)f; (void)n; (void)o; return 0; }\n')


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles_as_c99_and_as_cxx_and_the_struct_is_the_ctypes_one(nbx, tmp_path, compiler, std, ext):
    for name, text in (("main", PROGRAM), ("stubs", STUBS)):
        (tmp_path / (name + "." + ext)).write_text(text)
    exe = str(tmp_path / "layout")
    subprocess.check_call([compiler, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / ("main." + ext)), str(tmp_path / ("stubs." + ext)), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert [f for f, _ in nbx.Timescale._fields_] == list(STRUCT_FIELDS)
    assert got == [ctypes.sizeof(nbx.Timescale)] + [getattr(nbx.Timescale, f).offset for f in STRUCT_FIELDS], got
    assert got == [40, 0, 4, 8, 16, 24, 32]
    t = nbx.Timescale()
    t.n, t.steps_done, t.approach_rate2, t.freefall_rate2, t.min_r2 = 5, 7, 1.5, 2.5, math.inf
    assert t.asdict() == {"n": 5, "steps_done": 7, "approach_rate2": 1.5, "freefall_rate2": 2.5, "min_r2": math.inf}


def test_declared_set_is_the_three_symbols_exported_and_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_timescale.h")
    assert declared == sorted(ENTRY_POINTS) and set(declared) == set(nbx.TIMESCALE_SYMBOLS) and len(nbx.TIMESCALE_SYMBOLS) == 3
    for h in OTHER_HEADERS:
        assert not set(declared) & set(_declared(h)), h
        assert "nbx_timescale" not in open(os.path.join(ROOT, "include", h)).read(), h  # the other headers are as they were
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS) |
                                set(nbx.RAGGED_SYMBOLS) | set(nbx.RAGGED_DIAG_SYMBOLS) | set(nbx.BATCH_ACCEL_SYMBOLS) | set(nbx.KICK_SYMBOLS))
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert len(getattr(L, s).argtypes) == (2 if s == "nbx_timescale" else 4)
    assert L.nbx_abi_version() == 1
    assert "#define NBX_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nbx.h")).read()
    doc = open(os.path.join(ROOT, "include", "nbx_timescale.h")).read()
    for word in ("Deliberately not here", "groups and sliced contexts", "indices of the extreme pair", "a value per body", "a dt per member",
                 "nbody.x", "hipGraph", "mul_rn", "add_rn", "rsq", "by a mask", "+infinity", "r2 = eps^2", "the same bits", "NBX_ERR_STATE",
                 "NBX_ERR_ALLOC", "nbx_commit", "before the first HIP call", "count == 0", "synchronises once", "eta / sqrt("):
        assert word in doc, word


def _call(nbx, name, handle, out, first=0, count=1):
    f = getattr(nbx.load(), name)
    return f(handle, out) if name == "nbx_timescale" else f(handle, first, count, out)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_argument_errors_come_before_hip_with_the_entry_point_named_and_out_is_not_written(nbx, name):
    """No device exists here: a status other than the one stated, or another text, would mean a check came after a HIP call.  A
    handle that is merely not NULL -- zeroed memory that is no object -- has no members and nothing uploaded: it reaches the range
    check (a batch kind) or the struct_size and state checks (a context) and nothing behind them."""
    L = nbx.load()
    err = lambda: L.nbx_last_error().decode()
    out = (nbx.Timescale * 3)()
    for k in range(3):
        out[k].struct_size, out[k].n, out[k].min_r2 = ctypes.sizeof(nbx.Timescale), -7, -7.25
    before = bytes(out)
    zeroed = ctypes.create_string_buffer(1 << 16)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    # 1. the handle is NULL -- whatever else is wrong
    for o in (out, None):
        assert _call(nbx, name, None, o, -1, 5) == nbx.NBX_ERR_ARG
        assert err() == "%s: %s is NULL" % (name, NOUN[name])
    # 2. out is NULL
    assert _call(nbx, name, handle, None, -1, 5) == nbx.NBX_ERR_ARG
    assert err() == name + ": out is NULL"
    if name != "nbx_timescale":
        # 3. the range leaves [0, members): the zeroed object has none
        for first, count in ((0, 1), (-1, 1), (0, -1), (1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert _call(nbx, name, handle, out, first, count) == nbx.NBX_ERR_ARG, (first, count)
            assert err() == name + ": members [first, first + count) are outside [0, members)"
        # count == 0 inside the range: NBX_OK, nothing written, no HIP call
        assert _call(nbx, name, handle, out, 0, 0) == nbx.NBX_OK
    else:
        # 4. a wrong struct_size comes before the state
        out[0].struct_size = ctypes.sizeof(nbx.Timescale) - 8
        assert _call(nbx, name, handle, out) == nbx.NBX_ERR_ARG
        assert err() == "nbx_timescale: nbx_timescale_t.struct_size does not match this library"
        out[0].struct_size = ctypes.sizeof(nbx.Timescale)
        # 5. then the state: the zeroed context has not been uploaded -- still no HIP call
        for size in (ctypes.sizeof(nbx.Timescale), 0):
            out[0].struct_size = size
            assert _call(nbx, name, handle, out) == nbx.NBX_ERR_STATE
            assert err() == "nbx_timescale: nbx_upload has not been called"
        out[0].struct_size = ctypes.sizeof(nbx.Timescale)
    assert bytes(out) == before and zeroed.raw == bytes(1 << 16)


def test_python_methods(nbx):
    p = inspect.signature(nbx.Context.timescale).parameters
    assert list(p) == ["self"]
    for cls in (nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.timescale).parameters
        assert list(p) == ["self", "first", "count"] and p["first"].default == 0 and p["count"].default is None, cls
    for cls in (nbx.Context, nbx.Ensemble, nbx.Ragged):
        p = inspect.signature(cls.adaptive).parameters
        assert list(p) == ["self", "t_end", "eta", "dt_max", "max_steps"] and p["max_steps"].default == 100000, cls
        assert all(p[k].default is inspect.Parameter.empty for k in ("t_end", "eta", "dt_max")), cls
        assert cls.adaptive is nbx._Adaptive.adaptive, cls
    assert not hasattr(nbx.Group, "timescale") and not hasattr(nbx.Group, "adaptive")  # groups: deliberately not here
    assert list(inspect.signature(nbx.suggest_dt).parameters) == ["ts", "eta"]
    assert not [f for f, _ in nbx.Opts._fields_ if "time" in f or "adapt" in f or "eta" in f]  # no new nbx_opts field


def test_suggest_dt(nbx):
    ts = lambda a, f: {"approach_rate2": a, "freefall_rate2": f, "min_r2": 1.0, "n": 2, "steps_done": 0}
    for fn in (nbx.suggest_dt, R.suggest_dt):
        assert fn(ts(4.0, 1.0), 0.5) == 0.25 and fn(ts(1.0, 16.0), 0.5) == 0.125  # the larger of the two rates
        assert fn([ts(4.0, 1.0), ts(1.0, 64.0), ts(0.0, 0.0)], 1.0) == 0.125       # the largest rate of all entries
        assert fn(ts(0.0, 0.0), 0.05) == math.inf and fn([ts(0.0, 0.0)] * 3, 0.05) == math.inf and fn([], 0.05) == math.inf
        assert fn(ts(0.0, 100.0), 0.02) == 0.02 / math.sqrt(100.0)


def test_adaptive_takes_the_smallest_of_the_three_bounds_and_lands_on_t_end(nbx):
    calls = []

    class Fake(nbx._Adaptive):
        def __init__(self, rates):
            self.rates = list(rates)

        def timescale(self):
            calls.append("timescale")
            r = self.rates.pop(0)
            return [{"approach_rate2": r, "freefall_rate2": 0.0}, {"approach_rate2": 0.0, "freefall_rate2": r / 4}]  # a batch object's list

        def step(self, nsteps, dt, kenergy=True):
            calls.append(("step", nsteps, dt, kenergy))

    # eta = 0.5: rate 0 -> inf (dt_max binds), rate 16 -> 0.125 (the rate binds), rate 1 -> 0.5 (t_end - t binds: 1.0 - 0.75 - 0.125)
    t, steps, dts = Fake([0.0, 16.0, 1.0]).adaptive(1.0, 0.5, 0.75)
    assert (t, steps, dts) == (1.0, 3, [0.75, 0.125, 0.125])
    assert calls == ["timescale", ("step", 1, 0.75, False), "timescale", ("step", 1, 0.125, False), "timescale", ("step", 1, 0.125, False)]
    # thirds do not add up to 1.0 in binary: the last step is what is left, and t is t_end itself
    t, steps, dts = Fake([0.0] * 4).adaptive(1.0, 0.5, 1.0 / 3)
    assert t == 1.0 and steps == len(dts) and dts[:2] == [1.0 / 3] * 2 and all(d > 0 for d in dts) and steps in (3, 4)
    t, steps, dts = Fake([25.0] * 12).adaptive(1.0, 0.5, 1.0)
    assert t == 1.0 and steps == len(dts) in (10, 11) and dts[:9] == [0.1] * 9 and abs(sum(dts) - 1.0) < 1e-15
    with pytest.raises(RuntimeError, match="max_steps = 4"):
        Fake([25.0] * 10).adaptive(1.0, 0.5, 1.0, max_steps=4)
    assert Fake([]).adaptive(0.0, 0.5, 1.0) == (0.0, 0, [])  # nothing to do: no call at all


def test_the_build_files_compile_and_link_the_translation_unit():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(PKG\)/libnbx\.so:.*\$\(PKG\)/nbx_timescale\.o", mk, re.M)
    rule = re.search(r"^\$\(PKG\)/nbx_timescale\.o: \$\(CSRC\)/nbx_timescale\.hip(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c \$< -o \$@$", mk, re.M)
    assert rule
    for dep in ("nbx_timescale_kernels.hpp", "nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_internal.hpp", "nbx_batch.hpp",
                "nbx_object.hpp", "nbx_plan.hpp", "nbx_diag_shape.hpp", "nbx_pair.hpp", "include/nbx_timescale.h", "include/nbx_ensemble.h",
                "include/nbx_ragged.h"):
        assert dep in rule.group(1), dep
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    for word in ("-c nbx_timescale.hip", "include/nbx_timescale.h"):
        assert word in sh, word


def test_the_kernels_live_in_their_own_translation_unit_and_use_the_shared_shape_rule():
    for f in sorted(os.listdir(CSRC)):
        txt = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        if f != "nbx_timescale.hip":
            assert "nbx_timescale_kernels.hpp" not in txt, f  # nobody else includes the kernels
        if f not in ("nbx_timescale.hip", "nbx_timescale_kernels.hpp"):
            assert "timescale_kernel" not in txt, f
    src = open(SRC).read()
    assert src.count("diag_splits(") == 2 and "plan_ragged_diag(" in src  # a context, an ensemble member; a ragged member's work list
    assert "atomic" not in re.sub(r"//.*", "", src + open(os.path.join(CSRC, "nbx_timescale_kernels.hpp")).read())


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
    out = tmp_path_factory.mktemp("isa") / "nbx_timescale.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", SRC, "-o", str(out)])
    txt = open(out).read()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"  - \.agpr_count:.*?\.symbol:\s+(\S+)\.kd\n.*?\.wavefront_size:\s+\d+\n", txt, re.S)}
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3), meta[m.group(1)])
    return ks


def _key(name):
    """(kind, precision) of a pair-work kernel, (kind, 0) of a reduce kernel."""
    m = re.search(r"^_ZN3nbx\d+(ensemble_|ragged_|)timescale_kernelI([fd])EE", name)
    if m:
        return (m.group(1).rstrip("_") or "context", 32 if m.group(2) == "f" else 64)
    m = re.search(r"^_ZN3nbx\d+(ragged_|)timescale_reduce_kernelE", name)
    if m:
        return ("ragged reduce" if m.group(1) else "reduce", 0)
    return None


def test_the_kernels_are_the_pair_work_of_three_kinds_in_two_precisions_and_two_reduces(isa):
    keys = sorted(_key(k) or ("?", k) for k in isa)
    assert keys == sorted([(kind, p) for kind in ("context", "ensemble", "ragged") for p in (32, 64)] + [("reduce", 0), ("ragged reduce", 0)]), keys


def test_no_scratch_no_spills_no_atomics_and_one_row_of_three_doubles_per_workgroup(isa):
    for name, (body, desc, meta) in isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert re.search(r"\.private_segment_fixed_size:\s+0\n", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\n", meta) and re.search(r"\.vgpr_spill_count:\s+0\n", meta), name
        assert re.findall(r"\b((?:global|flat|buffer)_(?:store|atomic)\w*)", body) == ["global_store_dwordx2"], name  # lanes 0, 1, 2: one double each


def test_the_fp32_pair_loop_is_packed_reads_lds_records_whole_and_takes_the_raw_reciprocal_square_root(isa):
    for name, (body, desc, meta) in isa.items():
        kind, precision = _key(name)
        if precision == 32:
            for ins in ("v_rsq_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_max3_f32|v_max_f32", "v_min3_f32|v_min_f32"):
                assert re.search(r"\b(?:%s)" % ins, body), (name, ins)
            assert re.search(r"\bds_(?:read|load)_b128", body), name
            assert not re.search(r"\bv_sqrt|\bv_div_", body), name  # the raw v_rsq_f32, not an expanded 1 / sqrt
            lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)\n", meta).group(1))
            assert lds == 2 * 256 * 16 + 3 * 4 * 8, (name, lds)  # the two tiles and the workgroup's reduction
        if precision == 64:
            assert re.search(r"\bv_rsq_f64", body) and re.search(r"\bv_fma_f64", body), name


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement on its own
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_bodies_give_the_closed_forms_and_one_body_has_no_pair(dtype):
    d, m1, m2 = 0.75, 3.0e9, 5.0e9
    s = {"pos_x": [1.0, 1.0], "pos_y": [2.0, 2.0 + d], "pos_z": [-1.0, -1.0], "vel_x": [0.5, -0.25], "vel_y": [0.0, 1.0], "vel_z": [2.0, 2.0],
         "mass": [m1, m2]}
    s = {k: np.array(v, dtype=dtype) for k, v in s.items()}
    t = R.timescale(s)
    r2 = d * d + E.EPS2
    G = float(E.G32)
    assert t["n"] == 2 and t["min_r2"] == r2
    assert abs(t["approach_rate2"] - (0.75 ** 2 + 1.0) / r2) <= 1e-15 * t["approach_rate2"]
    assert abs(t["freefall_rate2"] - G * (m1 + m2) / r2 ** 1.5) <= (1e-6 if dtype == np.float32 else 1e-15) * t["freefall_rate2"]
    assert {k: t[k] for k in R.KEYS} == R.pair_values(s, 0, 1) == R.pair_values(s, 1, 0)
    # two DISTINCT bodies at one position are a pair, with r2 = eps^2
    s["pos_y"][1] = s["pos_y"][0]
    assert R.timescale(s)["min_r2"] == E.EPS2
    one = {k: v[:1] for k, v in s.items()}
    assert R.timescale(one) == {"approach_rate2": 0.0, "freefall_rate2": 0.0, "min_r2": math.inf, "n": 1}
    assert R.suggest_dt(R.timescale(one), 0.05) == math.inf


def test_a_planted_pair_is_extreme_by_a_factor_of_ten_in_all_three_values():
    for n, (i, j) in ((257, (255, 256)), (2049, (1279, 1280)), (4097, (4096, 0))):
        s = R.plant_pair(R.spread_state(11, n), i, j)
        t, pair = R.timescale(s), R.pair_values(s, i, j)
        back = R.timescale(s, exclude=((i, j), (j, i)))
        assert {k: t[k] for k in R.KEYS} == pair
        assert pair["approach_rate2"] >= 10 * back["approach_rate2"] and pair["freefall_rate2"] >= 10 * back["freefall_rate2"], (n, pair, back)
        assert 10 * pair["min_r2"] <= back["min_r2"], (n, pair, back)


@pytest.fixture(scope="module")
def encounters():
    """The three systems of ENCOUNTER_SEEDS advanced to T adaptively and with the same number of equal steps: alone and together."""
    out = {}
    start = [R.encounter_state(seed) for seed in R.ENCOUNTER_SEEDS]
    for name, groups in (("alone", [[0], [1], [2]]), ("together", [[0, 1, 2]])):
        rows = []
        for g in groups:
            s0 = [start[k] for k in g]
            a = [K.copy(s) for s in s0]
            t, steps, dts = R.adaptive(a, R.ENCOUNTER_T, R.ENCOUNTER_ETA, R.ENCOUNTER_DT_MAX)
            f = [K.copy(s) for s in s0]
            for s in f:
                K.step(s, steps, R.ENCOUNTER_T / steps)
            for k, ea, ef in zip(g, R.energy_errors(s0, a), R.energy_errors(s0, f)):
                rows.append((R.ENCOUNTER_SEEDS[k], t, steps, min(dts), max(dts), ea, ef))
        out[name] = rows
    return out


def test_the_encounter_systems_are_what_the_docstring_describes():
    for seed in R.ENCOUNTER_SEEDS:
        s, plain = R.encounter_state(seed), K.make_state(seed)
        assert len(s["mass"]) == 96 and s["mass"][0] == s["mass"][1] == 40.0 * plain["mass"].max()
        assert all((s[k][2:] == plain[k][2:]).all() for k in K.FIELDS)
        assert s["pos_x"][1] - s["pos_x"][0] == 20.0 and s["vel_x"][0] - s["vel_x"][1] == 80.0  # they meet at T / 2
        t, pair = R.timescale(s), R.pair_values(s, 0, 1)
        assert pair["approach_rate2"] == 6400.0 / (400.0 + E.EPS2) and pair["min_r2"] == 400.0 + E.EPS2
        assert t["approach_rate2"] > pair["approach_rate2"]  # at the start the background sets the step; the pair takes over as it closes


@pytest.mark.parametrize("how", ["alone", "together"])
def test_adaptive_steps_beat_equal_steps_of_the_same_number_by_four(encounters, how):
    for seed, t, steps, dt_min, dt_max, ea, ef in encounters[how]:
        print("seed %d %s: t = %r, %d steps of %.3e ... %.3e (fixed: %.3e): adaptive %.3e, fixed %.3e, %.2fx"
              % (seed, how, t, steps, dt_min, dt_max, R.ENCOUNTER_T / steps, ea, ef, ef / ea))
        assert t == R.ENCOUNTER_T and dt_max <= R.ENCOUNTER_DT_MAX
        assert dt_min < 0.05 * R.ENCOUNTER_T / steps  # the encounter is what the steps are spent on
        assert ef >= 4.0 * ea, (seed, how, ea, ef)
        assert 4.0e-4 <= ea <= 5.0e-4 and 2.1e-3 <= ef <= 3.3e-3, (seed, how, ea, ef)  # the figures of the docstring
    assert [r[2] for r in encounters[how]] == ([478, 494, 486] if how == "alone" else [610] * 3)
