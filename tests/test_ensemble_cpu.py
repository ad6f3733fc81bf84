"""Ensembles (include/nbx_ensemble.h), the parts that need no GPU: the header and the exported symbols, the argument checks of
nbx_ensemble_create (all of which run before the first HIP call), the host-only planner plan_ensemble through a g++ driver,
and an audit of the cross-compiled gfx950 code of nbx_ensemble.hip.

The audit does not look for the scalar-store family of instructions: the generated ISA of the eleven kernels was read by eye
for them when the kernels were written (there are none: every result leaves through global_store / ds_write)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG, has_gpu

CSRC = os.path.join(PKG, "csrc")
ENSEMBLE_SRC = os.path.join(CSRC, "nbx_ensemble.hip")
DRIVER = os.path.join(ROOT, "tests", "ensemble_plan_driver.cpp")
LOOP_CXX, LOOP_ASM = 0, 1  # nbx_plan.hpp's internal LOOP_*


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


def test_ensemble_symbols_are_exported_and_kept_apart_from_nbx_h(nbx):
    declared = _declared("nbx_ensemble.h")
    assert len(declared) == 9 and set(declared) == set(nbx.ENSEMBLE_SYMBOLS)
    assert not set(declared) & (set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS))
    assert not set(declared) & set(_declared("nbx.h"))  # nbx.h's own symbol set is untouched
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert getattr(L, s) is not None


def test_ensemble_header_compiles_as_c99_and_matches_the_ctypes_mirror(nbx, tmp_path):
    src = tmp_path / "ens.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_ensemble.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(nbx_ensemble_stats_t), offsetof(nbx_ensemble_stats_t, members), '
                   'offsetof(nbx_ensemble_stats_t, cu_count), offsetof(nbx_ensemble_stats_t, steps_done), '
                   'offsetof(nbx_ensemble_stats_t, step_ms_total)); return NBX_ABI_VERSION - 1; }\n')
    exe = str(tmp_path / "ens.x")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    S = nbx.EnsembleStats
    assert got == [ctypes.sizeof(S), S.members.offset, S.cu_count.offset, S.steps_done.offset, S.step_ms_total.offset]


def _create(nbx, n, precision, members, **opts):
    L = nbx.load()
    h = ctypes.c_void_p()
    o = nbx.Opts()
    o.struct_size = ctypes.sizeof(nbx.Opts)
    o.device = -1
    for k, v in opts.items():
        setattr(o, k, v)
    rc = L.nbx_ensemble_create(ctypes.byref(h), n, precision, members, ctypes.byref(o))
    text = L.nbx_last_error().decode()
    if h.value:
        L.nbx_ensemble_destroy(h)
    return rc, text


BAD_ARGS = [
    (0, 32, 4, {}, "n must"), (16384, 32, 4, {}, "nbx_create"), (12289, 64, 4, {}, "nbx_create"),
    (1000, 32, 0, {}, "members"), (1000, 32, 65536, {}, "members"), (1000, 16, 4, {}, "precision"),
    (1000, 32, 4, {"kernel_variant": 2}, "kernel_variant"),      # NBX_KERNEL_SGPR
    (1000, 32, 4, {"summation_order": 1}, "summation_order"),    # NBX_ORDER_REFERENCE
    (1000, 32, 4, {"j_split": 2}, "j_split"),
    (1000, 64, 4, {"bodies_per_lane": 16}, "bodies_per_lane"),
    # beyond the issue's list: the other fields an ensemble cannot honour
    (1000, 32, 4, {"i_begin": 1}, "i_begin"), (1000, 32, 4, {"i_count": 10}, "i_count"), (1000, 32, 4, {"external_stream": 1}, "external_stream"),
    (1000, 32, 4, {"bodies_per_lane": 3}, "bodies_per_lane"), (1000, 32, 4, {"inner_loop": 3}, "inner_loop"),
    (1000, 64, 4, {"inner_loop": 2}, "hand-scheduled"), (1000, 32, 4, {"bodies_per_lane": 16, "inner_loop": 2}, "hand-scheduled"),
]


@pytest.mark.parametrize("n,precision,members,opts,word", BAD_ARGS)
def test_create_rejects_bad_arguments_before_any_device_call(nbx, n, precision, members, opts, word):
    rc, text = _create(nbx, n, precision, members, **opts)
    assert rc == nbx.NBX_ERR_ARG, (rc, text)
    assert text and word in text, text


def test_null_arguments(nbx):
    L = nbx.load()
    null = ctypes.c_void_p()
    assert L.nbx_ensemble_create(None, 100, 32, 4, None) == nbx.NBX_ERR_ARG and L.nbx_last_error()
    L.nbx_ensemble_destroy(None)  # NULL-safe
    L.nbx_ensemble_destroy(null)
    d = (ctypes.c_double * 4)()
    st = nbx.EnsembleStats()
    for f in (lambda: L.nbx_ensemble_upload(null, 0, 1, *([null] * 7)), lambda: L.nbx_ensemble_step(null, 0.1, 1, None),
              lambda: L.nbx_ensemble_step_trace(null, 0.1, 1, d), lambda: L.nbx_ensemble_step_trace(null, 0.1, 1, None),
              lambda: L.nbx_ensemble_download(null, 0, 1, *([null] * 6)), lambda: L.nbx_ensemble_sync(null),
              lambda: L.nbx_ensemble_profile(null, 1), lambda: L.nbx_ensemble_stats(null, ctypes.byref(st)),
              lambda: L.nbx_ensemble_stats(null, None)):
        assert f() == nbx.NBX_ERR_ARG
        assert L.nbx_last_error()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly_no_cpu_fallback(nbx):
    for n, precision, members, opts in ((2048, 32, 64, {}), (5, 64, 1, {"bodies_per_lane": 8}), (16383, 32, 2, {"inner_loop": 2})):
        rc, text = _create(nbx, n, precision, members, **opts)
        assert rc == nbx.NBX_ERR_DEVICE, (rc, text)
        assert "no HIP device" in text
    with pytest.raises(nbx.NbxError) as e:
        nbx.Ensemble(1000, 8)
    assert e.value.code == nbx.NBX_ERR_DEVICE


# ---------------------------------------------------------------------------------------------------------------------------
# planner
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eplan") / "ensemble_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def _rows(driver, mode, rows, cus=256):
    text = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    out = subprocess.run([driver, mode, str(cus)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    res = []
    for line in out:
        kind, *vals = line.split(" ", 2) if line.startswith("E") else line.split()
        res.append((kind, vals if kind == "E" else [int(v) for v in vals]))
    return res


def test_one_member_takes_the_plan_of_a_single_context(driver):
    """members == 1: NB, loop and grid.x are what plan_launch gives a jlane context of that size (256 CUs)."""
    for precision, sizes in ((32, (5, 2000, 2048, 4096, 8192, 12288, 13000, 16383)), (64, (5, 2000, 2048, 4096, 8192, 12288))):
        ens = _rows(driver, "rows", [(n, precision, 1, 0, 0) for n in sizes])
        ctx = _rows(driver, "context", [(n, precision) for n in sizes])
        for n, (ke, e), (kc, c) in zip(sizes, ens, ctx):
            assert ke == "P" and kc == "P", (n, e, c)
            NB, loop, D, gx, gy, n_alloc = e
            assert [NB, loop, gx] == c, (n, precision, e, c)
            assert gy == 1 and n_alloc == -(-n // 256) * 256
            assert D == ((8 if NB <= 4 else 4) if precision == 32 else (8 if NB == 2 else 4))


def test_cost_model_counts_the_waves_of_all_members(driver):
    """cost(nb) = ceil(S * ceil(n / nb) / (4 * CUs)) * nb * weight(nb), weight 2 -> 129, 4 -> 106, 8 -> 100, 16 -> 106, and 16 -> 97
    in an ensemble (S > 1) whose S * ceil(n / 16) waves are at least one per SIMD (the sweep: profiles/ensemble_sweep.json);
    smallest wins, ties to the larger nb.  By hand at 256 CUs (1024 SIMDs), fp32, as (nb: waves -> rounds x nb x weight):
      (2048, 64): 2: 65536 -> 64 x 258 = 16512; 4: 32768 -> 32 x 424 = 13568; 8: 16384 -> 16 x 800 = 12800; 16: 8192 -> 8 x 1552 = 12416 => 16
      (2048,  4): 2: 4096 -> 4 x 258 = 1032;    4: 2048 -> 2 x 424 = 848;      8: 1024 -> 1 x 800 = 800;      16: 512 (< 1024) -> 1 x 1696 => 8
      (2048,  2): 2: 2048 -> 2 x 258 = 516;     4: 1024 -> 1 x 424 = 424;      8: 512 -> 1 x 800 = 800;       16: 256 -> 1 x 1696          => 4
      (8192, 16): 2: 65536 -> 16512;            4: 32768 -> 13568;             8: 16384 -> 12800;             16: 8192 -> 8 x 1552 = 12416 => 16
      (4096,  4): 2: 8192 -> 8 x 258 = 2064;    4: 4096 -> 4 x 424 = 1696;     8: 2048 -> 2 x 800 = 1600;     16: 1024 -> 1 x 1552         => 16
      (2048, 1) -> 2, (4096, 1) -> 4, (8192, 1) -> 8, (16383, 1): 8: 2048 -> 1600; 16: 1024 -> 1 x 1696 => 8: a lone system keeps its table.
    (Before the sweep the weight of 16 was 106 everywhere, which gave 8 at (2048, 64), (8192, 16) and (4096, 4); 16 measured 2-8 %
    faster at each.)  Loop under AUTO: the generated loop for NB = 8, and for NB = 4 with more than one wave per SIMD -- (2048, 2)
    has exactly 1024 waves of four bodies, one per SIMD: the compiled loop; NB = 16 has the compiled loop only."""
    cases = [((2048, 32, 64, 0, 0), 16, LOOP_CXX), ((2048, 32, 4, 0, 0), 8, LOOP_ASM), ((2048, 32, 2, 0, 0), 4, LOOP_CXX),
             ((8192, 32, 16, 0, 0), 16, LOOP_CXX), ((4096, 32, 4, 0, 0), 16, LOOP_CXX), ((2048, 32, 1, 0, 0), 2, LOOP_CXX),
             ((4096, 32, 1, 0, 0), 4, LOOP_CXX), ((8192, 32, 1, 0, 0), 8, LOOP_ASM), ((16383, 32, 1, 0, 0), 8, LOOP_ASM)]
    got = _rows(driver, "rows", [c[0] for c in cases])
    for (row, NB, loop), (kind, v) in zip(cases, got):
        assert kind == "P", (row, v)
        n, _, S = row[:3]
        assert v[0] == NB and v[1] == loop, (row, v)
        assert v[3] == -(-(-(-n // NB)) // 4) and v[4] == S, (row, v)
    # NB = 4 with two waves per SIMD takes the generated loop; explicit choices override the model and the loop rule
    got = _rows(driver, "rows", [(4096, 32, 2, 4, 0), (2048, 32, 64, 2, 0), (2048, 32, 64, 2, 2), (2048, 32, 64, 8, 1), (2048, 32, 64, 16, 0),
                                 (2000, 64, 8, 0, 0), (2000, 64, 8, 4, 1)])
    assert [v[:2] for _, v in got] == [[4, LOOP_ASM], [2, LOOP_CXX], [2, LOOP_ASM], [8, LOOP_CXX], [16, LOOP_CXX], [8, LOOP_CXX], [4, LOOP_CXX]]
    # the generated loop asked for by name, bodies per wave left to the planner: the choice is among the shapes that have one
    got = _rows(driver, "rows", [(2048, 32, 64, 0, 2), (16383, 32, 2, 0, 2), (2048, 32, 64, 0, 1)])
    assert [v[:2] for _, v in got] == [[8, LOOP_ASM], [8, LOOP_ASM], [16, LOOP_CXX]]


def test_planner_errors_carry_a_text(driver):
    rows = [(0, 32, 4, 0, 0), (16384, 32, 4, 0, 0), (12289, 64, 4, 0, 0), (100, 32, 0, 0, 0), (100, 32, 65536, 0, 0), (100, 16, 4, 0, 0),
            (100, 64, 4, 16, 0), (100, 32, 4, 16, 2), (100, 64, 4, 0, 2)]
    for row, (kind, v) in zip(rows, _rows(driver, "rows", rows)):
        assert kind == "E" and int(v[0]) == -1 and v[1].startswith("nbx_ensemble_create: "), (row, v)


def test_every_ensemble_plan_names_a_compiled_instance(driver):
    for cus in (256, 304, 64):
        r = subprocess.run([driver, "walk", str(cus)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:]
        assert int(r.stdout.split()[0]) > 1500, r.stdout


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the ensemble translation unit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ensemble_isa(tmp_path_factory):
    from test_isa_audit import _shipped_hipflags
    out = tmp_path_factory.mktemp("isa") / "nbx_ensemble.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", ENSEMBLE_SRC, "-o", str(out)])
    txt = open(out).read()
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3))
    return ks


def _ensemble_key(name):
    m = re.search(r"20ensemble_step_kernelILi(\d+)ELi(\d+)ELi(\d)E", name)
    if m:
        return (32, int(m.group(1)), int(m.group(3))), int(m.group(2))
    m = re.search(r"24ensemble_step_kernel_f64ILi(\d+)ELi(\d+)E", name)
    if m:
        return (64, int(m.group(1)), 0), int(m.group(2))
    return None


def test_compiled_ensemble_kernels_are_exactly_the_declared_instances(ensemble_isa, driver):
    declared = [tuple(map(int, l.split())) for l in subprocess.check_output([driver, "instances"], text=True).splitlines()]
    assert len(declared) == len(set(declared)) == 10
    steps = [k for k in ensemble_isa if "ensemble_step_kernel" in k]
    keys = [_ensemble_key(k) for k in steps]
    assert sorted(k for k, _ in keys) == sorted(declared)
    for (precision, NB, _), D in keys:  # the prefetch depth a context of that NB uses
        assert D == ((8 if NB <= 4 else 4) if precision == 32 else (8 if NB == 2 else 4)), (precision, NB, D)
    others = [k for k in ensemble_isa if k not in steps]
    assert len(others) == 1 and "ensemble_ke_reduce_kernel" in others[0], others
    assert not [k for k in ensemble_isa if re.search(r"force_(jlane_|exact_)?kernel", k)]


def test_ensemble_kernels_no_scratch_no_sgpr_spills_vector_stores_only(ensemble_isa):
    for name, (body, desc) in ensemble_isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert "v_writelane_b32" not in body and "v_readlane_b32" not in body, name
        assert not re.search(r"\b(global|buffer|flat)_atomic", body), name
        stores = set(re.findall(r"^\s+(\w*store\w*)", body, re.M))
        assert stores and all(s.startswith("global_store") for s in stores), (name, sorted(stores))
        assert re.search(r"\.amdhsa_system_sgpr_workgroup_id_y 1\b", desc) or "ke_reduce" in name, name  # the member index


def test_fp32_ensemble_kernels_run_the_packed_pair_with_the_raw_rsq(ensemble_isa):
    seen = 0
    for name, (body, _) in ensemble_isa.items():
        key = _ensemble_key(name)
        if not key or key[0][0] != 32:
            continue
        seen += 1
        assert "v_pk_fma_f32" in body and "v_pk_mul_f32" in body and "v_rsq_f32" in body, name
        assert "v_div_scale" not in body and "v_sqrt_f32" not in body, name
        if key[0][2] == LOOP_ASM:  # the generated loop of nbx_jlane_loop.inc, as it is: 8 records per lane and trip
            asm = [m.group(0) for m in re.finditer(r"#ASMSTART.*?#ASMEND", body, re.S) if "v_rsq_f32" in m.group(0)]
            assert len(asm) == 1 and asm[0].count("v_rsq_f32") == 8 * key[0][1], name
    assert seen == 7
