"""Ragged ensembles (include/nbx_ragged.h), the parts that need no GPU: the header and the exported symbols, the argument checks
of nbx_ragged_create (all of which run before the first HIP call), the host-only planner plan_ragged through a g++ driver --
its choice against plan_ensemble's where all members are equal, its layout and work list where they are not -- and an audit
of the cross-compiled gfx950 code of nbx_ragged.hip."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT, PKG, has_gpu
from test_ensemble_cpu import BAD_ARGS as ENSEMBLE_BAD_ARGS

CSRC = os.path.join(PKG, "csrc")
RAGGED_SRC = os.path.join(CSRC, "nbx_ragged.hip")
DRIVER = os.path.join(ROOT, "tests", "ragged_plan_driver.cpp")
LOOP_CXX, LOOP_ASM = 0, 1  # nbx_plan.hpp's internal LOOP_*
STATS_FIELDS = ("members", "precision", "n_min", "n_max", "bodies_total", "bodies_per_lane", "inner_loop", "grid_x", "block", "cu_count",
                "pairs_per_step", "steps_done", "launches_timed", "step_ms_total")


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))


def test_ragged_symbols_are_exported_and_kept_apart_from_the_other_headers(nbx):
    declared = _declared("nbx_ragged.h")
    assert len(declared) == 9 and set(declared) == set(nbx.RAGGED_SYMBOLS)
    others = set(nbx.SYMBOLS) | set(nbx.DIAG_SYMBOLS) | set(nbx.ENSEMBLE_SYMBOLS) | set(nbx.ENSEMBLE_DIAG_SYMBOLS)
    assert not set(declared) & others
    for h in ("nbx.h", "nbx_diag.h", "nbx_ensemble.h", "nbx_ensemble_diag.h"):
        assert not set(declared) & set(_declared(h)), h
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    L = nbx.load()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s
        assert getattr(L, s) is not None


def test_ragged_header_compiles_as_c99_and_matches_the_ctypes_mirror(nbx, tmp_path):
    src = tmp_path / "rag.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_ragged.h"\n'
                   'int main(void) { printf("%zu", sizeof(nbx_ragged_stats_t));\n'
                   + "".join('printf(" %%zu", offsetof(nbx_ragged_stats_t, %s));\n' % f for f in STATS_FIELDS)
                   + 'printf("\\n"); return NBX_ABI_VERSION - 1; }\n')
    exe = str(tmp_path / "rag.x")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    S = nbx.RaggedStats
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in STATS_FIELDS]
    assert S.struct_size.offset == 0 and set(STATS_FIELDS) == set(S().asdict())


def _create(nbx, sizes, precision, members=None, **opts):
    L = nbx.load()
    h = ctypes.c_void_p()
    o = nbx.Opts()
    o.struct_size = ctypes.sizeof(nbx.Opts)
    o.device = -1
    for k, v in opts.items():
        setattr(o, k, v)
    n = None if sizes is None else (ctypes.c_int32 * max(len(sizes), 1))(*sizes)
    rc = L.nbx_ragged_create(ctypes.byref(h), len(sizes) if members is None else members, n, precision, ctypes.byref(o))
    text = L.nbx_last_error().decode()
    if h.value:
        L.nbx_ragged_destroy(h)
    return rc, text


BAD_ARGS = [
    ([], 32, 0, {}, "members"), ([1000], 32, 65536, {}, "members"), (None, 32, 3, {}, "n is NULL"),
    ([1000, 0, 300], 32, None, {}, "n[1]"), ([5, 1000, 16384], 32, None, {}, "n[2]"), ([12289, 7], 64, None, {}, "n[0]"),
    ([300, 12288, 12289, 12290], 64, None, {}, "n[2]"),  # the first offender
    ([1000, 300], 16, None, {}, "precision"),
] + [([n, 300], precision, None, opts, word) for n, precision, _, opts, word in ENSEMBLE_BAD_ARGS if opts]


@pytest.mark.parametrize("sizes,precision,members,opts,word", BAD_ARGS)
def test_create_rejects_bad_arguments_before_any_device_call(nbx, sizes, precision, members, opts, word):
    rc, text = _create(nbx, sizes, precision, members, **opts)
    assert rc == nbx.NBX_ERR_ARG, (rc, text)
    assert text.startswith("nbx_ragged_create: ") and word in text, text


def test_every_opts_field_the_ensemble_rejects_is_tried():
    assert len([b for b in BAD_ARGS if b[3]]) == len([b for b in ENSEMBLE_BAD_ARGS if b[3]]) >= 11
    assert {"kernel_variant", "summation_order", "j_split", "i_begin", "i_count", "external_stream", "bodies_per_lane", "inner_loop"} <= \
        set().union(*[set(b[3]) for b in BAD_ARGS])


def test_null_arguments(nbx):
    L = nbx.load()
    null = ctypes.c_void_p()
    one = (ctypes.c_int32 * 1)(100)
    assert L.nbx_ragged_create(None, 1, one, 32, None) == nbx.NBX_ERR_ARG and L.nbx_last_error()
    L.nbx_ragged_destroy(None)  # NULL-safe
    L.nbx_ragged_destroy(null)
    d = (ctypes.c_double * 4)()
    st = nbx.RaggedStats()
    for f in (lambda: L.nbx_ragged_upload(null, 0, 1, *([null] * 7)), lambda: L.nbx_ragged_step(null, 0.1, 1, None),
              lambda: L.nbx_ragged_step_trace(null, 0.1, 1, d), lambda: L.nbx_ragged_step_trace(null, 0.1, 1, None),
              lambda: L.nbx_ragged_download(null, 0, 1, *([null] * 6)), lambda: L.nbx_ragged_sync(null),
              lambda: L.nbx_ragged_profile(null, 1), lambda: L.nbx_ragged_stats(null, ctypes.byref(st)),
              lambda: L.nbx_ragged_stats(null, None)):
        assert f() == nbx.NBX_ERR_ARG
        assert L.nbx_last_error()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly_no_cpu_fallback(nbx):
    for sizes, precision, opts in (([2048] * 64, 32, {}), ([5, 12288, 300], 64, {"bodies_per_lane": 8}), ([16383, 5, 8192], 32, {"inner_loop": 2})):
        rc, text = _create(nbx, sizes, precision, **opts)
        assert rc == nbx.NBX_ERR_DEVICE, (rc, text)
        assert "no HIP device" in text
    with pytest.raises(nbx.NbxError) as e:
        nbx.Ragged([1000, 300, 2048])
    assert e.value.code == nbx.NBX_ERR_DEVICE


# ---------------------------------------------------------------------------------------------------------------------------
# planner
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rplan") / "ragged_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe])
    return exe


def _uniform(driver, rows, cus=256):
    text = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    out = subprocess.run([driver, "uniform", str(cus)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    return [(l.split()[0], l.split(" ", 2)[1:] if l.startswith("E") else [int(v) for v in l.split()[1:]]) for l in out]


def _plan(driver, sizes, precision=32, bpl=0, il=0, cus=256):
    text = "%d %d %d %d %s\n" % (precision, bpl, il, len(sizes), " ".join(map(str, sizes)))
    out = subprocess.run([driver, "plan", str(cus)], input=text, capture_output=True, text=True, check=True).stdout
    return json.loads(out)


# the rows of test_ensemble_cpu.test_cost_model_counts_the_waves_of_all_members: (n, precision, members, bodies_per_lane, inner_loop)
UNIFORM_ROWS = [(2048, 32, 64, 0, 0), (2048, 32, 4, 0, 0), (2048, 32, 2, 0, 0), (8192, 32, 16, 0, 0), (4096, 32, 4, 0, 0), (2048, 32, 1, 0, 0),
                (4096, 32, 1, 0, 0), (8192, 32, 1, 0, 0), (16383, 32, 1, 0, 0),
                (4096, 32, 2, 4, 0), (2048, 32, 64, 2, 0), (2048, 32, 64, 2, 2), (2048, 32, 64, 8, 1), (2048, 32, 64, 16, 0), (2000, 64, 8, 0, 0),
                (2000, 64, 8, 4, 1), (2048, 32, 64, 0, 2), (16383, 32, 2, 0, 2), (2048, 32, 64, 0, 1)]
UNIFORM_EXPECT = [(16, LOOP_CXX), (8, LOOP_ASM), (4, LOOP_CXX), (16, LOOP_CXX), (16, LOOP_CXX), (2, LOOP_CXX), (4, LOOP_CXX), (8, LOOP_ASM),
                  (8, LOOP_ASM), (4, LOOP_ASM), (2, LOOP_CXX), (2, LOOP_ASM), (8, LOOP_CXX), (16, LOOP_CXX), (8, LOOP_CXX), (4, LOOP_CXX),
                  (8, LOOP_ASM), (8, LOOP_ASM), (16, LOOP_CXX)]


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_equal_members_take_exactly_the_plan_of_an_ensemble(driver, cus):
    got = _uniform(driver, UNIFORM_ROWS, cus)
    for i, (row, (kind, v)) in enumerate(zip(UNIFORM_ROWS, got)):
        assert kind == "P", (row, v)
        NB, loop, D, W, eNB, eloop, eD, egx, egy = v
        assert (NB, loop, D) == (eNB, eloop, eD) and W == egx * egy and egy == row[2], (row, v)
        if cus == 256:  # the values the ensemble test derives by hand
            assert (NB, loop) == UNIFORM_EXPECT[i], (row, v)


def test_both_planners_refuse_the_same_uniform_rows(driver):
    rows = [(0, 32, 4, 0, 0), (16384, 32, 4, 0, 0), (12289, 64, 4, 0, 0), (100, 32, 0, 0, 0), (100, 32, 65536, 0, 0), (100, 16, 4, 0, 0),
            (100, 64, 4, 16, 0), (100, 32, 4, 16, 2), (100, 64, 4, 0, 2)]
    for row, (kind, v) in zip(rows, _uniform(driver, rows)):
        assert kind == "E" and int(v[0]) == -1 and v[1].startswith("nbx_ragged_create: "), (row, v)


def test_the_walk_of_the_ensemble_planner_gives_the_same_plans(driver):
    for cus in (256, 304, 64):
        r = subprocess.run([driver, "walk", str(cus)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        assert int(r.stdout.split()[0]) > 1500, r.stdout


MIXED = [(5, 65, 1000, 256, 257, 2000, 63), (16383, 5, 8192)]


@pytest.mark.parametrize("sizes", MIXED)
@pytest.mark.parametrize("precision,bpl", [(32, 0), (32, 2), (32, 16), (64, 0)])
def test_mixed_members_layout_and_work_list(driver, sizes, precision, bpl):
    if precision == 64:
        sizes = tuple(min(n, 12288) for n in sizes)
    p = _plan(driver, sizes, precision, bpl)
    NB, spare = p["NB"], p["spare"]
    assert p["instance"] in range(10) and NB in ((2, 4, 8, 16) if precision == 32 else (2, 4, 8)) and (not bpl or NB == bpl)
    assert p["D"] == ((8 if NB <= 4 else 4) if precision == 32 else (8 if NB == 2 else 4))
    assert p["pairs"] == float(sum(n * n for n in sizes))
    mem = p["member"]
    assert len(mem) == len(sizes)
    for n, (pos, vel, ke, grid, mn, n_alloc) in zip(sizes, mem):
        assert mn == n and n_alloc == -(-n // 256) * 256 and grid == -(-(-(-n // NB)) // 4)
    # every (member, wg < grid_k) exactly once, and each descriptor carries its member's own offsets
    work = p["work"]
    assert p["W"] == len(work) == sum(m[3] for m in mem) == p["ke_parts"]
    assert sorted((w[0], w[1]) for w in work) == [(k, wg) for k in range(len(sizes)) for wg in range(mem[k][3])]
    for k, wg, pos, vel, ke, n, n_alloc in work:
        assert [pos, vel, ke, n, n_alloc] == mem[k][:3] + mem[k][4:], (k, wg)
    # longest member first, ties to the lower member index, wg ascending
    key = [(-w[6], w[0], w[1]) for w in work]
    assert key == sorted(key)
    # the members' ranges are disjoint and inside the buffers: positions with their spare records, velocities, partials
    for lo, length, total in ((0, lambda m: m[5] + spare, p["pos_records"]), (1, lambda m: m[5], p["vel_records"]), (2, lambda m: m[3], p["ke_parts"])):
        spans = sorted((m[lo], m[lo] + length(m)) for m in mem)
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    assert spare >= 64 * 8 + 16  # the jlane body's farthest prefetch: D <= 8 blocks of 64 records


def test_the_planner_counts_the_waves_of_all_members(driver):
    """cost(nb) = ceil(sum_k ceil(n_k / nb) / (4 CUs)) * nb * weight(nb), weights as for an ensemble.  By hand at 256 CUs (1024 SIMDs),
    fp32: (2048, 1024) x 32 each: nb 2: 32 x (1024 + 512) = 49152 waves -> 48 rounds x 258 = 12384; 4: 24576 -> 24 x 424 = 10176;
    8: 12288 -> 12 x 800 = 9600; 16: 6144 (>= 1024: weight 97) -> 6 x 1552 = 9312 => 16, the compiled loop.
    (300, 5): nb 2: 153 waves -> 1 x 258; 4: 77 -> 424; 8: 39 -> 800; 16: 20 (< 1024) -> 1696 => 2; one wave per SIMD at most: compiled loop.
    (2048, 2000, 100, 4): nb 4: 512 + 500 + 25 + 1 = 1038 waves -> 2 x 424 = 848; 8: 256 + 250 + 13 + 1 = 520 -> 800; 2: 2076 -> 3 x 258 = 774;
    16: 261 -> 1696 => 2."""
    for sizes, NB, loop in (((2048, 1024) * 32, 16, LOOP_CXX), ((300, 5), 2, LOOP_CXX), ((2048, 2000, 100, 4), 2, LOOP_CXX)):
        p = _plan(driver, sizes)
        assert (p["NB"], p["loop"]) == (NB, loop), (sizes, p["NB"], p["loop"])
    # NB = 4 asked for: 1038 waves are more than one per SIMD, so AUTO takes the generated loop; with (2048, 2000) alone (1012 waves) it does not
    assert _plan(driver, (2048, 2000, 100, 4), bpl=4)["loop"] == LOOP_ASM
    assert _plan(driver, (2048, 2000), bpl=4)["loop"] == LOOP_CXX


# ---------------------------------------------------------------------------------------------------------------------------
# the compiled gfx950 code of the ragged translation unit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged_isa(tmp_path_factory):
    from test_isa_audit import _shipped_hipflags
    out = tmp_path_factory.mktemp("isa") / "nbx_ragged.s"
    subprocess.check_call(["hipcc"] + _shipped_hipflags() + ["-S", "--cuda-device-only", RAGGED_SRC, "-o", str(out)])
    txt = open(out).read()
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3))
    return ks


def _ragged_key(name):
    m = re.search(r"18ragged_step_kernelILi(\d+)ELi(\d+)ELi(\d)E", name)
    if m:
        return (32, int(m.group(1)), int(m.group(3))), int(m.group(2))
    m = re.search(r"22ragged_step_kernel_f64ILi(\d+)ELi(\d+)E", name)
    if m:
        return (64, int(m.group(1)), 0), int(m.group(2))
    return None


def test_compiled_ragged_kernels_are_exactly_the_declared_instances(ragged_isa, driver):
    declared = [tuple(map(int, l.split())) for l in subprocess.check_output([driver, "instances"], text=True).splitlines()]
    assert len(declared) == len(set(declared)) == 10
    steps = [k for k in ragged_isa if "ragged_step_kernel" in k]
    keys = [_ragged_key(k) for k in steps]
    assert sorted(k for k, _ in keys) == sorted(declared)
    for (precision, NB, _), D in keys:  # the prefetch depth a context of that NB uses
        assert D == ((8 if NB <= 4 else 4) if precision == 32 else (8 if NB == 2 else 4)), (precision, NB, D)
    others = [k for k in ragged_isa if k not in steps]
    assert len(others) == 1 and "ragged_ke_reduce_kernel" in others[0], others
    assert not [k for k in ragged_isa if re.search(r"force_\w*kernel|ensemble_", k)]


def test_ragged_kernels_no_scratch_no_sgpr_spills(ragged_isa):
    assert len(ragged_isa) == 11
    for name, (body, desc) in ragged_isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert "v_writelane_b32" not in body and "v_readlane_b32" not in body, name


def test_fp32_ragged_kernels_run_the_packed_pair_with_the_raw_rsq(ragged_isa):
    seen = 0
    for name, (body, _) in ragged_isa.items():
        key = _ragged_key(name)
        if not key or key[0][0] != 32:
            continue
        seen += 1
        assert "v_pk_fma_f32" in body and "v_pk_mul_f32" in body and "v_rsq_f32" in body, name
        assert "v_div_scale" not in body and "v_sqrt_f32" not in body, name
        if key[0][2] == LOOP_ASM:  # the generated loop of nbx_jlane_loop.inc, as it is: 8 records per lane and trip
            asm = [m.group(0) for m in re.finditer(r"#ASMSTART.*?#ASMEND", body, re.S) if "v_rsq_f32" in m.group(0)]
            assert len(asm) == 1 and asm[0].count("v_rsq_f32") == 8 * key[0][1], name
    assert seen == 7
