"""Physics diagnostics (include/nbx_diag.h), the parts that need no GPU: the header, the exported symbols and their argument
checks, an audit of the cross-compiled gfx950 code of nbx_diag.hip, and ShardedSimulation.diagnostics() over gloo."""
import ctypes
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, PKG, rel_err

DIAG_SRC = os.path.join(PKG, "csrc", "nbx_diag.hip")


def test_diag_header_compiles_as_c99_and_matches_the_ctypes_mirror(nbx, tmp_path):
    src = tmp_path / "diag.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbx_diag.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(nbx_diag_t), offsetof(nbx_diag_t, steps_done), '
                   'offsetof(nbx_diag_t, potential), offsetof(nbx_diag_t, momentum), offsetof(nbx_diag_t, mass_moment)); '
                   'return (int)NBX_ERR_ARG + 1; }\n')
    exe = str(tmp_path / "diag.x")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    D = nbx.Diag
    assert got == [ctypes.sizeof(D), D.steps_done.offset, D.potential.offset, D.momentum.offset, D.mass_moment.offset]
    assert got[0] == 88


def test_diag_symbols_are_exported_and_kept_apart_from_nbx_h(nbx):
    txt = open(os.path.join(ROOT, "include", "nbx_diag.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nbx_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(nbx.DIAG_SYMBOLS)
    assert not set(nbx.DIAG_SYMBOLS) & set(nbx.SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", nbx.LIB_PATH]).decode()
    for s in declared:
        assert re.search(r" T %s$" % s, out, flags=re.M), s


def test_diag_entry_points_reject_null(nbx):
    L = nbx.load()
    d = nbx.Diag()
    null = ctypes.c_void_p()
    for f in (L.nbx_diagnostics, L.nbx_group_diagnostics):
        assert f(null, ctypes.byref(d)) == nbx.NBX_ERR_ARG
        assert L.nbx_last_error()
        assert f(null, None) == nbx.NBX_ERR_ARG


def test_context_diagnostics_method_exists_without_gpu_path(nbx):
    assert callable(nbx.Context.diagnostics) and callable(nbx.Group.diagnostics)
    d = nbx.Diag()
    d.kenergy, d.potential = 1.5, -4.0
    assert d.asdict()["etotal"] == -2.5


@pytest.fixture(scope="module")
def diag_isa(tmp_path_factory):
    mk = open(os.path.join(ROOT, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags
    out = tmp_path_factory.mktemp("isa") / "nbx_diag.s"
    subprocess.check_call(["hipcc"] + flags + ["-S", "--cuda-device-only", DIAG_SRC, "-o", str(out)])
    txt = open(out).read()
    ks = {}
    for m in re.finditer(r"\n(_ZN3nbx\w+):(.*?)\.amdhsa_kernel \1(.*?)\.end_amdhsa_kernel", txt, re.S):
        ks[m.group(1)] = (m.group(2), m.group(3))
    return ks


def _kernel(ks, pattern):
    names = [k for k in ks if re.search(pattern, k)]
    assert len(names) == 1, (pattern, list(ks))
    return ks[names[0]]


def test_diag_kernels_present(diag_isa):
    assert len(diag_isa) == 3, list(diag_isa)
    _kernel(diag_isa, r"diag_kernelIf")
    _kernel(diag_isa, r"diag_kernelId")
    _kernel(diag_isa, r"diag_reduce_kernel")


def test_fp32_potential_pair_is_raw_rsq(diag_isa):
    body, _ = _kernel(diag_isa, r"diag_kernelIf")
    assert re.search(r"\bv_rsq_f32", body)
    assert not re.search(r"\bv_div_scale|\bv_sqrt_f32|\bv_rcp_f32", body)
    # the pair on the packed pipe: 3 sub + 4 FMA per two bodies, in both the plain and the masked tile loop
    assert len(re.findall(r"\bv_pk_fma_f32", body)) >= 8 and len(re.findall(r"\bv_pk_add_f32", body)) >= 6
    assert re.search(r"\bds_read_b128", body)  # j records broadcast from the LDS tile


def test_fp64_potential_uses_the_newton_refined_rsq(diag_isa):
    body, _ = _kernel(diag_isa, r"diag_kernelId")
    assert re.search(r"\bv_rsq_f64", body)
    assert not re.search(r"\bv_div_scale|\bv_sqrt_f64", body)


def test_diag_kernels_no_scratch_no_atomics_vector_stores_only(diag_isa):
    for name, (body, desc) in diag_isa.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", desc), name
        assert not re.search(r"\b(global|buffer|flat)_atomic", body), name
        # results leave through vector stores: every line that stores to memory is a global_store
        stores = re.findall(r"^\s+(\w*store\w*)", body, re.M)
        assert stores and all(s.startswith("global_store") for s in stores), (name, sorted(set(stores)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("n,world", [(1000, 2), (1500, 3)])
def test_sharded_diagnostics_over_gloo_equal_the_single_process_value(nbx, tmp_path, n, world):
    import energy_ref
    out = str(tmp_path / "res")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", env["MASTER_PORT"],
           os.path.join(ROOT, "tests", "_diag_dist_worker.py"), str(n), out]
    subprocess.run(cmd, env=env, check=True, timeout=300, capture_output=True)
    res = [json.load(open("%s.%d" % (out, r))) for r in range(world)]
    state = nbx.initial_conditions(n)
    ref = energy_ref.diagnostics(state)
    pscale = energy_ref.momentum_scale(state)
    assert sum(r["i_count"] for r in res) == n
    for r in res:
        d = r["diag"]
        assert d == res[0]["diag"]  # every rank holds the same numbers
        for k in ("mass", "kenergy", "potential", "etotal"):
            assert rel_err(d[k], ref[k]) < 1e-12, (k, d[k], ref[k])
        assert np.abs(np.subtract(d["momentum"], ref["momentum"])).max() < 1e-12 * pscale
        assert rel_err(d["mass_moment"], ref["mass_moment"]).max() < 1e-12
        assert d["i_count"] == n and d["steps_done"] == 0


def test_variant_build_tool_links_the_diagnostics(nbx):
    """tools/build_variant.sh (A/B builds loaded through NBX_LIB) must build a library that nbx.load() accepts: the
    diagnostics translation unit and its header are part of every libnbx.so."""
    import shutil
    name = "test_diag_%d" % os.getpid()
    out = os.path.join(ROOT, "tools", "ab", name)
    try:
        subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), name], check=True, capture_output=True, timeout=900)
        lib = os.path.join(out, "libnbx.so")
        syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        for s in nbx.SYMBOLS + nbx.DIAG_SYMBOLS:
            assert re.search(r" T %s$" % s, syms, flags=re.M), s
        code = ("import sys; sys.path.insert(0, %r); import nbx; L = nbx.load(); assert L._name == %r; "
                "print(L.nbx_diagnostics(None, None))" % (PKG, lib))
        got = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, NBX_LIB=lib, NBX_NO_TORCH_PRELOAD="1"), text=True)
        assert got.strip() == str(nbx.NBX_ERR_ARG)
    finally:
        shutil.rmtree(out, ignore_errors=True)
