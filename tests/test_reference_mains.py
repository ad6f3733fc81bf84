"""Drop-in proof (skipped where oracle/_ref was not built, i.e. where the reference's sources are not at hand).

The reference's OWN, unmodified callers -- ver7/main.cpp, ver8/main.cpp (ver7/main.cpp:25-46) and ver5_all/main.cpp
(:23-66, which needs init_mpi(), world_rank and the <iostream>/<string> its GSimulation.hpp provides,
ver5_all/GSimulation.hpp:25-30,60-65) -- are compiled against host/GSimulation.{hpp,cpp} + libnbx and run.

`make -C oracle ref` (build()) compiles each main.cpp, fed to g++ on stdin, into oracle/_ref/<version>_main.o, so its
`#include "GSimulation.hpp"` cannot resolve to the header next to it and must find host/GSimulation.hpp through -I; the
headers it reached are recorded beside the object by -H.  Nothing of the reference is copied into the repo.
"""
import os
import subprocess

import pytest

from conftest import PKG, ROOT, has_gpu

REF_BUILD = os.path.join(ROOT, "oracle", "_ref")
HOST = os.path.join(PKG, "host")
MAINS = [("ver7", []), ("ver8", []), ("ver5_all", ["-DNBX_BANNER_IN_MAIN"])]
pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(REF_BUILD, v + "_main.o")) for v, _ in MAINS),
                                reason="oracle/_ref is only built where the reference's sources exist")


def _build(tmp_path, version, defs):
    if not os.path.exists(os.path.join(PKG, "libnbx.so")):
        subprocess.check_call(["make", "-s", "-C", ROOT, "lib"])
    exe = str(tmp_path / ("nbody_%s_main.x" % version))
    obj = os.path.join(REF_BUILD, version + "_main.o")
    with open(os.path.join(REF_BUILD, version + "_main.H")) as f:
        headers = [os.path.normpath(os.path.join(REF_BUILD, ln.split()[-1])) for ln in f if ln.startswith(".")]
    assert os.path.join(HOST, "GSimulation.hpp") in headers, headers
    # every header of the drop-in's name set came from host/, none from beside the reference's main.cpp
    own = set(os.listdir(HOST))
    assert all(os.path.dirname(h) == HOST for h in headers if os.path.basename(h) in own), headers
    subprocess.check_call(["g++", "-std=c++14", "-O2"] + defs + [os.path.join(HOST, "GSimulation.cpp"), obj, "-o", exe,
                                                                  "-L" + PKG, "-lnbx", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("version,defs", MAINS, ids=[m[0] for m in MAINS])
def test_unmodified_reference_main_builds_and_runs_against_the_drop_in(tmp_path, version, defs):
    exe = _build(tmp_path, version, defs)
    args = ["300", "100"] + (["gpu", "0.5", "256", "2"] if version == "ver5_all" else [])
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    lines = p.stdout.splitlines()
    if version == "ver5_all":
        assert lines[0] == "gpu"  # ver5_all/main.cpp:42 echoes the device word before the banner
        lines = lines[1:]
    assert lines[0] == "=" * 31 and lines[1] == " Initialize Gravity Simulation"
    assert lines[2] == " nPart = 300; nSteps = 100; dt = 0.1"
    assert lines[3] == "-" * 48
    if has_gpu():
        assert p.returncode == 0 and any(ln.startswith("# Average Perfomance : ") for ln in lines), p.stderr
    else:  # the product has no CPU path: the reference's caller gets the header, then a loud failure
        assert p.returncode != 0 and "no HIP device" in p.stderr


def test_reference_ver5_main_device_word_cpu_is_refused(tmp_path):
    exe = _build(tmp_path, "ver5_all", ["-DNBX_BANNER_IN_MAIN"])
    p = subprocess.run([exe, "300", "100", "cpu"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "no CPU engine" in p.stderr
    assert p.stdout.splitlines()[:3] == ["cpu", "=" * 31, " Initialize Gravity Simulation"]
