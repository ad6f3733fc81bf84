"""A/B of two builds of libnbx.so (tools/build_variant.sh) on the context call of every unit that stands on csrc/nbx_tilewalk.hpp,
at n = 131072 -- 256 columns by 4 splits, where a call is milliseconds of pair work: the cell the *_cost.py tools call
context_n131072.  One child process per library and round, the libraries alternated (the pattern of tools/lib_ab.py) and the
first of a round alternated too, so that clock drift and what the previous process left behind hit both alike; a child times
every cell, fp32 and fp64, as the median of its passes after one warm-up call.

Per cell: the median over the rounds of each library, and the parent's own round-to-round range in this session -- the margin:
a difference smaller than that cannot be told from noise on a shared machine.  verdict "slower" where head's median lies above
the parent's slowest round.

usage: python tools/tilewalk_ab.py [--rounds R] [--passes P] [--units a,b,...] [--out FILE] PARENT_LIB HEAD_LIB   (GPU box, repo root)
Writes profiles/tilewalk_ab.json; the cells of units that were not asked for stay as the file has them."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "tilewalk_ab.json")
N = 131072
UNITS = ("field", "neighbours", "paircount", "tracers", "knn", "fof", "binaries", "tidal", "nlist", "jerk", "timescale")


def cells(c, s):
    """{unit: a call that ends synchronised} on context c holding state s"""
    pts = (s["pos_x"], s["pos_y"], s["pos_z"])

    def tracers():
        c.tracers_kick(1e-3)  # one pair-work launch and one update launch at the bodies' current positions
        c.sync()

    return {"field": lambda: c.field(*pts), "neighbours": lambda: c.neighbours(0.05), "paircount": lambda: c.paircount([0.02, 0.05, 0.1, 0.2]),
            "tracers": tracers, "knn": lambda: c.knn(8), "fof": lambda: c.fof(0.01), "binaries": c.binaries, "tidal": lambda: c.tidal(*pts),
            "nlist": lambda: c.nlist(0.02, capacity=0), "jerk": c.jerk, "timescale": c.timescale}


def child(units, passes):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
    import binaries_cost as BC
    import nbx
    out = {}
    for precision in (32, 64):
        s = BC.member_state(N, 999, np.float32 if precision == 32 else np.float64)
        c = nbx.Context(N, precision)
        try:
            c.upload(s)
            c.tracers_upload((s["pos_x"], s["pos_y"], s["pos_z"]), (s["vel_x"], s["vel_y"], s["vel_z"]))
            todo = cells(c, s)
            for u in units:
                todo[u]()  # warm-up: scratch is allocated here
                ms = []
                for _ in range(passes):
                    t0 = time.perf_counter()
                    todo[u]()
                    ms.append((time.perf_counter() - t0) * 1e3)
                out["%s fp%d" % (u, precision)] = statistics.median(ms)
        finally:
            c.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--units", default=",".join(UNITS))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("libs", nargs="*")
    a = ap.parse_args()
    units = a.units.split(",")
    if a.child:
        return child(units, a.passes)
    assert a.rounds >= 5 and len(a.libs) == 2
    libs = (("parent", a.libs[0]), ("head", a.libs[1]))
    ms = {name: {} for name, _ in libs}
    for r in range(a.rounds):
        for name, path in (libs if r % 2 == 0 else libs[::-1]):  # the libraries alternated, and who goes first in a round too
            env = dict(os.environ, NBX_LIB=os.path.abspath(path))
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--passes", str(a.passes), "--units", a.units], env=env,
                               capture_output=True, text=True, timeout=300)
            line = [l for l in o.stdout.splitlines() if l.startswith("RESULT ")]
            if o.returncode != 0 or not line:
                print("child failed for %s (exit %d):\n%s\n%s" % (name, o.returncode, o.stdout[-2000:], o.stderr[-2000:]), flush=True)
                return 1
            for cell, v in json.loads(line[0][7:]).items():
                ms[name].setdefault(cell, []).append(v)
        print("round %d done" % r, flush=True)
    out = {"cells": {}}
    if os.path.exists(a.out):  # a run of some units replaces their cells and keeps the others: a unit is measured again when it changes
        with open(a.out) as f:
            out = json.load(f)
    out.update({"what": "ms per context call at n = %d, each round the median of the passes of one child process per library, the libraries "
                        "alternated; margin: the parent's own fastest and slowest round of the cell's session; verdict slower: head's "
                        "median above the parent's slowest round" % N, "n": N})
    for key in ("rounds", "note", "superseded_cells"):
        out.pop(key, None)
    print("%-18s %11s %11s %8s   %s" % ("cell", "parent ms", "head ms", "head/par", "parent's range ms"))
    for cell in sorted(ms["parent"]):
        p, h = ms["parent"][cell], ms["head"][cell]
        pm, hm = statistics.median(p), statistics.median(h)
        verdict = "slower" if hm > max(p) else "within" if hm >= min(p) else "faster"
        out["cells"][cell] = {"parent_ms": pm, "head_ms": hm, "ratio": hm / pm, "parent_min_ms": min(p), "parent_max_ms": max(p), "verdict": verdict,
                              "rounds": a.rounds, "passes": a.passes, "parent_rounds_ms": p, "head_rounds_ms": h}
        print("%-18s %11.3f %11.3f %8.4f   %.3f .. %.3f  %s" % (cell, pm, hm, hm / pm, min(p), max(p), verdict), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
