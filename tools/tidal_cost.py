"""Cost of the tidal tensor at caller-supplied points (include/nbx_tidal.h), in one process, fp32, with the machinery of
tools/field_cost.py (states, points, calibration, alternated rounds, medians):

  ensemble  16 members of 2048 bodies, m = 2048 points per member
            A  one nbx_ensemble_tidal call over all members
            B  16 nbx_tidal calls on 16 default contexts created and uploaded beforehand that hold the same states
  ragged    16 sizes spread over 512 ... 4096, m = 1024 points per member; A and B likewise (nbx_ragged_tidal)

B is not charged for creating or uploading the contexts.  A and B return the same bits (checked).  ratio = A / B.

A third cell is recorded, not gated: one context of 131072 bodies and as many points -- T one nbx_tidal call, F one nbx_field call
(upload of the points and read-back included in both): us of each and their quotient.  The instruction count suggests about
20 / 13 of the field's pair work; the read-back is six arrays against four.

usage: python tools/tidal_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/tidal_cost.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

import field_cost as FC

ROOT = FC.ROOT
OUT = os.path.join(ROOT, "profiles", "tidal_cost.json")
LARGE_N = FC.LARGE_N


def measure(nbx, kind, rounds=5, window=0.05):
    """A batch cell, kind "ensemble" or "ragged": one batch call against one nbx_tidal call per context."""
    assert rounds >= 5
    sizes = [FC.ENSEMBLE_N] * FC.MEMBERS if kind == "ensemble" else list(FC.RAGGED_SIZES)
    m = FC.ENSEMBLE_M if kind == "ensemble" else FC.RAGGED_M
    states = [FC.member_state(n, 1000 + k) for k, n in enumerate(sizes)]
    pts = [FC.member_points(m, 3000 + k) for k in range(FC.MEMBERS)]
    P = [np.ascontiguousarray(np.stack([q[c] for q in pts])) for c in range(3)]  # (members, m)
    batch = nbx.Ensemble(FC.ENSEMBLE_N, FC.MEMBERS, 32) if kind == "ensemble" else nbx.Ragged(sizes, 32)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, 32))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.tidal(*P), "B": lambda: [c.tidal(*q) for c, q in zip(ctxs, pts)]}
        a, b = arms["A"](), arms["B"]()
        same = all(a[k][j].tobytes() == b[j][k].tobytes() for j in range(FC.MEMBERS) for k in nbx.TIDAL_KEYS)
        us, passes = FC._time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    ta, tb = statistics.median(us["A"]), statistics.median(us["B"])
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "m": m, "precision": 32,
            "batch_us": ta, "contexts_us": tb, "ratio": ta / tb, "batch_rounds_us": us["A"], "contexts_rounds_us": us["B"],
            "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def measure_large(nbx, n=LARGE_N, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, nbx_tidal against nbx_field at the same n points."""
    assert rounds >= 5
    c = nbx.Context(n, 32)
    try:
        c.upload(FC.member_state(n, 999))
        p = FC.member_points(n, 998)
        us, passes = FC._time({"T": lambda: c.tidal(*p), "F": lambda: c.field(*p)}, rounds, window)
    finally:
        c.close()
    t, f = statistics.median(us["T"]), statistics.median(us["F"])
    return {"kind": "context", "n": n, "m": n, "precision": 32, "tidal_us": t, "field_us": f, "tidal_pairs_per_s": float(n) * n / (t * 1e-6),
            "field_pairs_per_s": float(n) * n / (f * 1e-6), "time_ratio": t / f, "packed_valu_ratio_expected": 20.0 / 13.0,
            "tidal_rounds_us": us["T"], "field_rounds_us": us["F"], "passes_per_round": passes}


WHAT = ("us per pass, fp32, medians of the rounds, arms alternated, one process.  ensemble (16 x 2048, m = 2048) and ragged (16 sizes "
        "over 512 ... 4096, m = 1024): one batch call against one nbx_tidal call on each of 16 default contexts created and uploaded "
        "beforehand; ratio = first arm / second arm (gated <= 1.0 by tests/test_tidal_gpu.py).  context_n131072: one nbx_tidal call "
        "at 131072 points against one nbx_field call at the same points on the same context, whole calls, recorded, not gated")


def write(path, cells):
    """Merge `cells` ({name: cell}) into the JSON file."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out["what"] = WHAT
    out.update(cells)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.1, help="seconds per timed round of an arm")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
    import nbx
    for kind in ("ensemble", "ragged"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-8s m = %d: batch %.1f us, 16 contexts %.1f us, ratio %.3f%s"
              % (kind, r["m"], r["batch_us"], r["contexts_us"], r["ratio"], "" if r["same_values_from_both_arms"] else "  VALUES DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = m = %d: tidal %.1f us, field %.1f us, time ratio %.2f (packed VALU: 20 / 13 = 1.54)"
          % (r["n"], r["tidal_us"], r["field_us"], r["time_ratio"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
