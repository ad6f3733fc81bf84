"""Cost of the time scales (include/nbx_timescale.h) of every member of a batch object, in one process:

  A  one nbx_ensemble_timescale / nbx_ragged_timescale call over all M members (one pair-work launch, one reduce launch, one
     read-back)
  B  M nbx_timescale calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and
     hold the same states (two launches and a synchronising read-back each)
  D  one diagnostics call on the same batch object (nbx_ensemble_diagnostics / nbx_ragged_diagnostics): the potential's pair
     loop over the same grid, recorded beside A and not gated

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts.  A and B return the same list of dicts (checked).  Per cell: the calibration passes double as warm-up,
then `rounds` rounds, the arms alternated; a round times `passes` back-to-back passes of an arm (each pass ends in a
synchronisation) so that it lasts >= `window` seconds; the figures are medians over the rounds, in us per pass.
ratio = A / B, against_diagnostics = A / D.

The cells above are launch-bound.  A third cell takes the pair loops themselves: one context of 131072 bodies, fp32, where a call
is milliseconds of pair work -- T one nbx_timescale call, D one nbx_diagnostics call, pair_loop_ratio = T / D, recorded.

usage: python tools/timescale_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/timescale_cost.json: an ensemble of 16 x 2048, a ragged ensemble of 16 sizes spread over 512 ... 4096 and a context
of 131072 bodies, fp32."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "timescale_cost.json")

MEMBERS = 16
ENSEMBLE_N = 2048
RAGGED_SIZES = [512 + round(k * (4096 - 512) / (MEMBERS - 1)) for k in range(MEMBERS)]  # 512 ... 4096, evenly


def member_state(n, seed, dtype):
    """n bodies, G sum m ~ 1, positions uniform in [-1, 1]^3, velocities 0.3 uniform in [-1, 1]^3 (the systems of the kick tests)."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.5, 1.5, n) / (6.67259e-11 * n)
    pos = rng.uniform(-1.0, 1.0, (3, n))
    vel = 0.3 * rng.uniform(-1.0, 1.0, (3, n))
    names = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in zip(names, list(pos) + list(vel) + [m])}


def _passes_for(run, window):
    """Passes per round such that a round lasts >= window seconds; the calibration passes double as warm-up."""
    k = 1
    while True:
        t0 = time.perf_counter()
        for _ in range(k):
            run()
        t = time.perf_counter() - t0
        if t >= window or k >= 1 << 16:
            return k
        k = max(2 * k, int(1.2 * k * window / max(t, 1e-7)) + 1)


def measure(nbx, kind, precision=32, rounds=5, window=0.05):
    """One cell, kind "ensemble" or "ragged".  Median us per pass of each arm, ratio = A / B, against_diagnostics = A / D."""
    assert rounds >= 5
    sizes = [ENSEMBLE_N] * MEMBERS if kind == "ensemble" else list(RAGGED_SIZES)
    dtype = np.float32 if precision == 32 else np.float64
    states = [member_state(n, 1000 + k, dtype) for k, n in enumerate(sizes)]
    batch = nbx.Ensemble(ENSEMBLE_N, MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arms = {"A": batch.timescale, "B": lambda: [c.timescale() for c in ctxs], "D": batch.diagnostics}
        same = arms["A"]() == arms["B"]()
        passes = {k: _passes_for(run, window) for k, run in arms.items()}
        us = {k: [] for k in arms}
        for _ in range(rounds):
            for k, run in arms.items():  # A B D A B D ...
                t0 = time.perf_counter()
                for _ in range(passes[k]):
                    run()
                us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b, d = (statistics.median(us[k]) for k in "ABD")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes),
            "precision": precision, "batch_us": a, "contexts_us": b, "diagnostics_us": d, "ratio": a / b, "against_diagnostics": a / d,
            "batch_rounds_us": us["A"], "contexts_rounds_us": us["B"], "diagnostics_rounds_us": us["D"], "passes_per_round": passes,
            "same_values_from_both_arms": bool(same)}


LARGE_N = 131072


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, a timescale call against a diagnostics call."""
    assert rounds >= 5
    c = nbx.Context(n, precision)
    try:
        c.upload(member_state(n, 999, np.float32 if precision == 32 else np.float64))
        arms = {"T": c.timescale, "D": c.diagnostics}
        passes = {k: _passes_for(run, window) for k, run in arms.items()}
        us = {k: [] for k in arms}
        for _ in range(rounds):
            for k, run in arms.items():  # T D T D ...
                t0 = time.perf_counter()
                for _ in range(passes[k]):
                    run()
                us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
    finally:
        c.close()
    t, d = statistics.median(us["T"]), statistics.median(us["D"])
    return {"kind": "context", "n": n, "precision": precision, "timescale_us": t, "diagnostics_us": d, "pair_loop_ratio": t / d,
            "timescale_pairs_per_s": float(n) * (n - 1) / (t * 1e-6), "diagnostics_pairs_per_s": float(n) * (n - 1) / (d * 1e-6),
            "timescale_rounds_us": us["T"], "diagnostics_rounds_us": us["D"], "passes_per_round": passes}


WHAT = ("us per pass over all 16 members, fp32; batch: one nbx_ensemble_timescale / nbx_ragged_timescale call; contexts: one "
        "nbx_timescale call on each of 16 default contexts, one per member, created and uploaded beforehand (not charged for "
        "download, create or upload); diagnostics: one diagnostics call on the batch object; medians of the rounds, arms "
        "alternated, one process; ratio = batch / contexts (gated <= 1.0 by tests/test_timescale_gpu.py), against_diagnostics = "
        "batch / diagnostics (recorded); context_n131072: one nbx_timescale call against one nbx_diagnostics call on one context of "
        "131072 bodies, where the pair loops are what is timed: pair_loop_ratio = timescale / diagnostics (recorded)")


def write(path, cells):
    """Merge `cells` ({kind: cell}) into the JSON file."""
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
    print("%-10s %10s %12s %14s %8s %10s" % ("kind", "batch us", "contexts us", "diagnostics us", "ratio", "vs diag"))
    for kind in ("ensemble", "ragged"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-10s %10.1f %12.1f %14.1f %8.3f %10.2f%s" % (kind, r["batch_us"], r["contexts_us"], r["diagnostics_us"], r["ratio"],
                                                             r["against_diagnostics"], "" if r["same_values_from_both_arms"] else "  VALUES DIFFER"),
              flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d: timescale %.1f us (%.3g pair/s), diagnostics %.1f us (%.3g pair/s), ratio %.2f"
          % (r["n"], r["timescale_us"], r["timescale_pairs_per_s"], r["diagnostics_us"], r["diagnostics_pairs_per_s"], r["pair_loop_ratio"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
