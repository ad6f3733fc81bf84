"""Cost of the nearest neighbours and radius counts (include/nbx_neighbours.h) of every member of a batch object, in one process:

  A  one nbx_ensemble_neighbours / nbx_ragged_neighbours call over all M members (one pair-work launch, one finish launch, one
     read-back), with the count
  B  M nbx_neighbours calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and
     hold the same states (two launches and a synchronising read-back each)

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts.  A and B return the same arrays (checked).  The cells, the warm-up and the repetitions are those of
tools/timescale_cost.py (its member_state and its calibration are used as they are): the calibration passes double as warm-up,
then `rounds` rounds, the arms alternated; a round times `passes` back-to-back passes of an arm (each pass ends in a
synchronisation) so that it lasts >= `window` seconds; the figures are medians over the rounds, in us per pass.  ratio = A / B.

The cells above are launch-bound.  A third cell takes the pair loops themselves: one context of 131072 bodies, fp32, where a call
is milliseconds of pair work -- N one nbx_neighbours call with the count, I one without, T one nbx_timescale call on the same
context; with_count_ratio = N / T, index_only_ratio = I / T and the implied pair/s, recorded and not gated.

usage: python tools/neighbours_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/neighbours_cost.json: an ensemble of 16 x 2048, a ragged ensemble of 16 sizes spread over 512 ... 4096 and a
context of 131072 bodies, fp32."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timescale_cost as TC  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "neighbours_cost.json")
RADIUS = 0.25
KEYS = ("index", "r2", "within")


def _same(a, b):
    """A's result (a dict of (M, n) arrays, or a list of dicts) against B's list of dicts: the same arrays."""
    if isinstance(a, dict):
        a = [{k: a[k][m] for k in KEYS} for m in range(len(b))]
    return len(a) == len(b) and all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in KEYS)


def _time(arms, rounds, window):
    passes = {k: TC._passes_for(run, window) for k, run in arms.items()}
    us = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():  # the arms alternated
            t0 = time.perf_counter()
            for _ in range(passes[k]):
                run()
            us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
    return us, passes


def measure(nbx, kind, precision=32, rounds=5, window=0.05):
    """One cell, kind "ensemble" or "ragged".  Median us per pass of each arm, ratio = A / B."""
    assert rounds >= 5
    sizes = [TC.ENSEMBLE_N] * TC.MEMBERS if kind == "ensemble" else list(TC.RAGGED_SIZES)
    dtype = np.float32 if precision == 32 else np.float64
    states = [TC.member_state(n, 1000 + k, dtype) for k, n in enumerate(sizes)]
    batch = nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.neighbours(RADIUS), "B": lambda: [c.neighbours(RADIUS) for c in ctxs]}
        same = _same(arms["A"](), arms["B"]())
        us, passes = _time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b = (statistics.median(us[k]) for k in "AB")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "radius": RADIUS, "batch_us": a, "contexts_us": b, "ratio": a / b, "batch_rounds_us": us["A"], "contexts_rounds_us": us["B"],
            "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


LARGE_N = 131072


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, a neighbours call with and without the count against a timescale call."""
    assert rounds >= 5
    c = nbx.Context(n, precision)
    try:
        c.upload(TC.member_state(n, 999, np.float32 if precision == 32 else np.float64))
        arms = {"N": lambda: c.neighbours(RADIUS), "I": c.neighbours, "T": c.timescale}
        us, passes = _time(arms, rounds, window)
    finally:
        c.close()
    w, i, t = (statistics.median(us[k]) for k in "NIT")
    pairs = float(n) * (n - 1)
    return {"kind": "context", "n": n, "precision": precision, "radius": RADIUS, "with_count_us": w, "index_only_us": i, "timescale_us": t,
            "with_count_ratio": w / t, "index_only_ratio": i / t, "with_count_pairs_per_s": pairs / (w * 1e-6),
            "index_only_pairs_per_s": pairs / (i * 1e-6), "timescale_pairs_per_s": pairs / (t * 1e-6), "with_count_rounds_us": us["N"],
            "index_only_rounds_us": us["I"], "timescale_rounds_us": us["T"], "passes_per_round": passes}


WHAT = ("us per pass over all 16 members, fp32, radius 0.25; batch: one nbx_ensemble_neighbours / nbx_ragged_neighbours call; "
        "contexts: one nbx_neighbours call on each of 16 default contexts, one per member, created and uploaded beforehand (not "
        "charged for download, create or upload); medians of the rounds, arms alternated, one process; ratio = batch / contexts (gated "
        "<= 1.0 by tests/test_neighbours_gpu.py); context_n131072: one nbx_neighbours call with the count and one without against "
        "one nbx_timescale call on one context of 131072 bodies, where the pair loops are what is timed: with_count_ratio and "
        "index_only_ratio = neighbours / timescale (recorded)")


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
    print("%-10s %10s %12s %8s" % ("kind", "batch us", "contexts us", "ratio"))
    for kind in ("ensemble", "ragged"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-10s %10.1f %12.1f %8.3f%s" % (kind, r["batch_us"], r["contexts_us"], r["ratio"],
                                                "" if r["same_values_from_both_arms"] else "  VALUES DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d: with the count %.1f us (%.3g pair/s, %.2f of timescale), index and r2 only %.1f us (%.3g pair/s, %.2f), "
          "timescale %.1f us (%.3g pair/s)" % (r["n"], r["with_count_us"], r["with_count_pairs_per_s"], r["with_count_ratio"], r["index_only_us"],
                                               r["index_only_pairs_per_s"], r["index_only_ratio"], r["timescale_us"], r["timescale_pairs_per_s"]),
          flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
