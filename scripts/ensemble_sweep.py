#!/usr/bin/env python3
"""Ensemble against today's best for many small systems, in one process: time per ensemble step (one step of all S members).

  A  ensemble:               nbx.Ensemble.step(k, kenergy=False), then sync
  B  contexts, sequential:   S nbx.Context objects with default options (jlane auto, graph replay as the planner decides),
                             step(k, kenergy=False) on each in turn, then sync on each
  C  contexts, concurrent:   the same S contexts, their step calls issued round-robin in chunks of 50 steps (one graph replay
                             each; every context has its own non-blocking stream), then sync on all
  A with every explicit bodies_per_lane, to check the planner's choice.

Per cell: a warm-up window of every leg, then the legs alternated (A B C A B C ...) for --repeats windows each; k steps per
window so that a window lasts >= --window seconds.  Writes one JSON file (default profiles/ensemble_sweep.json): medians and
min/max in us per ensemble step, aggregate pair/s, the share of the fp32 (fp64) vector roofline at 20 flop per pair as a
WHOLE-LAUNCH figure (launch gaps and the epilogue included), ratio = min(B, C) / A, the NB taken and the NB that measured
fastest.

  python3 scripts/ensemble_sweep.py [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
import nbx  # noqa: E402

ROOFLINE = {32: 157.3e12, 64: 78.6e12}  # flop/s, vector pipe (README)
RECORDED_S1_US = {2048: 5.8, 4096: 8.7, 8192: 20.0}  # profiles/r04_sweep_multi_gpu_proxy.txt: one context, us per step
CHUNK = 50  # steps per step() call of leg C = the longest window a context replays from one graph


def member_states(n, S, precision):
    big = nbx.initial_conditions(S * n, precision)
    states = [{f: big[f][m * n:(m + 1) * n].copy() for f in nbx.FIELDS} for m in range(S)]
    states[-1] = nbx.initial_conditions(n, precision)
    return states


def leg_ensemble(e):
    def run(k):
        t = time.perf_counter()
        e.step(k, kenergy=False)
        e.sync()
        return time.perf_counter() - t
    return run


def leg_sequential(ctxs):
    def run(k):
        t = time.perf_counter()
        for c in ctxs:
            c.step(k, kenergy=False)
        for c in ctxs:
            c.sync()
        return time.perf_counter() - t
    return run


def leg_concurrent(ctxs):
    def run(k):
        t = time.perf_counter()
        for _ in range(k // CHUNK):
            for c in ctxs:
                c.step(CHUNK, kenergy=False)
        for c in ctxs:
            c.sync()
        return time.perf_counter() - t
    return run


def steps_for(run, window):
    """k (a multiple of CHUNK) such that run(k) lasts >= window seconds; the calibration runs double as warm-up."""
    k = 2 * CHUNK
    run(k)
    while True:
        t = run(k)
        if t >= window or k >= 1 << 22:
            return k
        k = max(2 * k, int(k * window / max(t, 1e-6) * 1.2)) // CHUNK * CHUNK + CHUNK


def summary(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "windows_us": us}


def measure_cell(n, S, precision, window, repeats):
    states = member_states(n, S, precision)
    nbs = (2, 4, 8, 16) if precision == 32 else (2, 4, 8)
    ens = nbx.Ensemble(n, S, precision)
    ens.upload(states)
    variants = {nb: nbx.Ensemble(n, S, precision, bodies_per_lane=nb) for nb in nbs}
    for v in variants.values():
        v.upload(states)
    ctxs = [nbx.Context(n, precision) for _ in range(S)]
    for c, s in zip(ctxs, states):
        c.upload(s)
    try:
        legs = {"A": leg_ensemble(ens), "B": leg_sequential(ctxs), "C": leg_concurrent(ctxs)}
        legs.update({"A_nb%d" % nb: leg_ensemble(v) for nb, v in variants.items()})
        ks = {name: steps_for(run, window) for name, run in legs.items()}
        for name, run in legs.items():  # the warm-up window of every leg at its own k
            run(ks[name])
        us = {name: [] for name in legs}
        for _ in range(repeats):
            for name, run in legs.items():  # A B C A_nb2 ... A B C ...
                us[name].append(run(ks[name]) / ks[name] * 1e6)
        est, cst = ens.stats(), ctxs[0].stats()
    finally:
        for o in [ens] + list(variants.values()) + ctxs:
            o.close()
    res = {name: summary(v) for name, v in us.items()}
    a = res["A"]
    other = min(("B", "C"), key=lambda x: res[x]["median_us"])
    o = res[other]
    spread = max(a["max_us"] - a["min_us"], o["max_us"] - o["min_us"])
    per_nb = {nb: res["A_nb%d" % nb]["median_us"] for nb in nbs}
    pairs = float(S) * n * n
    cell = {
        "n": n, "members": S, "precision": precision, "steps_per_window": ks,
        "A": a, "B": res["B"], "C": res["C"],
        "pairs_per_s": pairs / (a["median_us"] * 1e-6),
        "roofline_share_whole_launch": pairs * 20 / (a["median_us"] * 1e-6) / ROOFLINE[precision],
        "ratio_min_BC_over_A": o["median_us"] / a["median_us"], "best_of_today": other,
        "A_below_best_of_today_by_more_than_the_spread": a["median_us"] < o["median_us"] - spread,
        "nb_taken": est["bodies_per_lane"], "inner_loop_taken": est["inner_loop"], "grid": [est["grid_x"], est["grid_y"]],
        "A_by_nb_median_us": per_nb, "A_by_nb": {nb: res["A_nb%d" % nb] for nb in nbs},
        "nb_fastest": min(per_nb, key=per_nb.get),
        "context_plan": {k: cst[k] for k in ("kernel_variant", "bodies_per_lane", "inner_loop", "use_graph", "force_grid_x")},
    }
    if S == 1 and precision == 32 and n in RECORDED_S1_US:
        cell["B_over_recorded_single_context"] = res["B"]["median_us"] / RECORDED_S1_US[n]
    return cell, cst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_sweep.json"))
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="two small cells only (a rehearsal of the script)")
    a = ap.parse_args()
    cells = [(n, S, 32) for n in (2048, 4096, 8192) for S in (1, 4, 16, 64)] + [(2048, S, 64) for S in (4, 64)]
    if a.quick:
        cells = [(2048, 4, 32), (2048, 4, 64)]
    out = {"what": "us per ensemble step (one step of all members); A ensemble, B contexts one after the other, C contexts round-robin in "
                   "chunks of %d steps; medians of %d windows of >= %.2f s, legs alternated, one process" % (CHUNK, a.repeats, a.window),
           "roofline_flops": ROOFLINE, "flop_per_pair": 20, "cells": []}
    for n, S, precision in cells:
        cell, cst = measure_cell(n, S, precision, a.window, a.repeats)
        out.setdefault("device", {"name": cst["device_name"], "clock_mhz": cst["clock_mhz"], "cu_count": cst["cu_count"]})
        out["cells"].append(cell)
        print("fp%d n %5d S %3d: A %9.2f us  B %9.2f  C %9.2f  ratio %5.2f  NB taken %d fastest %d %s  %.1f %% of the roofline" % (
            precision, n, S, cell["A"]["median_us"], cell["B"]["median_us"], cell["C"]["median_us"], cell["ratio_min_BC_over_A"],
            cell["nb_taken"], cell["nb_fastest"], json.dumps(cell["A_by_nb_median_us"]), 100 * cell["roofline_share_whole_launch"]), flush=True)
        with open(a.out, "w") as f:  # after every cell: a partial sweep is still a record
            json.dump(out, f, indent=1)
    drift = [c["B_over_recorded_single_context"] for c in out["cells"] if "B_over_recorded_single_context" in c]
    out["single_context_vs_recorded"] = {"ratios": drift, "recorded_us": RECORDED_S1_US,
                                         "beyond_the_10_percent_the_pool_spreads": any(abs(r - 1.0) > 0.10 for r in drift)}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
