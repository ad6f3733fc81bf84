#!/usr/bin/env python3
"""A ragged ensemble (members of different size, one launch per step) against today's best for the same systems, in one
process: time per step of ALL members, in us.

  R       ragged:               nbx.Ragged.step(k, kenergy=False), then sync -- with the planner's bodies per wave, and
  R_nb*                         with every other legal bodies_per_lane, to argue the planner's choice from numbers
  B       contexts, sequential: one nbx.Context per member with default options (jlane auto, graph replay as the planner decides,
                                a non-blocking stream each), step(k, kenergy=False) on each in turn, then sync on each
  C       contexts, concurrent: the same contexts, their step calls issued round-robin in chunks of 50 steps, then sync on all
  G       ensembles by size:    one nbx.Ensemble per distinct size that repeats, one context per size that does not, stepped
                                round-robin in chunks of 50 steps (only where a size repeats; for the uniform population this is
                                nbx_ensemble itself)

Populations (fp32): uniform 64 x 2048; 32 x 2048 + 32 x 1024; 64 sizes spread evenly over 512 ... 4096; 4 x 8192 + 60 x 1024.
Per population: a calibration that doubles as warm-up and one warm-up window of every leg, then the legs alternated
(R B C G R_nb2 ... R B C ...) for --repeats windows each; k steps per window so that a window lasts >= --window seconds.
Medians, min and max (the spread) of the windows are recorded; ratio = min(B, C, G) / R.

  python3 scripts/ragged_sweep.py [--out FILE] [--quick]      (on the device, from the repository root)

Writes profiles/ragged_sweep.json under "cells"; tests/test_ragged_gpu.py writes its cost gate into the same file under "gate"."""
import argparse
import json
import os
import statistics
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ragged_sweep.json")
ROOFLINE = {32: 157.3e12, 64: 78.6e12}  # flop/s, vector pipe (README)
CHUNK = 50  # steps per step() call of the round-robin legs = the longest window a context replays from one graph

POPULATIONS = {
    "uniform 64 x 2048": [2048] * 64,
    "32 x 2048 + 32 x 1024": [2048] * 32 + [1024] * 32,
    "64 sizes spread evenly over 512 ... 4096": [512 + round(k * (4096 - 512) / 63) for k in range(64)],
    "4 x 8192 + 60 x 1024": [8192] * 4 + [1024] * 60,
}


def member_states(nbx, sizes, precision):
    """As tests/test_ragged_gpu.member_states: consecutive slices of one seed-42 system; the last member is the seed-42 system of its size."""
    big = nbx.initial_conditions(sum(sizes), precision)
    at = [0]
    for n in sizes:
        at.append(at[-1] + n)
    states = [{f: big[f][at[k]:at[k + 1]].copy() for f in nbx.FIELDS} for k in range(len(sizes))]
    states[-1] = nbx.initial_conditions(sizes[-1], precision)
    return states


def leg_one(obj):
    def run(k):
        t = time.perf_counter()
        obj.step(k, kenergy=False)
        obj.sync()
        return time.perf_counter() - t
    return run


def leg_sequential(objs):
    def run(k):
        t = time.perf_counter()
        for o in objs:
            o.step(k, kenergy=False)
        for o in objs:
            o.sync()
        return time.perf_counter() - t
    return run


def leg_round_robin(objs):
    def run(k):
        t = time.perf_counter()
        for _ in range(k // CHUNK):
            for o in objs:
                o.step(CHUNK, kenergy=False)
        for o in objs:
            o.sync()
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


def measure(nbx, sizes, precision=32, window=0.2, repeats=5, every_nb=True, by_size=True):
    """One population.  Returns the cell that goes into the JSON file."""
    states = member_states(nbx, sizes, precision)
    objs = []  # everything to close
    try:
        rag = nbx.Ragged(sizes, precision)
        objs.append(rag)
        rag.upload(states)
        rst = rag.stats()
        legs = {"R": leg_one(rag)}
        ctxs = []
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            objs.append(ctxs[-1])
            ctxs[-1].upload(s)
        legs["B"], legs["C"] = leg_sequential(ctxs), leg_round_robin(ctxs)
        count = Counter(sizes)
        groups = None
        if by_size and any(c > 1 for c in count.values()):
            groups = []
            for n, c in sorted(count.items(), reverse=True):
                mine = [s for m, s in zip(sizes, states) if m == n]
                if c > 1:
                    groups.append(nbx.Ensemble(n, c, precision))
                    groups[-1].upload(mine)
                else:
                    groups.append(nbx.Context(n, precision))
                    groups[-1].upload(mine[0])
                objs.append(groups[-1])
            legs["G"] = leg_round_robin(groups)
        nbs = ((2, 4, 8, 16) if precision == 32 else (2, 4, 8)) if every_nb else ()
        for nb in nbs:
            v = nbx.Ragged(sizes, precision, bodies_per_lane=nb)
            objs.append(v)
            v.upload(states)
            legs["R_nb%d" % nb] = leg_one(v)
        ks = {name: steps_for(run, window) for name, run in legs.items()}
        for name, run in legs.items():  # the warm-up window of every leg at its own k
            run(ks[name])
        us = {name: [] for name in legs}
        for _ in range(repeats):
            for name, run in legs.items():
                us[name].append(run(ks[name]) / ks[name] * 1e6)
        cst = ctxs[-1].stats()
    finally:
        for o in objs:
            o.close()
    res = {name: summary(v) for name, v in us.items()}
    r = res["R"]
    other = min((x for x in ("B", "C", "G") if x in res), key=lambda x: res[x]["median_us"])
    o = res[other]
    spread = max(r["max_us"] - r["min_us"], o["max_us"] - o["min_us"])
    pairs = rst["pairs_per_step"]
    cell = {
        "sizes": {str(n): c for n, c in sorted(count.items())}, "members": len(sizes), "bodies_total": rst["bodies_total"], "precision": precision,
        "pairs_per_step": pairs, "steps_per_window": ks,
        "R": r, "B": res["B"], "C": res["C"], "G": res.get("G"),
        "G_is": None if groups is None else ("nbx_ensemble itself" if len(count) == 1 else "one nbx_ensemble per repeating size, one context per single size"),
        "pairs_per_s": pairs / (r["median_us"] * 1e-6),
        "roofline_share_whole_launch": pairs * 20 / (r["median_us"] * 1e-6) / ROOFLINE[precision],
        "best_of_today": other, "ratio_best_of_today_over_R": o["median_us"] / r["median_us"],
        "R_below_best_of_today_by_more_than_the_spread": r["median_us"] < o["median_us"] - spread,
        "nb_taken": rst["bodies_per_lane"], "inner_loop_taken": rst["inner_loop"], "grid_x": rst["grid_x"],
        "device": {"name": cst["device_name"], "clock_mhz": cst["clock_mhz"], "cu_count": cst["cu_count"]},
    }
    if nbs:
        per_nb = {nb: res["R_nb%d" % nb]["median_us"] for nb in nbs}
        cell.update({"R_by_nb_median_us": per_nb, "R_by_nb": {nb: res["R_nb%d" % nb] for nb in nbs}, "nb_fastest": min(per_nb, key=per_nb.get)})
    return cell


def measure_gate(nbx, window=0.1, repeats=5):
    """The cell tests/test_ragged_gpu.py gates: uniform 64 x 2048 fp32, one ragged step of all members against the 64 contexts on
    their own streams with graph replay (the better of the sequential and the round-robin way of driving them)."""
    cell = measure(nbx, POPULATIONS["uniform 64 x 2048"], 32, window, repeats, every_nb=False, by_size=False)
    contexts = min(cell["B"]["median_us"], cell["C"]["median_us"])
    return {"population": "uniform 64 x 2048", "precision": 32, "ragged_us": cell["R"]["median_us"], "contexts_sequential_us": cell["B"]["median_us"],
            "contexts_round_robin_us": cell["C"]["median_us"], "ratio_ragged_over_contexts": cell["R"]["median_us"] / contexts,
            "ragged_windows_us": cell["R"]["windows_us"], "contexts_sequential_windows_us": cell["B"]["windows_us"],
            "contexts_round_robin_windows_us": cell["C"]["windows_us"], "steps_per_window": cell["steps_per_window"],
            "nb_taken": cell["nb_taken"], "inner_loop_taken": cell["inner_loop_taken"], "grid_x": cell["grid_x"], "device": cell["device"]}


WHAT = ("us per step of all members, fp32; R one nbx_ragged launch, B one context per member stepped one after the other, C the same "
        "contexts round-robin in chunks of %d steps, G one nbx_ensemble per repeating size; medians of the windows, legs alternated, one "
        "process; ratio = min(B, C, G) / R; the roofline share is a whole-launch figure at 20 flop per pair" % CHUNK)


def write(path, cells=None, gate=None):
    """Merge `cells` (the sweep) and / or `gate` (the cell tests/test_ragged_gpu.py measures) into the JSON file."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out["what"] = WHAT
    out["roofline_flops"] = ROOFLINE
    if cells is not None:
        out["cells"] = cells
    if gate is not None:
        out["gate"] = gate
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one small mixed population only (a rehearsal of the script)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
    import nbx
    pops = {"quick: 300, 1000, 300, 2048": [300, 1000, 300, 2048]} if a.quick else POPULATIONS
    cells = {}
    for name, sizes in pops.items():
        cell = measure(nbx, sizes, 32, a.window, a.repeats)
        cells[name] = cell
        print("%-42s R %9.2f us  B %9.2f  C %9.2f  G %s  ratio %5.2f (%s)  NB taken %d fastest %d %s  %.1f %% of the roofline" % (
            name, cell["R"]["median_us"], cell["B"]["median_us"], cell["C"]["median_us"],
            "%9.2f" % cell["G"]["median_us"] if cell["G"] else "        -", cell["ratio_best_of_today_over_R"], cell["best_of_today"],
            cell["nb_taken"], cell["nb_fastest"], json.dumps(cell["R_by_nb_median_us"]), 100 * cell["roofline_share_whole_launch"]), flush=True)
        write(a.out, cells=cells)  # after every population: a partial sweep is still a record
    print("wrote", a.out)


if __name__ == "__main__":
    main()
