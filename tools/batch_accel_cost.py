"""Cost of the accelerations of every member of an ensemble or a ragged ensemble, two ways, in one process:

  A  one nbx_ensemble_accel / nbx_ragged_accel call over all M members (one launch, one read-back, one synchronisation)
  B  M nbx_accel calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and
     hold the same states (a launch, a read-back and a synchronisation each)

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts, which a user without the call would pay as well, and every context runs the shape the planner takes for
a lone system of its size.  Both arms go through the Python binding and return host arrays of the same bodies; they agree to
rounding (checked; a member sums in the order of the batch's bodies per wave, a default context in the order of its own).  Per
cell: a warm-up of both arms, then `rounds` rounds, A and B alternated; a round times `passes` back-to-back passes of an arm
(each pass ends in a synchronisation) so that it lasts >= `window` seconds; the figures are medians over the rounds, in us per
pass.  ratio = A / B.

usage: python tools/batch_accel_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/batch_accel_cost.json: ensembles of 4, 16 and 64 x 2048 and 16 x 8192, and the ragged population "64 sizes spread
evenly over 512 ... 4096" of scripts/ragged_sweep.py, fp32."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "batch_accel_cost.json")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from ragged_sweep import POPULATIONS, member_states  # noqa: E402  (the populations and states of the step's sweep, not restated)

ENSEMBLE_CELLS = [(4, 2048), (16, 2048), (64, 2048), (16, 8192)]  # members x n
RAGGED_POPULATION = "64 sizes spread evenly over 512 ... 4096"
GATE_ENSEMBLE = (16, 2048)                                                  # the cells tests/test_batch_accel_gpu.py gates
GATE_RAGGED = [512 + round(k * (4096 - 512) / 15) for k in range(16)]       # 16 members spread evenly over 512 ... 4096


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


def _worst_difference(batch, ctxs):
    """max over members of |batch - context|inf / |context|inf, both arms' arrays as lists of [ax, ay, az] per member."""
    worst = 0.0
    for a, b in zip(batch, ctxs):
        a, b = np.stack(a).astype(np.float64), np.stack(b).astype(np.float64)
        worst = max(worst, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)))
    return worst


def measure(nbx, sizes, precision=32, rounds=5, window=0.05, ensemble=False, population=None):
    """One cell: `sizes` as an ensemble (all equal) or as a ragged ensemble.  {'batch_us', 'contexts_us', 'ratio', ...}: median time
    of one pass of each arm and A / B."""
    assert rounds >= 5
    sizes = [int(n) for n in sizes]
    states = member_states(nbx, sizes, precision)
    if ensemble:
        assert len(set(sizes)) == 1
        batch = nbx.Ensemble(sizes[0], len(sizes), precision)
    else:
        batch = nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arm_a = batch.accel
        arm_b = lambda: [c.accel() for c in ctxs]  # noqa: E731
        got = arm_a()
        if ensemble:
            got = [[a[m] for a in got] for m in range(len(sizes))]
        diff = _worst_difference(got, arm_b())
        arms = {"A": arm_a, "B": arm_b}
        passes = {k: _passes_for(run, window) for k, run in arms.items()}
        us = {k: [] for k in arms}
        for _ in range(rounds):
            for k, run in arms.items():  # A B A B ...
                t0 = time.perf_counter()
                for _ in range(passes[k]):
                    run()
                us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
        st = batch.stats()
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b = statistics.median(us["A"]), statistics.median(us["B"])
    return {"kind": "ensemble" if ensemble else "ragged", "population": population, "members": len(sizes), "n_min": min(sizes),
            "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision, "bodies_per_lane": st["bodies_per_lane"],
            "inner_loop": st["inner_loop"], "batch_us": a, "contexts_us": b, "ratio": a / b, "batch_rounds_us": us["A"],
            "contexts_rounds_us": us["B"], "passes_per_round": passes, "worst_relative_difference_of_the_arms": diff,
            "arms_agree_to_rounding": bool(diff <= (1e-4 if precision == 32 else 1e-12))}


def measure_gate_ensemble(nbx, rounds=5, window=0.05):
    S, n = GATE_ENSEMBLE
    return measure(nbx, [n] * S, 32, rounds, window, ensemble=True, population="%d x %d" % (S, n))


def measure_gate_ragged(nbx, rounds=5, window=0.05):
    return measure(nbx, GATE_RAGGED, 32, rounds, window, population="16 sizes spread evenly over 512 ... 4096")


WHAT = ("us per pass over all members, fp32; batch: one nbx_ensemble_accel / nbx_ragged_accel call; contexts: one nbx_accel call on each "
        "of M default contexts, one per member, created and uploaded beforehand (not charged for download, create or upload); medians "
        "of the rounds, arms alternated, one process; ratio = batch / contexts")


def write(path, cells=None, **gates):
    """Merge `cells` (the sweep) and / or the cells tests/test_batch_accel_gpu.py measures (gate_ensemble=, gate_ragged=) into the JSON file."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out["what"] = WHAT
    if cells is not None:
        out["cells"] = cells
    for k, v in gates.items():
        out[k + "_cell_of_the_test_suite"] = v
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
    cells = []
    todo = [("%d x %d" % (S, n), [n] * S, True) for S, n in ENSEMBLE_CELLS] + [(RAGGED_POPULATION, POPULATIONS[RAGGED_POPULATION], False)]
    print("%-42s %12s %12s %8s" % ("population", "batch us", "contexts us", "ratio"))
    for name, sizes, ensemble in todo:
        r = measure(nbx, sizes, rounds=a.rounds, window=a.window, ensemble=ensemble, population=name)
        cells.append(r)
        print("%-42s %12.1f %12.1f %8.3f%s" % (name, r["batch_us"], r["contexts_us"], r["ratio"],
                                                "" if r["arms_agree_to_rounding"] else "  VALUES DIFFER"), flush=True)
        write(a.out, cells=cells)  # after every cell: a partial sweep is still a record
    print("wrote", a.out)


if __name__ == "__main__":
    main()
