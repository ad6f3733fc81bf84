"""Cost of the diagnostics of every member of a ragged ensemble, two ways, in one process:

  A  one nbx_ragged_diagnostics call over all M members (one pair-work launch, one reduce launch, one read-back)
  B  M nbx_diagnostics calls on M default contexts, one per member and of its size, that were created and uploaded beforehand
     and hold the same states (two launches and a synchronising read-back each)

B is the most favourable alternative without nbx_ragged_diagnostics: it is not charged for downloading the members or for
creating and uploading the contexts, which a user without the call would pay as well.  Both arms go through the Python binding
and return the same list of dicts (checked).  Per cell: a warm-up of both arms, then `rounds` rounds, A and B alternated; a
round times `passes` back-to-back passes of an arm (each pass ends in a synchronisation) so that it lasts >= `window` seconds;
the figures are medians over the rounds, in us per pass.  ratio = A / B.

usage: python tools/ragged_diag_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/ragged_diag_cost.json: the four populations of scripts/ragged_sweep.py, fp32."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ragged_diag_cost.json")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from ragged_sweep import POPULATIONS, member_states  # noqa: E402  (the populations and states of the step's sweep, not restated)

GATE_POPULATION = "64 sizes spread evenly over 512 ... 4096"  # the cell tests/test_ragged_diag_gpu.py gates


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


def measure(nbx, sizes, precision=32, rounds=5, window=0.05, population=None):
    """One cell.  {'ragged_us', 'contexts_us', 'ratio', ...}: median time of one pass of each arm and A / B."""
    assert rounds >= 5
    sizes = [int(n) for n in sizes]
    states = member_states(nbx, sizes, precision)
    rag = nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        rag.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arm_a = rag.diagnostics
        arm_b = lambda: [c.diagnostics() for c in ctxs]  # noqa: E731
        same = arm_a() == arm_b()
        arms = {"A": arm_a, "B": arm_b}
        passes = {k: _passes_for(run, window) for k, run in arms.items()}
        us = {k: [] for k in arms}
        for _ in range(rounds):
            for k, run in arms.items():  # A B A B ...
                t0 = time.perf_counter()
                for _ in range(passes[k]):
                    run()
                us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
    finally:
        for o in [rag] + ctxs:
            o.close()
    a, b = statistics.median(us["A"]), statistics.median(us["B"])
    return {"population": population, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes),
            "precision": precision, "ragged_us": a, "contexts_us": b, "ratio": a / b, "ragged_rounds_us": us["A"],
            "contexts_rounds_us": us["B"], "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def measure_gate(nbx, rounds=5, window=0.05):
    return measure(nbx, POPULATIONS[GATE_POPULATION], 32, rounds, window, population=GATE_POPULATION)


WHAT = ("us per pass over all members, fp32 unless a cell says otherwise; ragged: one nbx_ragged_diagnostics call; contexts: one "
        "nbx_diagnostics call on each of M default contexts, one per member, created and uploaded beforehand (not charged for "
        "download, create or upload); medians of the rounds, arms alternated, one process; ratio = ragged / contexts")


def write(path, cells=None, gate=None):
    """Merge `cells` (the sweep) and / or `gate` (the cell tests/test_ragged_diag_gpu.py measures) into the JSON file."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out["what"] = WHAT
    if cells is not None:
        out["cells"] = cells
    if gate is not None:
        out["gate_cell_of_the_test_suite"] = gate
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
    print("%-42s %12s %12s %8s" % ("population", "ragged us", "contexts us", "ratio"))
    for name, sizes in POPULATIONS.items():
        r = measure(nbx, sizes, rounds=a.rounds, window=a.window, population=name)
        cells.append(r)
        print("%-42s %12.1f %12.1f %8.3f%s" % (name, r["ragged_us"], r["contexts_us"], r["ratio"],
                                                "" if r["same_values_from_both_arms"] else "  VALUES DIFFER"), flush=True)
        write(a.out, cells=cells)  # after every cell: a partial sweep is still a record
    print("wrote", a.out)


if __name__ == "__main__":
    main()
