"""Cost of a resident Hermite step (include/nbx_hermite.h) of every member of a batch object, in one process, per step:

  A  hermite_step(dt, 8, resume=True) and a sync: 16 launches, nothing copied
  B  eight steps of the round trip it replaces, carried from step to step (tests/hermite_ref.py round_trip): per step the host
     predictor in numpy, nbx_*_upload of the predicted state, nbx_*_jerk, the host corrector; one more upload at the end
  S  step(8, dt) and a sync on a third object of the same states: the plain step, for scale (recorded, not gated)

A and B start from the same upload and return the same bits (checked once, before the timing).  The cells, the states, the
warm-up and the repetitions are those of tools/binaries_cost.py (its member_state and _time are used as they are).
ratio = A / B, gated <= 1.0 by tests/test_hermite_gpu.py.

One more cell is recorded and not gated.  context_n131072: hermite_step(dt, 1, resume=True) and a sync on one context of 131072
bodies against one whole nbx_jerk call on the same context (its two launches, its read-back and its synchronisation): the pair
loops are what is timed, and they are the same loop.

usage: python tools/hermite_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/hermite_cost.json, fp32."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binaries_cost as BC  # noqa: E402
import hermite_ref as H  # noqa: E402
import timescale_cost as TC  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "hermite_cost.json")
STEPS, DT, LARGE_N = 8, 1e-5, 131072


def _downloaded(obj):
    """download() in the form hermite_ref holds a state in."""
    d = obj.download()
    return {f: np.concatenate([m[f] for m in d]) for f in H.POS + H.VEL} if isinstance(d, list) else d


def measure(nbx, kind, precision=32, rounds=5, window=0.05):
    """One cell, kind "ensemble" or "ragged".  Median us per step of each arm, ratio = A / B."""
    assert rounds >= 5
    sizes = [TC.ENSEMBLE_N] * TC.MEMBERS if kind == "ensemble" else list(TC.RAGGED_SIZES)
    dtype = np.float32 if precision == 32 else np.float64
    states = [BC.member_state(n, 1000 + k, dtype) for k, n in enumerate(sizes)]
    state = {f: np.stack([s[f] for s in states]) for f in states[0]} if kind == "ensemble" else H.joined(states)
    objs = [nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision) for _ in range(3)]
    resident, trip, plain = objs
    try:
        for o in objs:
            H.device_upload(o, state)
        resident.hermite_step(DT, STEPS)
        carried = list(H.round_trip(trip, state, DT, STEPS))
        same = H.same(_downloaded(resident), carried[0]) and H.same(_downloaded(trip), carried[0])

        def arm_a():
            resident.hermite_step(DT, STEPS, resume=True)
            resident.sync()

        def arm_b():
            carried[:] = H.round_trip(trip, carried[0], DT, STEPS, carried[1])

        def arm_s():
            plain.step(STEPS, DT, kenergy=False)
            plain.sync()

        us, passes = BC._time({"A": arm_a, "B": arm_b, "S": arm_s}, rounds, window)
    finally:
        for o in objs:
            o.close()
    per_step = {k: [t / STEPS for t in v] for k, v in us.items()}
    a, b, s = (statistics.median(per_step[k]) for k in "ABS")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "steps_per_pass": STEPS, "resident_us_per_step": a, "round_trip_us_per_step": b, "ratio": a / b, "plain_step_us_per_step": s,
            "resident_over_plain_step": a / s, "resident_rounds_us_per_step": per_step["A"], "round_trip_rounds_us_per_step": per_step["B"],
            "plain_step_rounds_us_per_step": per_step["S"], "passes_per_round": passes, "same_bits_from_both_arms": bool(same)}


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, one resumed resident step and a sync against one whole jerk call."""
    assert rounds >= 5
    c = nbx.Context(n, precision)
    try:
        c.upload(BC.member_state(n, 999, np.float32 if precision == 32 else np.float64))
        c.hermite_step(DT, 1)

        def arm_h():
            c.hermite_step(DT, 1, resume=True)
            c.sync()

        us, passes = BC._time({"H": arm_h, "J": c.jerk}, rounds, window)
    finally:
        c.close()
    h, j = (statistics.median(us[k]) for k in "HJ")
    pairs = float(n) * n
    return {"kind": "context", "n": n, "precision": precision, "hermite_step_us": h, "jerk_call_us": j, "hermite_step_over_jerk_call": h / j,
            "hermite_pairs_per_s": pairs / (h * 1e-6), "jerk_pairs_per_s": pairs / (j * 1e-6), "hermite_step_rounds_us": us["H"],
            "jerk_call_rounds_us": us["J"], "passes_per_round": passes}


WHAT = ("us per step, fp32; ensemble / ragged: over all 16 members; resident: hermite_step(dt, 8, resume=True) and a sync, over 8; "
        "round_trip: eight carried steps of the round trip of public calls it replaces -- per step the host predictor (numpy), "
        "nbx_*_upload, nbx_*_jerk, the host corrector, and one upload at the end -- over 8; medians of the rounds, arms alternated, one "
        "process; ratio = resident / round_trip (gated <= 1.0 by tests/test_hermite_gpu.py); plain_step: step(8, dt) and a sync on "
        "a third object, over 8 (recorded); context_n131072: one resumed resident step and a sync against one whole nbx_jerk call on "
        "the same context, where the pair loops are what is timed (recorded)")


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
    print("%-10s %12s %14s %8s %12s" % ("kind", "resident us", "round trip us", "ratio", "plain step us"))
    for kind in ("ensemble", "ragged"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-10s %12.1f %14.1f %8.4f %12.1f%s" % (kind, r["resident_us_per_step"], r["round_trip_us_per_step"], r["ratio"],
                                                      r["plain_step_us_per_step"], "" if r["same_bits_from_both_arms"] else "  BITS DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d: resident step %.1f us (%.3g pair/s), jerk call %.1f us (%.3g pair/s), ratio %.3f" % (
        r["n"], r["hermite_step_us"], r["hermite_pairs_per_s"], r["jerk_call_us"], r["jerk_pairs_per_s"], r["hermite_step_over_jerk_call"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
