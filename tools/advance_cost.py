"""Cost of an adaptive step (include/nbx_advance.h) against the fixed Hermite step it restates, in one process, per step:

  A  advance(t_end, dt_cap, eta, levels=0, max_steps=8, resume=True) and a sync: 24 launches, nothing copied; eta is so large
     that every step is dt_cap, and t_end so far away that no system is ever done
  H  hermite_step(dt_cap, 8, resume=True) and a sync on a second object of the same kind holding the same upload: 16 launches (a
     resumed call of one stepper is refused after a call of the other, so each arm keeps an object of its own)
  E  the same advance call on a third object that has reached its t_end: all 24 launches are empty (recorded, not gated)

Cells: an ensemble of 64 x 256, the ragged ensemble of tools/timescale_cost.py (16 members, 512 ... 4096) and one context of
131072 bodies, fp32.  The states and the timing loop are those of tools/binaries_cost.py (its member_state and _time are used as
they are: warm-up by calibration, the arms alternated, rounds of at least `window` seconds).  ratio = best A / best H over the
rounds; tests/test_advance_gpu.py gates the ensemble's at <= 2.0: three launches against two where the step is launch-bound,
the rest for the candidate write and timer noise.  Near 1.0 is expected at n = 131072, where the pair loop is what is timed.

usage: python tools/advance_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/advance_cost.json, fp32."""
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

OUT = os.path.join(ROOT, "profiles", "advance_cost.json")
STEPS, DT_CAP, ETA, LARGE_N = 8, 2.0 ** -17, 2.0 ** 20, 131072
FAR = DT_CAP * 2.0 ** 50  # a t_end no run here reaches: with levels = 0 it is 2^50 steps away
ENSEMBLE = (64, 256)      # members, n


def _objects(nbx, kind, precision, count):
    """(`count` objects of the kind holding one upload, the sizes of their systems)."""
    dtype = np.float32 if precision == 32 else np.float64
    if kind == "context":
        state = BC.member_state(LARGE_N, 999, dtype)
        objs = [nbx.Context(LARGE_N, precision) for _ in range(count)]
        for o in objs:
            o.upload(state)
        return objs, [LARGE_N]
    sizes = [ENSEMBLE[1]] * ENSEMBLE[0] if kind == "ensemble" else list(TC.RAGGED_SIZES)
    states = [BC.member_state(n, 1000 + k, dtype) for k, n in enumerate(sizes)]
    state = {f: np.stack([s[f] for s in states]) for f in states[0]} if kind == "ensemble" else H.joined(states)
    objs = [nbx.Ensemble(ENSEMBLE[1], ENSEMBLE[0], precision) if kind == "ensemble" else nbx.Ragged(sizes, precision) for _ in range(count)]
    for o in objs:
        H.device_upload(o, state)
    return objs, sizes


def _downloaded(obj):
    """download() in the form hermite_ref holds a state in."""
    d = obj.download()
    return {f: np.concatenate([m[f] for m in d]) for f in H.POS + H.VEL} if isinstance(d, list) else d


def _clocks(obj):
    c = obj.clock()
    return c if isinstance(c, list) else [c]


def measure(nbx, kind, precision=32, rounds=5, window=0.05):
    """One cell, kind "ensemble", "ragged" or "context".  us per step of each arm: the best and the median of the rounds."""
    assert rounds >= 5
    objs, sizes = _objects(nbx, kind, precision, 3)
    adaptive, fixed, ended = objs
    try:
        adaptive.advance(FAR, DT_CAP, ETA, 0, STEPS)
        fixed.hermite_step(DT_CAP, STEPS)
        same = H.same(_downloaded(adaptive), _downloaded(fixed))  # eight steps of dt_cap either way
        ended.advance(DT_CAP, DT_CAP, ETA, 0, STEPS)  # one step, and every system is done
        all_done = all(c["done"] and c["steps"] == 1 for c in _clocks(ended))

        def arm_a():
            adaptive.advance(FAR, DT_CAP, ETA, 0, STEPS, resume=True)
            adaptive.sync()

        def arm_h():
            fixed.hermite_step(DT_CAP, STEPS, resume=True)
            fixed.sync()

        def arm_e():
            ended.advance(DT_CAP, DT_CAP, ETA, 0, STEPS, resume=True)
            ended.sync()

        us, passes = BC._time({"A": arm_a, "H": arm_h, "E": arm_e}, rounds, window)
        every_step_is_dt_cap = all(c["dt_last"] == DT_CAP and c["dt_next"] == DT_CAP and not c["done"] for c in _clocks(adaptive))
        still_one_step = all(c["steps"] == 1 for c in _clocks(ended))
    finally:
        for o in objs:
            o.close()
    per_step = {k: [t / STEPS for t in v] for k, v in us.items()}
    best = {k: min(v) for k, v in per_step.items()}
    return {"kind": kind, "systems": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "steps_per_pass": STEPS, "rounds": rounds, "advance_us_per_step": best["A"], "hermite_us_per_step": best["H"],
            "ratio": best["A"] / best["H"], "advance_median_us_per_step": statistics.median(per_step["A"]),
            "hermite_median_us_per_step": statistics.median(per_step["H"]), "finished_us_per_step": best["E"],
            "finished_us_per_launch": best["E"] / 3.0, "advance_rounds_us_per_step": per_step["A"], "hermite_rounds_us_per_step": per_step["H"],
            "finished_rounds_us_per_step": per_step["E"], "passes_per_round": passes, "same_bits_from_both_arms": bool(same),
            "every_step_is_dt_cap": bool(every_step_is_dt_cap), "finished_object_is_done_and_stays": bool(all_done and still_one_step)}


WHAT = ("us per step, fp32, the best of the rounds (medians beside them); advance: advance(max_steps=8, resume=True) and a sync, over 8, "
        "eta so large that every step is dt_cap; hermite: hermite_step(dt_cap, 8, resume=True) and a sync on a second object holding the "
        "same upload, over 8; arms alternated, one process; ratio = advance / hermite (the ensemble's gated <= 2.0 by "
        "tests/test_advance_gpu.py); finished: the same advance call on an object whose systems are all done, 24 empty launches, over 8 "
        "(recorded); cells: an ensemble of 64 x 256, a ragged ensemble of 16 members of 512 ... 4096, one context of 131072")


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds per timed round of an arm")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
    import nbx
    print("%-10s %12s %12s %8s %14s" % ("kind", "advance us", "hermite us", "ratio", "finished us"))
    for kind in ("ensemble", "ragged", "context"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-10s %12.1f %12.1f %8.4f %14.1f%s" % (kind, r["advance_us_per_step"], r["hermite_us_per_step"], r["ratio"], r["finished_us_per_step"],
                                                      "" if r["same_bits_from_both_arms"] else "  BITS DIFFER"), flush=True)
        write(a.out, {kind if kind != "context" else "context_n%d" % LARGE_N: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
