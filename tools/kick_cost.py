"""Cost of a velocity-only half step of every member of an ensemble or a ragged ensemble (include/nbx_kick.h), in one process:

  A  one nbx_ensemble_kick / nbx_ragged_kick call (one launch, nothing read back) and the synchronisation that ends the pass
  B  what a caller does without it: the accelerations of all members (one nbx_*_accel call), a download of all members, the
     update v += a * h on the host in numpy, and an upload of all members -- three synchronisations and two copies each way
  C  one step launch of the same object (step(1) without the energy) and the synchronisation that ends the pass

B is the most favourable form of the alternative: the batch accel call instead of one context per member, and numpy's vectorised
update.  Arms A and B leave the same velocities to rounding (checked once: B multiplies and adds in numpy, as the kick does on the
device).  Per cell: a warm-up of the arms, then `rounds` rounds, A, B and C alternated; a round times `passes` back-to-back passes
of an arm so that it lasts >= `window` seconds; the figures are medians over the rounds, in us per pass.  The kick size
alternates in sign from pass to pass, so that the velocities stay where they are.
  ratio = A / B          gated at <= 1.0 by tests/test_kick_gpu.py
  kick_to_step = A / C   recorded, not gated

usage: python tools/kick_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/kick_cost.json: 16 x 2048 as an ensemble and 16 sizes spread evenly over 512 ... 4096 as a ragged ensemble, fp32."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "kick_cost.json")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from ragged_sweep import member_states  # noqa: E402  (the states of the step's sweep, not restated)

GATE_ENSEMBLE = (16, 2048)
GATE_RAGGED = [512 + round(k * (4096 - 512) / 15) for k in range(16)]  # 16 members spread evenly over 512 ... 4096
VEL = ("vel_x", "vel_y", "vel_z")
H = 1.0 / 128


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


def _velocities(batch, ensemble):
    d = batch.download()
    return [np.concatenate([np.ravel(d[f]) for f in VEL])] if ensemble else [np.concatenate([m[f] for f in VEL]) for m in d]


def measure(nbx, sizes, precision=32, rounds=5, window=0.05, ensemble=False, population=None):
    """One cell: `sizes` as an ensemble (all equal) or as a ragged ensemble."""
    assert rounds >= 5
    sizes = [int(n) for n in sizes]
    states = member_states(nbx, sizes, precision)
    masses = [s["mass"] for s in states]
    if ensemble:
        assert len(set(sizes)) == 1
        make = lambda: nbx.Ensemble(sizes[0], len(sizes), precision)  # noqa: E731
    else:
        make = lambda: nbx.Ragged(sizes, precision)  # noqa: E731
    T = states[0]["mass"].dtype.type
    sign = {"A": 1.0, "B": 1.0}

    def host_kick(batch, h):
        acc = batch.accel()
        d = batch.download()
        if ensemble:
            for f, a in zip(VEL, acc):
                d[f] = d[f] + a * T(h)
            d["mass"] = np.stack(masses)
            batch.upload(d)
        else:
            for m, a in zip(d, acc):
                for f, c in zip(VEL, a):
                    m[f] = m[f] + c * T(h)
            for m, mass in zip(d, masses):
                m["mass"] = mass
            batch.upload(d)

    a_obj, b_obj = make(), make()
    try:
        for o in (a_obj, b_obj):
            o.upload(states)
        a_obj.kick(H)
        host_kick(b_obj, H)
        va, vb = _velocities(a_obj, ensemble), _velocities(b_obj, ensemble)
        diff = max(float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max() / max(np.abs(y).max(), 1e-300)) for x, y in zip(va, vb))
        a_obj.kick(-H)
        host_kick(b_obj, -H)

        def arm_a():
            a_obj.kick(sign["A"] * H)
            a_obj.sync()
            sign["A"] = -sign["A"]

        def arm_b():
            host_kick(b_obj, sign["B"] * H)
            sign["B"] = -sign["B"]

        def arm_c():
            a_obj.step(1, 0.0, kenergy=False)  # dt = 0: the launch of a step, the state left where it is
            a_obj.sync()

        arms = {"A": arm_a, "B": arm_b, "C": arm_c}
        passes = {k: _passes_for(run, window) for k, run in arms.items()}
        passes = {k: v + (v & 1) for k, v in passes.items()}  # even: the kicks of a round cancel
        us = {k: [] for k in arms}
        for _ in range(rounds):
            for k, run in arms.items():  # A B C A B C ...
                t0 = time.perf_counter()
                for _ in range(passes[k]):
                    run()
                us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
        st = a_obj.stats()
    finally:
        a_obj.close()
        b_obj.close()
    a, b, c = (statistics.median(us[k]) for k in "ABC")
    return {"kind": "ensemble" if ensemble else "ragged", "population": population, "members": len(sizes), "n_min": min(sizes),
            "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision, "bodies_per_lane": st["bodies_per_lane"],
            "inner_loop": st["inner_loop"], "kick_us": a, "host_round_trip_us": b, "step_us": c, "ratio": a / b, "kick_to_step": a / c,
            "kick_rounds_us": us["A"], "host_round_trip_rounds_us": us["B"], "step_rounds_us": us["C"], "passes_per_round": passes,
            "worst_relative_difference_of_the_arms": diff, "arms_agree_to_rounding": bool(diff <= (1e-5 if precision == 32 else 1e-13))}


def measure_gate_ensemble(nbx, rounds=5, window=0.05):
    S, n = GATE_ENSEMBLE
    return measure(nbx, [n] * S, 32, rounds, window, ensemble=True, population="%d x %d" % (S, n))


def measure_gate_ragged(nbx, rounds=5, window=0.05):
    return measure(nbx, GATE_RAGGED, 32, rounds, window, population="16 sizes spread evenly over 512 ... 4096")


WHAT = ("us per pass over all members, fp32; kick: one nbx_ensemble_kick / nbx_ragged_kick call and a synchronisation; host round trip: "
        "nbx_*_accel of all members, download, v += a * h in numpy, upload; step: one step launch (dt = 0) and a synchronisation; medians "
        "of the rounds, arms alternated, one process; ratio = kick / host round trip, kick_to_step = kick / step")


def write(path, cells):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"what": WHAT, "cells": cells}, f, indent=1)
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
    print("%-42s %10s %14s %10s %8s %12s" % ("population", "kick us", "round trip us", "step us", "ratio", "kick / step"))
    for fn in (measure_gate_ensemble, measure_gate_ragged):
        r = fn(nbx, a.rounds, a.window)
        cells.append(r)
        print("%-42s %10.1f %14.1f %10.1f %8.3f %12.3f%s" % (r["population"], r["kick_us"], r["host_round_trip_us"], r["step_us"], r["ratio"],
                                                           r["kick_to_step"], "" if r["arms_agree_to_rounding"] else "  VALUES DIFFER"), flush=True)
        write(a.out, cells)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
