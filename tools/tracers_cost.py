"""Cost of resident tracers (include/nbx_tracers.h) against the round trip they replace, in one process, fp32, per time step:

  A  one <prefix>_tracers_step call of K steps, then a synchronisation
  B  K round trips on an object that holds the same bodies: <prefix>_field at the host's tracer positions, the update
     w += a dt; p += w dt in numpy, <prefix>_step(dt, 1)            (tests/tracers_ref.py: round_trip)
  S  one <prefix>_step call of K steps on the same kind of object without tracers, then a synchronisation   (recorded)

  context   n = 4096 bodies, m = 4096 tracers
  ensemble  16 members of 2048 bodies, m = 2048 tracers per member
  ragged    16 sizes spread over 512 ... 4096, m = 1024 tracers per member

Every object is created and uploaded beforehand.  A and B do the same pair work; B adds two copies and a synchronisation per
step.  ratio = A / B per step (tests/test_tracers_gpu.py gates the context and the ensemble cell at <= 1.0); step_ratio = A / S,
what the tracers add to a step, is recorded.  Per cell: the calibration passes double as warm-up, then `rounds` rounds, the arms
alternated; a round times `passes` back-to-back passes of an arm (each pass ends in a synchronisation) so that it lasts >=
`window` seconds; the figures are medians over the rounds, in us per step.

A fourth cell is recorded, not gated: one context of 131072 bodies and as many tracers, where a step is milliseconds of pair
work -- one nbx_tracers_step(dt, 1) against nbx_field + nbx_step(dt, 1), both 2 n^2 pairs per step: pairs per second of each.

usage: python tools/tracers_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/tracers_cost.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "tracers_cost.json")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from field_cost import MEMBERS, RAGGED_SIZES, _time, member_points, member_state  # noqa: E402  the field's cells and its timing loop

CONTEXT_N, CONTEXT_M = 4096, 4096
ENSEMBLE_N, ENSEMBLE_M = 2048, 2048
RAGGED_M = 1024
LARGE_N = 131072
K_STEPS = 10
DT = 0.01
POS, VEL = ("pos_x", "pos_y", "pos_z"), ("vel_x", "vel_y", "vel_z")
ACC = ("acc_x", "acc_y", "acc_z")


def member_tracers(m, seed):
    """m tracers: positions uniform in [-1, 1]^3, velocities 0.3 uniform in [-1, 1]^3, fp32."""
    v = 0.3 * np.random.default_rng([seed, m, 1]).uniform(-1.0, 1.0, (3, m))
    out = dict(zip(POS, member_points(m, seed)))
    out.update({k: np.ascontiguousarray(c.astype(np.float32)) for k, c in zip(VEL, v)})
    return out


def _round_trips(o, tr, steps, dt):
    """`steps` round trips of object o (bodies resident) and the host tracers tr (arrays of any one shape), in place."""
    h = np.float32(dt)
    for _ in range(steps):
        f = o.field(tr["pos_x"], tr["pos_y"], tr["pos_z"])
        for p, w, a in zip(POS, VEL, ACC):
            tr[w] = tr[w] + f[a] * h
            tr[p] = tr[p] + tr[w] * h
        o.step(1, dt, kenergy=False)


def _make(nbx, kind):
    if kind == "context":
        sizes, m = [CONTEXT_N], CONTEXT_M
        new = lambda: nbx.Context(CONTEXT_N, 32)
    elif kind == "ensemble":
        sizes, m = [ENSEMBLE_N] * MEMBERS, ENSEMBLE_M
        new = lambda: nbx.Ensemble(ENSEMBLE_N, MEMBERS, 32)
    else:
        sizes, m = list(RAGGED_SIZES), RAGGED_M
        new = lambda: nbx.Ragged(sizes, 32)
    states = [member_state(n, 1000 + k) for k, n in enumerate(sizes)]
    trs = [member_tracers(m, 5000 + k) for k in range(len(sizes))]
    if kind == "context":
        return new, states[0], trs[0], sizes, m
    return new, states, {k: np.ascontiguousarray(np.stack([t[k] for t in trs])) for k in POS + VEL}, sizes, m


def measure(nbx, kind, rounds=5, window=0.05, steps=K_STEPS):
    """One cell, kind "context", "ensemble" or "ragged"."""
    assert rounds >= 5
    new, state, tr, sizes, m = _make(nbx, kind)
    a, b, s = new(), new(), new()
    try:
        for o in (a, b, s):
            o.upload(state)
        a.tracers_upload([tr[k] for k in POS], [tr[k] for k in VEL])
        host = {k: v.copy() for k, v in tr.items()}
        # the two arms compute the same thing: `steps` steps from the same start
        a.tracers_step(steps, DT, kenergy=False)
        _round_trips(b, host, steps, DT)
        got = a.tracers_download()
        same = all(got[k].tobytes() == host[k].tobytes() for k in POS + VEL)

        def arm_a():
            a.tracers_step(steps, DT, kenergy=False)
            a.sync()

        def arm_s():
            s.step(steps, DT, kenergy=False)
            s.sync()

        us, passes = _time({"A": arm_a, "B": lambda: _round_trips(b, host, steps, DT), "S": arm_s}, rounds, window)
    finally:
        for o in (a, b, s):
            o.close()
    ta, tb, ts = (statistics.median(us[k]) / steps for k in "ABS")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "m": m, "precision": 32,
            "steps_per_pass": steps, "tracers_step_us": ta, "round_trip_us": tb, "plain_step_us": ts, "ratio": ta / tb, "step_ratio": ta / ts,
            "tracers_step_rounds_us": [u / steps for u in us["A"]], "round_trip_rounds_us": [u / steps for u in us["B"]],
            "plain_step_rounds_us": [u / steps for u in us["S"]], "passes_per_round": passes, "same_bits_from_both_arms": bool(same)}


def measure_large(nbx, n=LARGE_N, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies and n tracers, one step at a time."""
    assert rounds >= 5
    a, b = nbx.Context(n, 32), nbx.Context(n, 32)
    try:
        state, tr = member_state(n, 999), member_tracers(n, 998)
        a.upload(state)
        b.upload(state)
        a.tracers_upload([tr[k] for k in POS], [tr[k] for k in VEL])
        host = {k: v.copy() for k, v in tr.items()}

        def arm_a():
            a.tracers_step(1, DT, kenergy=False)
            a.sync()

        us, passes = _time({"A": arm_a, "B": lambda: _round_trips(b, host, 1, DT)}, rounds, window)
    finally:
        a.close()
        b.close()
    ta, tb = statistics.median(us["A"]), statistics.median(us["B"])
    pairs = 2.0 * n * n  # the tracers' and the bodies'
    return {"kind": "context", "n": n, "m": n, "precision": 32, "tracers_step_us": ta, "round_trip_us": tb, "tracers_step_pairs_per_s": pairs / (ta * 1e-6),
            "round_trip_pairs_per_s": pairs / (tb * 1e-6), "ratio": ta / tb, "tracers_step_rounds_us": us["A"], "round_trip_rounds_us": us["B"],
            "passes_per_round": passes}


WHAT = ("us per time step, fp32, medians of the rounds, arms alternated, one process, every object created and uploaded beforehand.  "
        "tracers_step: one *_tracers_step call of steps_per_pass steps and a synchronisation; round_trip: per step *_field at the host's "
        "tracer positions, the update in numpy, *_step(dt, 1); plain_step: one *_step call of steps_per_pass steps on an object without "
        "tracers and a synchronisation.  ratio = tracers_step / round_trip (context and ensemble gated <= 1.0 by tests/test_tracers_gpu.py); "
        "step_ratio = tracers_step / plain_step, recorded.  context_n131072: one nbx_tracers_step(dt, 1) against nbx_field + nbx_step(dt, 1) "
        "at 131072 bodies and as many tracers, 2 n^2 pairs per step, recorded")


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
    for kind in ("context", "ensemble", "ragged"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-8s m = %d: tracers_step %.1f us, round trip %.1f us, plain step %.1f us per step; ratio %.3f, step ratio %.2f%s"
              % (kind, r["m"], r["tracers_step_us"], r["round_trip_us"], r["plain_step_us"], r["ratio"], r["step_ratio"],
                 "" if r["same_bits_from_both_arms"] else "  VALUES DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = m = %d: tracers_step %.1f us (%.3g pair/s), field + step %.1f us (%.3g pair/s), ratio %.3f"
          % (r["n"], r["tracers_step_us"], r["tracers_step_pairs_per_s"], r["round_trip_us"], r["round_trip_pairs_per_s"], r["ratio"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
