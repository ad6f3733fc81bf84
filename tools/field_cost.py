"""Cost of the field at caller-supplied points (include/nbx_field.h) against what a caller had to do without it, in one process,
fp32:

  context   n = 4096 bodies, m = 4096 points
            A  one nbx_field call
            B  the workaround: a context of n + m = 8192 bodies created beforehand; per pass an nbx_upload of the bodies plus the
               points as massless bodies, then nbx_accel (O((n + m)^2) pairs, no potential)
  ensemble  16 members of 2048 bodies, m = 2048 points per member
            A  one nbx_ensemble_field call over all members
            B  16 nbx_field calls on 16 default contexts created and uploaded beforehand that hold the same states
  ragged    16 sizes spread over 512 ... 4096, m = 1024 points per member; A and B likewise (nbx_ragged_field)

B is the most favourable alternative: it is not charged for creating contexts, for building the arrays it uploads or, in the
batch cells, for downloading the members and uploading them again.  In the batch cells A and B return the same bits (checked); in
the context cell B's accelerations of the appended bodies are compared with A's to 1e-4 of the largest (another summation order).
Per cell: the calibration passes double as warm-up, then `rounds` rounds, the arms alternated; a round times `passes`
back-to-back passes of an arm (each pass ends in a synchronisation) so that it lasts >= `window` seconds; the figures are medians
over the rounds, in us per pass.  ratio = A / B.

A fourth cell is recorded, not gated: one context of 131072 bodies and as many points, where a call is milliseconds of pair work --
F one nbx_field call (n m pairs, upload of the points and read-back included), C one nbx_accel call (n^2 pairs, read-back
included): pairs per second of each and their quotient.

usage: python tools/field_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/field_cost.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "field_cost.json")

MEMBERS = 16
CONTEXT_N, CONTEXT_M = 4096, 4096
ENSEMBLE_N, ENSEMBLE_M = 2048, 2048
RAGGED_SIZES = [512 + round(k * (4096 - 512) / (MEMBERS - 1)) for k in range(MEMBERS)]  # 512 ... 4096, evenly
RAGGED_M = 1024
LARGE_N = 131072
KEYS = ("acc_x", "acc_y", "acc_z", "phi")
FIELDS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")


def member_state(n, seed, dtype=np.float32):
    """n bodies, G sum m ~ 1, positions uniform in [-1, 1]^3, velocities 0.3 uniform in [-1, 1]^3 (the systems of the kick tests)."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.5, 1.5, n) / (6.67259e-11 * n)
    pos = rng.uniform(-1.0, 1.0, (3, n))
    vel = 0.3 * rng.uniform(-1.0, 1.0, (3, n))
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in zip(FIELDS, list(pos) + list(vel) + [m])}


def member_points(m, seed, dtype=np.float32):
    """m points uniform in [-1, 1]^3: (px, py, pz)."""
    p = np.random.default_rng([seed, m]).uniform(-1.0, 1.0, (3, m))
    return [np.ascontiguousarray(c.astype(dtype)) for c in p]


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


def _time(arms, rounds, window):
    """{arm: us per pass of every round}, the arms alternated; and the passes per round."""
    passes = {k: _passes_for(run, window) for k, run in arms.items()}
    us = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():
            t0 = time.perf_counter()
            for _ in range(passes[k]):
                run()
            us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
    return us, passes


def measure_context(nbx, rounds=5, window=0.05):
    """The context cell: nbx_field against upload + nbx_accel on a context of n + m bodies."""
    assert rounds >= 5
    n, m = CONTEXT_N, CONTEXT_M
    s, p = member_state(n, 2000), member_points(m, 2001)
    aug = {f: np.concatenate([s[f], q]) for f, q in zip(FIELDS[:3], p)}
    aug.update({f: np.concatenate([s[f], np.zeros(m, dtype=np.float32)]) for f in FIELDS[3:]})
    c, big = nbx.Context(n, 32), nbx.Context(n + m, 32)
    try:
        c.upload(s)

        def workaround():
            big.upload(aug)
            return big.accel()

        arms = {"A": lambda: c.field(*p), "B": workaround}
        a, b = arms["A"](), arms["B"]()
        scale = max(float(np.abs(a[k]).max()) for k in KEYS[:3])
        close = all(float(np.abs(a[k] - w[n:]).max()) <= 1e-4 * scale for k, w in zip(KEYS[:3], b))
        us, passes = _time(arms, rounds, window)
    finally:
        c.close()
        big.close()
    ta, tb = statistics.median(us["A"]), statistics.median(us["B"])
    return {"kind": "context", "n": n, "m": m, "precision": 32, "field_us": ta, "workaround_us": tb, "ratio": ta / tb,
            "field_pairs": float(n) * m, "workaround_pairs": float(n + m) * (n + m), "field_rounds_us": us["A"], "workaround_rounds_us": us["B"],
            "passes_per_round": passes, "accelerations_agree": bool(close)}


def measure(nbx, kind, rounds=5, window=0.05):
    """A batch cell, kind "ensemble" or "ragged": one batch call against one nbx_field call per context."""
    assert rounds >= 5
    sizes = [ENSEMBLE_N] * MEMBERS if kind == "ensemble" else list(RAGGED_SIZES)
    m = ENSEMBLE_M if kind == "ensemble" else RAGGED_M
    states = [member_state(n, 1000 + k) for k, n in enumerate(sizes)]
    pts = [member_points(m, 3000 + k) for k in range(MEMBERS)]
    P = [np.ascontiguousarray(np.stack([q[c] for q in pts])) for c in range(3)]  # (members, m)
    batch = nbx.Ensemble(ENSEMBLE_N, MEMBERS, 32) if kind == "ensemble" else nbx.Ragged(sizes, 32)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, 32))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.field(*P), "B": lambda: [c.field(*q) for c, q in zip(ctxs, pts)]}
        a, b = arms["A"](), arms["B"]()
        same = all(a[k][j].tobytes() == b[j][k].tobytes() for j in range(MEMBERS) for k in KEYS)
        us, passes = _time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    ta, tb = statistics.median(us["A"]), statistics.median(us["B"])
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "m": m, "precision": 32,
            "batch_us": ta, "contexts_us": tb, "ratio": ta / tb, "batch_rounds_us": us["A"], "contexts_rounds_us": us["B"],
            "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def measure_large(nbx, n=LARGE_N, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, nbx_field at n points against nbx_accel."""
    assert rounds >= 5
    c = nbx.Context(n, 32)
    try:
        c.upload(member_state(n, 999))
        p = member_points(n, 998)
        us, passes = _time({"F": lambda: c.field(*p), "C": c.accel}, rounds, window)
    finally:
        c.close()
    f, a = statistics.median(us["F"]), statistics.median(us["C"])
    pf, pa = float(n) * n / (f * 1e-6), float(n) * n / (a * 1e-6)
    return {"kind": "context", "n": n, "m": n, "precision": 32, "field_us": f, "accel_us": a, "field_pairs_per_s": pf, "accel_pairs_per_s": pa,
            "pair_rate_ratio": pf / pa, "field_rounds_us": us["F"], "accel_rounds_us": us["C"], "passes_per_round": passes}


WHAT = ("us per pass, fp32, medians of the rounds, arms alternated, one process.  context: one nbx_field call (n = m = 4096) against "
        "nbx_upload + nbx_accel on a context of 8192 bodies created beforehand; ensemble (16 x 2048, m = 2048) and ragged (16 sizes over "
        "512 ... 4096, m = 1024): one batch call against one nbx_field call on each of 16 default contexts created and uploaded "
        "beforehand; ratio = first arm / second arm (gated <= 1.0 by tests/test_field_gpu.py).  context_n131072: one nbx_field call at "
        "131072 points against one nbx_accel call on the same context, pairs per second of the whole calls, recorded")


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
    r = measure_context(nbx, rounds=a.rounds, window=a.window)
    print("context  n = %d, m = %d: field %.1f us, upload + accel of %d bodies %.1f us, ratio %.3f%s"
          % (r["n"], r["m"], r["field_us"], r["n"] + r["m"], r["workaround_us"], r["ratio"], "" if r["accelerations_agree"] else "  VALUES DIFFER"),
          flush=True)
    write(a.out, {"context": r})
    for kind in ("ensemble", "ragged"):
        r = measure(nbx, kind, rounds=a.rounds, window=a.window)
        print("%-8s m = %d: batch %.1f us, 16 contexts %.1f us, ratio %.3f%s"
              % (kind, r["m"], r["batch_us"], r["contexts_us"], r["ratio"], "" if r["same_values_from_both_arms"] else "  VALUES DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = m = %d: field %.1f us (%.3g pair/s), accel %.1f us (%.3g pair/s), rate ratio %.2f"
          % (r["n"], r["field_us"], r["field_pairs_per_s"], r["accel_us"], r["accel_pairs_per_s"], r["pair_rate_ratio"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
