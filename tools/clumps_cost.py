"""Cost of the clumps call (include/nbx_clumps.h) of every member of a batch object, in one process:

  A  one nbx_ensemble_clumps / nbx_ragged_clumps call over all M members (one label upload, one pair-work launch, one finish
     launch, one read-back)
  B  M nbx_clumps calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and hold
     the same states (an upload, two launches and a synchronising read-back each)

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts.  A and B return the same arrays (checked).  The cells, the states, the warm-up and the repetitions are
those of tools/binaries_cost.py (its member_state and _time are used as they are); the labels are i % 7 with every 11th body in
no clump.  ratio = A / B.

Two more cells are recorded and not gated.  context_n8192: one nbx_clumps call against what it replaces, a download and the
numpy evaluation of the host (fp64, per clump).  context_n131072: one nbx_clumps call against nbx_field with m = n at the bodies'
own positions and nbx_binaries on the same context, the pair kernels it sits between -- there a call is milliseconds of pair work
and the pair loops are what is timed; the instruction count predicts about 16/13 of the field.

usage: python tools/clumps_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/clumps_cost.json, fp32."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binaries_cost as BC  # noqa: E402
import timescale_cost as TC  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "clumps_cost.json")
KEYS = ("members", "gm", "centre_x", "centre_y", "centre_z", "velocity_x", "velocity_y", "velocity_z", "phi", "energy")
HOST_N, LARGE_N = 8192, 131072


def stripes(n):
    i = np.arange(n)
    return np.where(i % 11 == 10, -1, i % 7).astype(np.int32)


def _same(a, b):
    if isinstance(a, dict):
        a = [{k: a[k][m] for k in KEYS} for m in range(len(b))]
    return len(a) == len(b) and all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in KEYS)


def measure(nbx, kind, precision=32, rounds=5, window=0.05):
    """One cell, kind "ensemble" or "ragged".  Median us per pass of each arm, ratio = A / B."""
    assert rounds >= 5
    sizes = [TC.ENSEMBLE_N] * TC.MEMBERS if kind == "ensemble" else list(TC.RAGGED_SIZES)
    dtype = np.float32 if precision == 32 else np.float64
    states = [BC.member_state(n, 1000 + k, dtype) for k, n in enumerate(sizes)]
    labels = [stripes(n) for n in sizes]
    batch = nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)
    arg = np.stack(labels) if kind == "ensemble" else labels
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.clumps(arg), "B": lambda: [c.clumps(l) for c, l in zip(ctxs, labels)]}
        first = arms["A"]()
        same = _same(first, arms["B"]())
        energy = first["energy"] if isinstance(first, dict) else np.concatenate([m["energy"] for m in first])
        us, passes = BC._time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b = (statistics.median(us[k]) for k in "AB")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "share_bound": float((energy < 0).mean()), "batch_us": a, "contexts_us": b, "ratio": a / b, "batch_rounds_us": us["A"],
            "contexts_rounds_us": us["B"], "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def host_clumps(state, mass, label):
    """The host's way: phi and energy of every body and the sums of every clump of one downloaded system, fp64, clump by clump."""
    x = np.stack([np.asarray(state[k], dtype=np.float64) for k in ("pos_x", "pos_y", "pos_z")])
    v = np.stack([np.asarray(state[k], dtype=np.float64) for k in ("vel_x", "vel_y", "vel_z")])
    gm = BC.G * np.asarray(mass, dtype=np.float64)
    n = len(gm)
    phi, energy = np.zeros(n), np.zeros(n)
    for l in np.unique(label[label >= 0]):
        idx = np.nonzero(label == l)[0]
        g = gm[idx]
        vel = (v[:, idx] * g).sum(axis=1) / g.sum()
        for lo in range(0, len(idx), 512):
            r = idx[lo:lo + 512]
            r2 = sum((x[c][None, idx] - x[c][r, None]) ** 2 for c in range(3)) + BC.EPS2
            t = g[None, :] / np.sqrt(r2)
            t[np.arange(len(r)), np.arange(lo, lo + len(r))] = 0.0
            phi[r] = -t.sum(axis=1)
        energy[idx] = 0.5 * ((v[:, idx] - vel[:, None]) ** 2).sum(axis=0) + phi[idx]
    return {"phi": phi, "energy": energy}


def measure_host(nbx, n=HOST_N, precision=32, rounds=5):
    """One context of n bodies: one nbx_clumps call against download plus the numpy evaluation."""
    c = nbx.Context(n, precision)
    try:
        s = BC.member_state(n, 998, np.float32 if precision == 32 else np.float64)
        label = stripes(n)
        c.upload(s)
        arms = {"D": lambda: c.clumps(label), "H": lambda: host_clumps(c.download(), s["mass"], label)}
        dev, host = arms["D"](), arms["H"]()
        us, passes = BC._time(arms, rounds, 0.05)
    finally:
        c.close()
    d, h = (statistics.median(us[k]) for k in "DH")
    return {"kind": "context", "n": n, "precision": precision, "call_us": d, "download_and_numpy_us": h, "ratio": d / h,
            "same_sign_of_energy": int(((dev["energy"] < 0) == (host["energy"] < 0)).sum()), "call_rounds_us": us["D"],
            "download_and_numpy_rounds_us": us["H"], "passes_per_round": passes}


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, a clumps call against a field call at the bodies' own positions (m = n)
    and a binaries call."""
    assert rounds >= 5
    c = nbx.Context(n, precision)
    try:
        s = BC.member_state(n, 999, np.float32 if precision == 32 else np.float64)
        label = stripes(n)
        c.upload(s)
        arms = {"C": lambda: c.clumps(label), "F": lambda: c.field(s["pos_x"], s["pos_y"], s["pos_z"]), "B": c.binaries}
        us, passes = BC._time(arms, rounds, window)
    finally:
        c.close()
    w, f, b = (statistics.median(us[k]) for k in "CFB")
    pairs = float(n) * n
    return {"kind": "context", "n": n, "precision": precision, "clumps_us": w, "field_us": f, "binaries_us": b, "clumps_over_field": w / f,
            "clumps_over_binaries": w / b, "predicted_over_field": 16.0 / 13.0, "clumps_pairs_per_s": pairs / (w * 1e-6),
            "field_pairs_per_s": pairs / (f * 1e-6), "binaries_pairs_per_s": pairs / (b * 1e-6), "clumps_rounds_us": us["C"],
            "field_rounds_us": us["F"], "binaries_rounds_us": us["B"], "passes_per_round": passes}


WHAT = ("us per pass, fp32; ensemble / ragged: over all 16 members; batch: one nbx_ensemble_clumps / nbx_ragged_clumps call; contexts: one "
        "nbx_clumps call on each of 16 default contexts, one per member, created and uploaded beforehand (not charged for download, create "
        "or upload); medians of the rounds, arms alternated, one process; ratio = batch / contexts (gated <= 1.0 by "
        "tests/test_clumps_gpu.py); context_n8192: one nbx_clumps call against a download and the numpy evaluation of the host "
        "(recorded); context_n131072: one nbx_clumps call against one nbx_field call with m = n and one nbx_binaries call on the same "
        "context, where the pair loops are what is timed (recorded)")


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
    r = measure_host(nbx, rounds=a.rounds)
    print("context n = %d: one call %.1f us, download and numpy %.1f us, ratio %.5f; sign of energy equal on %d of %d"
          % (r["n"], r["call_us"], r["download_and_numpy_us"], r["ratio"], r["same_sign_of_energy"], r["n"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d: clumps %.1f us (%.3g pair/s), field %.1f us (%.3g pair/s), binaries %.1f us (%.3g pair/s); clumps / field %.3f"
          % (r["n"], r["clumps_us"], r["clumps_pairs_per_s"], r["field_us"], r["field_pairs_per_s"], r["binaries_us"],
             r["binaries_pairs_per_s"], r["clumps_over_field"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
