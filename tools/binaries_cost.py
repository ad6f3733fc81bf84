"""Cost of the most bound partners and bound counts (include/nbx_binaries.h) of every member of a batch object, in one process:

  A  one nbx_ensemble_binaries / nbx_ragged_binaries call over all M members (one pair-work launch, one finish launch, one
     read-back), with the count
  B  M nbx_binaries calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and
     hold the same states (two launches and a synchronising read-back each)

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts.  A and B return the same arrays (checked).  The cells, the warm-up and the repetitions are those of
tools/timescale_cost.py (its member_state and its calibration are used as they are, the masses scaled to order 1/G so that there
is something bound): the calibration passes double as warm-up, then `rounds` rounds, the arms alternated; a round times `passes`
back-to-back passes of an arm (each pass ends in a synchronisation) so that it lasts >= `window` seconds; the figures are
medians over the rounds, in us per pass.  ratio = A / B.

Two more cells are recorded and not gated.  context_n8192: one nbx_binaries call against what it replaces, a download and the
O(n^2) numpy search of the host (row chunks of 512, fp64, the same three arrays).  context_n131072: one nbx_binaries call with
the count and one without against nbx_timescale and nbx_neighbours (with its count) on the same context, the two pair kernels it
sits between -- there a call is milliseconds of pair work and the pair loops are what is timed.

usage: python tools/binaries_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/binaries_cost.json, fp32."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timescale_cost as TC  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "binaries_cost.json")
KEYS = ("partner", "energy", "bound")
HOST_N, LARGE_N = 8192, 131072
G = float(np.float32(6.67259e-11))
EPS2 = float(np.float32(1e-3))


def member_state(n, seed, dtype):
    """timescale_cost.member_state with masses of order 1/G and velocities to match: about half of all pairs are bound."""
    s = TC.member_state(n, seed, np.float64)
    s["mass"] = s["mass"] * n
    for k in ("vel_x", "vel_y", "vel_z"):
        s[k] = s[k] * (1.4 / 0.3)
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in s.items()}


def _same(a, b):
    """A's result (a dict of (M, n) arrays, or a list of dicts) against B's list of dicts: the same arrays."""
    if isinstance(a, dict):
        a = [{k: a[k][m] for k in KEYS} for m in range(len(b))]
    return len(a) == len(b) and all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in KEYS)


def _time(arms, rounds, window):
    passes = {k: TC._passes_for(run, window) for k, run in arms.items()}
    us = {k: [] for k in arms}
    for _ in range(rounds):
        for k, run in arms.items():  # the arms alternated
            t0 = time.perf_counter()
            for _ in range(passes[k]):
                run()
            us[k].append((time.perf_counter() - t0) / passes[k] * 1e6)
    return us, passes


def measure(nbx, kind, precision=32, rounds=5, window=0.05):
    """One cell, kind "ensemble" or "ragged".  Median us per pass of each arm, ratio = A / B."""
    assert rounds >= 5
    sizes = [TC.ENSEMBLE_N] * TC.MEMBERS if kind == "ensemble" else list(TC.RAGGED_SIZES)
    dtype = np.float32 if precision == 32 else np.float64
    states = [member_state(n, 1000 + k, dtype) for k, n in enumerate(sizes)]
    batch = nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arms = {"A": batch.binaries, "B": lambda: [c.binaries() for c in ctxs]}
        first = arms["A"]()
        same = _same(first, arms["B"]())
        bound = first["bound"] if isinstance(first, dict) else np.concatenate([m["bound"] for m in first])
        us, passes = _time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b = (statistics.median(us[k]) for k in "AB")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "mean_bound": float(bound.mean()), "batch_us": a, "contexts_us": b, "ratio": a / b, "batch_rounds_us": us["A"],
            "contexts_rounds_us": us["B"], "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def host_search(state, mass, chunk=512):
    """The host's way: the three arrays of one downloaded system (positions and velocities; the masses are the caller's) by an
    O(n^2) numpy search in fp64."""
    x = [np.asarray(state[k], dtype=np.float64) for k in ("pos_x", "pos_y", "pos_z")]
    v = [np.asarray(state[k], dtype=np.float64) for k in ("vel_x", "vel_y", "vel_z")]
    gm = G * np.asarray(mass, dtype=np.float64)
    n = len(gm)
    partner, energy, bound = np.empty(n, dtype=np.int32), np.empty(n), np.empty(n, dtype=np.int32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        r2 = sum((x[c][None, :] - x[c][lo:hi, None]) ** 2 for c in range(3)) + EPS2
        e = 0.5 * sum((v[c][None, :] - v[c][lo:hi, None]) ** 2 for c in range(3)) - (gm[None, :] + gm[lo:hi, None]) / np.sqrt(r2)
        rows = np.arange(hi - lo)
        e[rows, np.arange(lo, hi)] = np.inf
        partner[lo:hi] = e.argmin(axis=1)
        energy[lo:hi] = e[rows, partner[lo:hi]]
        bound[lo:hi] = (e < 0).sum(axis=1)
    return {"partner": partner, "energy": energy, "bound": bound}


def measure_host(nbx, n=HOST_N, precision=32, rounds=5):
    """One context of n bodies: one nbx_binaries call against download plus the numpy search."""
    c = nbx.Context(n, precision)
    try:
        s = member_state(n, 998, np.float32 if precision == 32 else np.float64)
        c.upload(s)
        arms = {"D": c.binaries, "H": lambda: host_search(c.download(), s["mass"])}
        dev, host = arms["D"](), arms["H"]()
        us, passes = _time(arms, rounds, 0.05)
    finally:
        c.close()
    d, h = (statistics.median(us[k]) for k in "DH")
    return {"kind": "context", "n": n, "precision": precision, "call_us": d, "download_and_numpy_us": h, "ratio": d / h,
            "partners_equal": int((dev["partner"] == host["partner"]).sum()), "call_rounds_us": us["D"], "download_and_numpy_rounds_us": us["H"],
            "passes_per_round": passes}


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, a binaries call with and without the count against a timescale call and
    a neighbours call with its count."""
    assert rounds >= 5
    c = nbx.Context(n, precision)
    try:
        c.upload(member_state(n, 999, np.float32 if precision == 32 else np.float64))
        arms = {"C": c.binaries, "P": lambda: c.binaries(bound=False), "T": c.timescale, "N": lambda: c.neighbours(0.25)}
        us, passes = _time(arms, rounds, window)
    finally:
        c.close()
    w, p, t, nb = (statistics.median(us[k]) for k in "CPTN")
    pairs = float(n) * (n - 1)
    return {"kind": "context", "n": n, "precision": precision, "with_count_us": w, "partner_only_us": p, "timescale_us": t, "neighbours_us": nb,
            "with_count_over_timescale": w / t, "with_count_over_neighbours": w / nb, "partner_only_over_timescale": p / t,
            "with_count_pairs_per_s": pairs / (w * 1e-6), "partner_only_pairs_per_s": pairs / (p * 1e-6),
            "timescale_pairs_per_s": pairs / (t * 1e-6), "neighbours_pairs_per_s": pairs / (nb * 1e-6), "with_count_rounds_us": us["C"],
            "partner_only_rounds_us": us["P"], "timescale_rounds_us": us["T"], "neighbours_rounds_us": us["N"], "passes_per_round": passes}


WHAT = ("us per pass, fp32; ensemble / ragged: over all 16 members; batch: one nbx_ensemble_binaries / nbx_ragged_binaries call; contexts: "
        "one nbx_binaries call on each of 16 default contexts, one per member, created and uploaded beforehand (not charged for download, "
        "create or upload); medians of the rounds, arms alternated, one process; ratio = batch / contexts (gated <= 1.0 by "
        "tests/test_binaries_gpu.py); context_n8192: one nbx_binaries call against a download and the numpy search of the host "
        "(recorded); context_n131072: one nbx_binaries call with the count and one without against one nbx_timescale and one "
        "nbx_neighbours call on the same context, where the pair loops are what is timed (recorded)")


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
    print("context n = %d: one call %.1f us, download and numpy search %.1f us, ratio %.5f; %d of %d partners equal"
          % (r["n"], r["call_us"], r["download_and_numpy_us"], r["ratio"], r["partners_equal"], r["n"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d: with the count %.1f us (%.3g pair/s), partner and energy only %.1f us (%.3g pair/s), timescale %.1f us "
          "(%.3g pair/s), neighbours %.1f us (%.3g pair/s)" % (r["n"], r["with_count_us"], r["with_count_pairs_per_s"], r["partner_only_us"],
                                                              r["partner_only_pairs_per_s"], r["timescale_us"], r["timescale_pairs_per_s"],
                                                              r["neighbours_us"], r["neighbours_pairs_per_s"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
