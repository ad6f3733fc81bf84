"""Cost of the k nearest neighbours (include/nbx_knn.h), in one process:

  A  one nbx_ensemble_knn / nbx_ragged_knn call over all M members (one pair-work launch, one finish launch, one read-back), k = 6
  B  M nbx_knn calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and hold
     the same states (two launches and a synchronising read-back each)

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts.  A and B return the same arrays (checked).  The cells, the warm-up and the repetitions are those of
tools/timescale_cost.py (its member_state and its calibration are used as they are): the calibration passes double as warm-up,
then `rounds` rounds, the arms alternated; a round times `passes` back-to-back passes of an arm (each pass ends in a
synchronisation) so that it lasts >= `window` seconds; the figures are medians over the rounds, in us per pass.  ratio = A / B.

Recorded and not gated:
  context_n8192    one nbx_knn call (k = 6) on a context of 8192 bodies against what the call replaces: a download plus the
                   numpy search of tests/knn_ref.py (an fp64 r2 matrix and a lexsort, in row chunks), timed once
  context_n131072  where the pair loop is what is timed: k = 1, 6 and 16 against nbx_neighbours without a count on the same
                   context, as the time and as the ratio to it -- "almost every tile iteration takes the fast path, so the call
                   costs about what nbx_neighbours without a count costs" is read here -- and the same state with the bodies sorted
                   by DECREASING distance from body 0, the adversarial order: body 0 inserts at every pair, and so does, with it,
                   its whole wave

usage: python tools/knn_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/knn_cost.json, fp32."""
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

OUT = os.path.join(ROOT, "profiles", "knn_cost.json")
K = 6
KEYS = ("index", "r2")


def _same(a, b):
    """A's result (a dict of (M, n, k) arrays, or a list of dicts) against B's list of dicts: the same arrays."""
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


def measure(nbx, kind, precision=32, rounds=5, window=0.05, k=K):
    """One cell, kind "ensemble" or "ragged".  Median us per pass of each arm, ratio = A / B."""
    assert rounds >= 5
    sizes = [TC.ENSEMBLE_N] * TC.MEMBERS if kind == "ensemble" else list(TC.RAGGED_SIZES)
    dtype = np.float32 if precision == 32 else np.float64
    states = [TC.member_state(n, 1000 + m, dtype) for m, n in enumerate(sizes)]
    batch = nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.knn(k), "B": lambda: [c.knn(k) for c in ctxs]}
        same = _same(arms["A"](), arms["B"]())
        us, passes = _time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b = (statistics.median(us[key]) for key in "AB")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "k": k, "batch_us": a, "contexts_us": b, "ratio": a / b, "batch_rounds_us": us["A"], "contexts_rounds_us": us["B"],
            "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def measure_host(nbx, n=8192, precision=32, rounds=5, window=0.05, k=K):
    """One context of n bodies: the call against a download plus the numpy search (timed once: it takes seconds)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import knn_ref
    c = nbx.Context(n, precision)
    try:
        c.upload(TC.member_state(n, 998, np.float32 if precision == 32 else np.float64))
        us, passes = _time({"D": lambda: c.knn(k)}, rounds, window)
        t0 = time.perf_counter()
        state = c.download()
        host = knn_ref.knn(state, k, precision)
        host_us = (time.perf_counter() - t0) * 1e6
        # the device rounds r2 in T, the host search in fp64: held to each other as the device tests hold them (knn_ref.differs)
        found = knn_ref.differs(c.knn(k), host, state, precision)
    finally:
        c.close()
    d = statistics.median(us["D"])
    return {"kind": "context", "n": n, "precision": precision, "k": k, "device_us": d, "download_and_numpy_us": host_us, "ratio": d / host_us,
            "device_rounds_us": us["D"], "passes_per_round": passes, "agrees_with_the_host_search": not found, "differences": found}


LARGE_N = 131072
LARGE_KS = (1, 6, 16)


def adversarial(state):
    """The state with its bodies sorted by decreasing distance from body 0 (which stays body 0)."""
    d2 = sum((np.asarray(state[c], dtype=np.float64) - float(state[c][0])) ** 2 for c in ("pos_x", "pos_y", "pos_z"))
    order = np.concatenate([[0], 1 + np.argsort(-d2[1:], kind="stable")])
    return {f: np.ascontiguousarray(v[order]) for f, v in state.items()}


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, knn calls against a neighbours call without a count, in the state's own
    order and in the adversarial one."""
    assert rounds >= 5
    state = TC.member_state(n, 999, np.float32 if precision == 32 else np.float64)
    out = {"kind": "context", "n": n, "precision": precision}
    pairs = float(n) * (n - 1)
    for name, st in (("random_order", state), ("decreasing_distance_from_body_0", adversarial(state))):
        c = nbx.Context(n, precision)
        try:
            c.upload(st)
            arms = {"N": c.neighbours}
            for k in LARGE_KS:
                arms["k%d" % k] = lambda k=k: c.knn(k)
            us, passes = _time(arms, rounds, window)
        finally:
            c.close()
        nb = statistics.median(us["N"])
        cell = {"neighbours_without_count_us": nb, "neighbours_pairs_per_s": pairs / (nb * 1e-6), "passes_per_round": passes,
                "neighbours_rounds_us": us["N"]}
        for k in LARGE_KS:
            t = statistics.median(us["k%d" % k])
            cell["k%d_us" % k] = t
            cell["k%d_ratio_to_neighbours" % k] = t / nb
            cell["k%d_pairs_per_s" % k] = pairs / (t * 1e-6)
            cell["k%d_rounds_us" % k] = us["k%d" % k]
        out[name] = cell
    return out


WHAT = ("us per pass, fp32; ensemble and ragged: all 16 members, k = 6, batch: one nbx_ensemble_knn / nbx_ragged_knn call, contexts: one "
        "nbx_knn call on each of 16 default contexts, one per member, created and uploaded beforehand (not charged for download, create "
        "or upload), medians of the rounds, arms alternated, one process, ratio = batch / contexts (gated <= 1.0 by "
        "tests/test_knn_gpu.py); context_n8192: one nbx_knn call against a download plus the numpy search of tests/knn_ref.py "
        "(recorded); context_n131072: nbx_knn with k = 1, 6 and 16 against nbx_neighbours without a count on the same context, in the "
        "state's own order and with the bodies sorted by decreasing distance from body 0 (recorded)")


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
    r = measure_host(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d, k = %d: the call %.1f us, download plus numpy search %.0f us (%.5f of it)%s"
          % (r["n"], r["k"], r["device_us"], r["download_and_numpy_us"], r["ratio"], "" if r["agrees_with_the_host_search"] else "  DIFFERS: %r" % r["differences"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    for name in ("random_order", "decreasing_distance_from_body_0"):
        c = r[name]
        print("context n = %d, %s: neighbours without a count %.1f us; " % (r["n"], name, c["neighbours_without_count_us"]) +
              ", ".join("k = %d %.1f us (%.2f)" % (k, c["k%d_us" % k], c["k%d_ratio_to_neighbours" % k]) for k in LARGE_KS), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
