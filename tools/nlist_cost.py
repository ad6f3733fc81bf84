"""Cost of the neighbour lists (include/nbx_nlist.h), in one process:

  A  one nbx_ensemble_nlist / nbx_ragged_nlist call over all M members (a filling call: two pair-work launches, five small
     launches, two synchronisations), at a radius with about 6 neighbours per body
  B  M nbx_nlist calls on M default contexts, one per member and of its size, that were created and uploaded beforehand and hold
     the same states (the same launches and synchronisations each)

B is the most favourable alternative without the batch call: it is not charged for downloading the members or for creating and
uploading the contexts.  A and B return the same bytes (checked).  Both arms go through nbx.py's nlist() with its default
capacity, 16 entries per body, which these radii do not exceed: one filling call each.  The cells, the warm-up and the
repetitions are those of tools/timescale_cost.py (its member_state and its calibration are used as they are): the calibration
passes double as warm-up, then `rounds` rounds, the arms alternated; a round times `passes` back-to-back passes of an arm so that
it lasts >= `window` seconds; the figures are medians over the rounds, in us per pass.  ratio = A / B.

Recorded and not gated:
  context_n8192    one filling call on a context of 8192 bodies against what the call replaces: a download plus the numpy search of
                   tests/nlist_ref.py (an fp64 r2 matrix in row chunks), timed once
  context_n131072  where the pair loop is what is timed: at about 6 neighbours per body a counting call and a filling call
                   against nbx_neighbours with the count on the same context, as times and as ratios to it; and a filling call at
                   about 200 neighbours per body, where the fill's wave-wide branch is usually taken

usage: python tools/nlist_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/nlist_cost.json, fp32."""
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

OUT = os.path.join(ROOT, "profiles", "nlist_cost.json")
KEYS = ("offsets", "index", "r2")
DEGREE = 6.0
DENSE_DEGREE = 200.0


def radius_for(n, degree):
    """The radius at which a body of n uniform in [-1, 1]^3 has `degree` neighbours on average (less near the faces)."""
    return float((degree * 8.0 * 3.0 / (4.0 * np.pi * n)) ** (1.0 / 3))


def _same(a, b):
    """A's result (one dict over all members) against B's list of dicts: the same bytes, member after member."""
    if a["total"] != sum(x["total"] for x in b):
        return False
    body = entry = 0
    for x in b:
        n, t = len(x["offsets"]) - 1, x["total"]
        if not (np.array_equal(a["offsets"][body:body + n + 1] - a["offsets"][body], x["offsets"]) and
                a["index"][entry:entry + t].tobytes() == x["index"].tobytes() and a["r2"][entry:entry + t].tobytes() == x["r2"].tobytes()):
            return False
        body, entry = body + n, entry + t
    return True


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
    states = [TC.member_state(n, 1000 + m, dtype) for m, n in enumerate(sizes)]
    radius = radius_for(sum(n * n for n in sizes) / sum(sizes), DEGREE)  # one radius for all members: about 6 per body over all bodies
    batch = nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, precision))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.nlist(radius), "B": lambda: [c.nlist(radius) for c in ctxs]}
        a0 = arms["A"]()
        same = _same(a0, arms["B"]())
        us, passes = _time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    a, b = (statistics.median(us[key]) for key in "AB")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": precision,
            "radius": radius, "neighbours_per_body": a0["total"] / sum(sizes), "batch_us": a, "contexts_us": b, "ratio": a / b,
            "batch_rounds_us": us["A"], "contexts_rounds_us": us["B"], "passes_per_round": passes, "same_bytes_from_both_arms": bool(same)}


def measure_host(nbx, n=8192, precision=32, rounds=5, window=0.05):
    """One context of n bodies: the call against a download plus the numpy search (timed once: it takes seconds)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nlist_ref
    radius = radius_for(n, DEGREE)
    c = nbx.Context(n, precision)
    try:
        c.upload(TC.member_state(n, 998, np.float32 if precision == 32 else np.float64))
        us, passes = _time({"D": lambda: c.nlist(radius)}, rounds, window)
        t0 = time.perf_counter()
        state = c.download()
        host = nlist_ref.nlist(state, radius, precision)
        host_us = (time.perf_counter() - t0) * 1e6
        # the device rounds r2 in T, the host search in fp64: a pair within a few u of h2 may be decided differently
        got = c.nlist(radius)
        found = nlist_ref.differs(got, host, precision)
        unambiguous = not nlist_ref.ambiguous(state, radius, precision)
    finally:
        c.close()
    d = statistics.median(us["D"])
    return {"kind": "context", "n": n, "precision": precision, "radius": radius, "neighbours_per_body": got["total"] / n, "device_us": d,
            "download_and_numpy_us": host_us, "ratio": d / host_us, "device_rounds_us": us["D"], "passes_per_round": passes,
            "no_pair_within_8u_of_h2": bool(unambiguous), "agrees_with_the_host_search": not found, "differences": found}


LARGE_N = 131072


def measure_large(nbx, n=LARGE_N, precision=32, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, counting and filling calls against a neighbours call with the count."""
    assert rounds >= 5
    state = TC.member_state(n, 999, np.float32 if precision == 32 else np.float64)
    r6, r200 = radius_for(n, DEGREE), radius_for(n, DENSE_DEGREE)
    c = nbx.Context(n, precision)
    try:
        c.upload(state)
        per = {"sparse": c.nlist(r6, 0)["total"] / n, "dense": c.nlist(r200, 0)["total"] / n}
        arms = {"N": lambda: c.neighbours(r6), "count": lambda: c.nlist(r6, 0), "fill": lambda: c.nlist(r6),
                "N_dense": lambda: c.neighbours(r200), "count_dense": lambda: c.nlist(r200, 0),
                "fill_dense": lambda: c.nlist(r200, int(per["dense"] * n))}
        us, passes = _time(arms, rounds, window)
    finally:
        c.close()
    med = {k: statistics.median(v) for k, v in us.items()}
    pairs = float(n) * (n - 1)
    out = {"kind": "context", "n": n, "precision": precision, "passes_per_round": passes, "rounds_us": us}
    for tag, suffix, radius in (("about_6_per_body", "", r6), ("about_200_per_body", "_dense", r200)):
        nb = med["N" + suffix]
        out[tag] = {"radius": radius, "neighbours_per_body": per["dense" if suffix else "sparse"], "neighbours_with_count_us": nb,
                    "neighbours_pairs_per_s": pairs / (nb * 1e-6), "counting_call_us": med["count" + suffix],
                    "counting_call_ratio_to_neighbours": med["count" + suffix] / nb, "filling_call_us": med["fill" + suffix],
                    "filling_call_ratio_to_neighbours": med["fill" + suffix] / nb,
                    "fill_pass_and_lists_us": med["fill" + suffix] - med["count" + suffix]}
    return out


WHAT = ("us per pass, fp32; ensemble and ragged: all 16 members at a radius with about 6 neighbours per body, batch: one filling "
        "nbx_ensemble_nlist / nbx_ragged_nlist call, contexts: one filling nbx_nlist call on each of 16 default contexts, one per member, "
        "created and uploaded beforehand (not charged for download, create or upload), medians of the rounds, arms alternated, one "
        "process, ratio = batch / contexts (gated <= 1.0 by tests/test_nlist_gpu.py); context_n8192: one filling call against a download "
        "plus the numpy search of tests/nlist_ref.py (recorded); context_n131072: a counting and a filling call against nbx_neighbours "
        "with the count on the same context at about 6 and at about 200 neighbours per body (recorded); every time includes nbx.py's "
        "allocation of the result arrays and, for a filling call, the read-back of the lists")


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
        print("%-10s %10.1f %12.1f %8.3f  (%.2f per body)%s" % (kind, r["batch_us"], r["contexts_us"], r["ratio"], r["neighbours_per_body"],
                                                                "" if r["same_bytes_from_both_arms"] else "  BYTES DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_host(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d, %.2f per body: the call %.1f us, download plus numpy search %.0f us (%.5f of it)%s"
          % (r["n"], r["neighbours_per_body"], r["device_us"], r["download_and_numpy_us"], r["ratio"],
             "" if r["agrees_with_the_host_search"] else "  DIFFERS: %r" % r["differences"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    for tag in ("about_6_per_body", "about_200_per_body"):
        c = r[tag]
        print("context n = %d, %s (%.1f): neighbours with the count %.1f us; counting call %.1f us (%.2f), filling call %.1f us (%.2f)"
              % (r["n"], tag, c["neighbours_per_body"], c["neighbours_with_count_us"], c["counting_call_us"], c["counting_call_ratio_to_neighbours"],
                 c["filling_call_us"], c["filling_call_ratio_to_neighbours"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
