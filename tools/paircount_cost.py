"""Cost of the pair counts within a list of radii (include/nbx_paircount.h), fp32, 16 radii, in one process:

  context   one context of 8192 bodies.  A: one nbx_paircount call.  B: 16 nbx_neighbours calls on the same context, index and
            r2 NULL, plus the host sums of within -- the route a caller had before: the same pairs walked 16 times, 16
            synchronisations.  ratio = A / B.
  ensemble  16 x 2048.  A: one nbx_ensemble_paircount call over all members.  B: 16 nbx_paircount calls on 16 default contexts,
  ragged    16 sizes spread over 512 ... 4096.  A: one nbx_ragged_paircount call.  B likewise.  The contexts were created and
            uploaded beforehand and hold the same states: B is not charged for download, create or upload.  ratio = A / B.

A and B return the same values (checked).  The cells, the warm-up and the repetitions are those of tools/timescale_cost.py (its
member_state and its calibration are used as they are): the calibration passes double as warm-up, then `rounds` rounds, the
arms alternated; a round times `passes` back-to-back passes of an arm (each pass ends in a synchronisation) so that it lasts >=
`window` seconds; the figures are medians over the rounds, in us per pass.

The cells above are launch-bound.  A fourth takes the pair loop itself: one context of 131072 bodies, where a call is
milliseconds of pair work -- L one call with the lane counters, W one with the wave counters (NBX_PAIRCOUNT_SCHEME, read per
call), N one nbx_neighbours call with the count alone, P20 one call with 20 radii (two passes) and P16 one with 16 under the
compiled default.  Recorded and not gated; the faster of L and W is the scheme the library is compiled to use.

usage: python tools/paircount_cost.py [--out FILE] [--rounds R] [--window SECONDS]   (GPU box, repo root)
Writes profiles/paircount_cost.json."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timescale_cost as TC  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "paircount_cost.json")
RADII20 = [0.03, 0.038, 0.049, 0.062, 0.079, 0.101, 0.128, 0.164, 0.209, 0.266, 0.339, 0.432, 0.55, 0.701, 0.893, 1.138, 1.45, 1.848,
           2.354, 3.0]
RADII = RADII20[:16]
CONTEXT_N = 8192
LARGE_N = 131072
SCHEME = "NBX_PAIRCOUNT_SCHEME"


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


def within_only(nbx, c, radius, within):
    """One nbx_neighbours call with index and r2 NULL: the count alone."""
    rc = nbx.load().nbx_neighbours(c._h, radius, None, None, within.ctypes.data_as(ctypes.c_void_p))
    if rc != nbx.NBX_OK:
        raise RuntimeError(nbx.load().nbx_last_error().decode())
    return within


def _cell(kind, sizes, us, passes, same):
    a, b = (statistics.median(us[k]) for k in "AB")
    return {"kind": kind, "members": len(sizes), "n_min": min(sizes), "n_max": max(sizes), "bodies_total": sum(sizes), "precision": 32,
            "nradii": len(RADII), "batch_us" if kind != "context" else "paircount_us": a,
            "contexts_us" if kind != "context" else "neighbours_x16_us": b, "ratio": a / b, "a_rounds_us": us["A"], "b_rounds_us": us["B"],
            "passes_per_round": passes, "same_values_from_both_arms": bool(same)}


def measure_context(nbx, n=CONTEXT_N, rounds=5, window=0.05):
    """Cell 1: one nbx_paircount call against 16 nbx_neighbours calls on the same context plus the host sums."""
    assert rounds >= 5
    c = nbx.Context(n, 32)
    try:
        c.upload(TC.member_state(n, 998, np.float32))
        within = np.zeros(n, dtype=np.int32)
        arms = {"A": lambda: c.paircount(RADII),
                "B": lambda: np.array([int(within_only(nbx, c, r, within).sum(dtype=np.int64)) // 2 for r in RADII], dtype=np.uint64)}
        same = np.array_equal(arms["A"](), arms["B"]())
        us, passes = _time(arms, rounds, window)
    finally:
        c.close()
    return _cell("context", [n], us, passes, same)


def measure(nbx, kind, rounds=5, window=0.05):
    """Cells 2 and 3, kind "ensemble" or "ragged": one batch call against one nbx_paircount call per context."""
    assert rounds >= 5
    sizes = [TC.ENSEMBLE_N] * TC.MEMBERS if kind == "ensemble" else list(TC.RAGGED_SIZES)
    states = [TC.member_state(n, 1000 + k, np.float32) for k, n in enumerate(sizes)]
    batch = nbx.Ensemble(TC.ENSEMBLE_N, TC.MEMBERS, 32) if kind == "ensemble" else nbx.Ragged(sizes, 32)
    ctxs = []
    try:
        batch.upload(states)
        for n, s in zip(sizes, states):
            ctxs.append(nbx.Context(n, 32))
            ctxs[-1].upload(s)
        arms = {"A": lambda: batch.paircount(RADII), "B": lambda: np.stack([c.paircount(RADII) for c in ctxs])}
        same = np.array_equal(arms["A"](), arms["B"]())
        us, passes = _time(arms, rounds, window)
    finally:
        for o in [batch] + ctxs:
            o.close()
    return _cell(kind, sizes, us, passes, same)


def _with_scheme(scheme, run):
    def arm():
        old = os.environ.get(SCHEME)
        os.environ[SCHEME] = scheme
        try:
            return run()
        finally:
            if old is None:
                del os.environ[SCHEME]
            else:
                os.environ[SCHEME] = old
    return arm


def measure_large(nbx, n=LARGE_N, rounds=5, window=0.05):
    """The compute-bound cell: one context of n bodies, 16 radii under each scheme, one neighbours call with the count alone,
    and 20 radii against 16 under the compiled default."""
    assert rounds >= 5
    c = nbx.Context(n, 32)
    try:
        c.upload(TC.member_state(n, 999, np.float32))
        within = np.zeros(n, dtype=np.int32)
        arms = {"L": _with_scheme("lane", lambda: c.paircount(RADII)), "W": _with_scheme("wave", lambda: c.paircount(RADII)),
                "N": lambda: within_only(nbx, c, RADII[8], within), "P16": lambda: c.paircount(RADII), "P20": lambda: c.paircount(RADII20)}
        same = np.array_equal(arms["L"](), arms["W"]())
        us, passes = _time(arms, rounds, window)
    finally:
        c.close()
    med = {k: statistics.median(v) for k, v in us.items()}
    pairs = float(n) * (n - 1)
    return {"kind": "context", "n": n, "precision": 32, "nradii": len(RADII), "lane_us": med["L"], "wave_us": med["W"],
            "faster_scheme": "lane" if med["L"] <= med["W"] else "wave", "neighbours_count_us": med["N"],
            "against_one_neighbours_call": min(med["L"], med["W"]) / med["N"], "default_16_radii_us": med["P16"], "default_20_radii_us": med["P20"],
            "second_pass_ratio": med["P20"] / med["P16"], "lane_pairs_per_s": pairs / (med["L"] * 1e-6), "wave_pairs_per_s": pairs / (med["W"] * 1e-6),
            "rounds_us": us, "passes_per_round": passes, "same_values_from_both_schemes": bool(same)}


WHAT = ("us per pass, fp32, 16 radii; context: one nbx_paircount call against 16 nbx_neighbours calls (index and r2 NULL) on the same "
        "context of 8192 bodies plus the host sums; ensemble (16 x 2048) and ragged (16 sizes over 512 ... 4096): one batch call "
        "against one nbx_paircount call on each of 16 default contexts created and uploaded beforehand; medians of the rounds, arms "
        "alternated, one process; ratio = A / B (each gated <= 1.0 by tests/test_paircount_gpu.py); context_n131072: one call under "
        "each counting scheme, one nbx_neighbours call with the count alone, 20 radii against 16 (recorded)")


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
    print("%-10s %10s %10s %8s" % ("cell", "A us", "B us", "ratio"))
    for kind in ("context", "ensemble", "ragged"):
        r = measure_context(nbx, rounds=a.rounds, window=a.window) if kind == "context" else measure(nbx, kind, rounds=a.rounds, window=a.window)
        us = [v for k, v in r.items() if k.endswith("_us") and not k.endswith("rounds_us")]
        print("%-10s %10.1f %10.1f %8.3f%s" % (kind, us[0], us[1], r["ratio"], "" if r["same_values_from_both_arms"] else "  VALUES DIFFER"), flush=True)
        write(a.out, {kind: r})
    r = measure_large(nbx, rounds=a.rounds, window=a.window)
    print("context n = %d, 16 radii: lane counters %.1f us, wave counters %.1f us (%s is faster), one neighbours count %.1f us, "
          "20 radii %.1f us against 16 radii %.1f us" % (r["n"], r["lane_us"], r["wave_us"], r["faster_scheme"], r["neighbours_count_us"],
                                                         r["default_20_radii_us"], r["default_16_radii_us"]), flush=True)
    write(a.out, {"context_n%d" % r["n"]: r})
    print("wrote", a.out)


if __name__ == "__main__":
    main()
