"""record_group_shares.py -- writes tests/golden/group_shares.json: what the share planner of the groups gave BEFORE it moved to
csrc/nbx_shares.hpp.  Run it with the library built at the commit before that move (NBX_LIB=<that libnbx.so>), never with a later
one: tests/test_shares_cpu.py and the replay in tests/test_parity_gpu.py hold the planner to this recording.

`partition`: nbx_partition, nbx_partition_weighted and nbx_tune_weights -- host arithmetic, the same on any machine -- over the
parameter list of tests/test_weighted_partition.py plus 200 seeded random cases, and the inputs they refuse.
`retune`: nbx_group_retune on an MI355X (its cu_count is stored: the cost model reads it).  Logical ranks on device 0, synthetic
force_ms only, nothing stepped -- create, upload, retune -- so every decision is deterministic; after each call the `changed` flag
and nbx_group_shares.  One scenario per branch of the decision.
usage (GPU box): NBX_LIB=old/libnbx.so python tools/record_group_shares.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-demo-2023_amd"))
import nbx  # noqa: E402
import numpy as np  # noqa: E402

# tests/test_weighted_partition.py::test_every_body_has_one_owner_and_blocks_are_whole_tiles, and the sizes of its other tests
LISTED = [(1048576, 8, None), (1048576, 8, [1, 1, 1, 1, 1, 1, 1, 0.9]), (262144, 4, [1, 2, 1, 3]), (5001, 3, [1, 2, 1]),
          (2000, 8, [5, 1, 1, 1, 1, 1, 1, 1]), (300, 8, None), (256, 2, [1, 1]), (257, 2, [1, 1000]), (1, 4, None),
          (4099, 5, [0.3, 0.1, 0.2, 0.25, 0.15]), (1048576, 2, None), (1048576, 4, None), (5000, 3, [1, 2, 1])]
# arguments are JSON: the non-finite weights and times are strings that float() reads
REFUSED = [("partition", [0, 4, 0]), ("partition", [100, 0, 0]), ("partition", [100, 4, 4]), ("partition", [100, 4, -1]),
           ("partition_weighted", [0, 4, None, 0]), ("partition_weighted", [100, 0, None, 0]), ("partition_weighted", [100, 4, None, 4]),
           ("partition_weighted", [100, 4, None, -1]), ("partition_weighted", [5000, 3, [1, 0, 1], 0]),
           ("partition_weighted", [5000, 3, [1, -1, 1], 0]), ("partition_weighted", [5000, 3, [1, "nan", 1], 0]),
           ("partition_weighted", [5000, 3, [1, "inf", 1], 2]), ("partition_weighted", [5000, 3, ["-inf", 1, 1], 1]),
           ("tune_weights", [[100, 0], [1.0, 1.0]]), ("tune_weights", [[100, -5], [1.0, 1.0]]), ("tune_weights", [[100, 100], [1.0, 0.0]]),
           ("tune_weights", [[100, 100], [-1.0, 1.0]]), ("tune_weights", [[100, 100], [1.0, "nan"]]),
           ("tune_weights", [[100, 100], ["inf", 1.0]]), ("tune_weights", [[], []])]
# name, n, precision, ranks, weights (None: equal), options, the force_ms of each nbx_group_retune call
SCENARIOS = [
    ("shares below one workgroup per CU: the model sees no gain, kept", 5001, 32, 3, [1, 2, 1], {"summation_order": nbx.ORDER_REFERENCE}, [[1, 8, 1]]),
    ("one workgroup per CU everywhere: refused by the prediction", 262144, 32, 4, None, {}, [[4.30, 4.70, 4.70, 4.70]]),
    ("a move that pays", 262144, 32, 3, [1, 2, 1], {}, [[1, 8, 1]]),
    ("move, taken back, frozen", 20000, 32, 2, None, {"summation_order": nbx.ORDER_TREE}, [[1, 2], [3.0, 0.5], [1, 2]]),
    ("move, kept fixed point, then on", 20000, 32, 2, None, {"summation_order": nbx.ORDER_TREE}, [[1, 2], [1.3, 1.3], [1.0, 1.3]]),
    ("move, kept, then a slow window: the move before the last is no longer judged", 20000, 32, 2, None, {"summation_order": nbx.ORDER_TREE},
     [[1, 2], [1.3, 1.3], [2.5, 1.0]]),
    ("the window after a move 1.005 times slower: not taken back", 20000, 32, 2, None, {"summation_order": nbx.ORDER_TREE},
     [[1, 2], [2 * 1.005, 2 * 1.005], [1, 2]]),
    ("the window after a move 1.02 times slower: taken back", 20000, 32, 2, None, {"summation_order": nbx.ORDER_TREE},
     [[1, 2], [2 * 1.02, 2 * 1.02], [1, 2]]),
    ("fp64 move", 20000, 64, 2, [1, 3], {}, [[1, 9]]),
    ("two tiles for eight ranks: ranks dropped, nothing finer to move", 300, 32, 8, None, {}, [[1, 2]]),
    ("the one-tile floor: nothing finer to move", 257, 32, 2, [1, 1000], {}, [[2, 1]]),
]


def _floats(x):
    return None if x is None else [float(v) for v in x]


def call(name, args):
    """One of the three host functions with JSON arguments -> its result, or ["E", code, text of nbx_last_error()]."""
    try:
        if name == "partition":
            return list(nbx.partition(*args))
        if name == "partition_weighted":
            return list(nbx.partition_weighted(args[0], args[1], _floats(args[2]), args[3]))
        return nbx.tune_weights(args[0], _floats(args[1]))
    except nbx.NbxError as e:
        return ["E", e.code, nbx.load().nbx_last_error().decode()]


def partition_case(rng, n, P, w):
    """Every rank's answer of both partitions, and nbx_tune_weights on the weighted shares with seeded times."""
    eq = [call("partition", [n, P, r]) for r in range(P)]
    wt = [call("partition_weighted", [n, P, w, r]) for r in range(P)]
    assert all(e[:2] == eq[0][:2] and e[4] == eq[0][4] for e in eq) and all(x[0] == wt[0][0] and x[3] == wt[0][3] for x in wt)
    used = wt[0][0]
    count = [x[2] for x in wt[:used]]
    ms = [float(t) for t in rng.uniform(0.5, 5.0, used)]
    return {"n": n, "ranks": P, "weights": w,
            "equal": {"ranks_used": eq[0][0], "block": eq[0][1], "n_alloc": eq[0][4], "begin": [e[2] for e in eq], "count": [e[3] for e in eq]},
            "weighted": {"ranks_used": used, "n_alloc": wt[0][3], "begin": [x[1] for x in wt], "count": [x[2] for x in wt]},
            "force_ms": ms, "tuned": call("tune_weights", [count, ms])}


def record_partition():
    rng = np.random.default_rng(20261018)
    cases = [partition_case(rng, n, P, _floats(w)) for n, P, w in LISTED]
    for _ in range(200):
        n, P = int(rng.integers(1, 300001)), int(rng.integers(1, 17))
        cases.append(partition_case(rng, n, P, [float(x) for x in rng.uniform(0.05, 5.0, P)]))
    refused = [{"call": name, "args": args, "refusal": call(name, args)[1:]} for name, args in REFUSED]
    assert all(len(r["refusal"]) == 2 and isinstance(r["refusal"][1], str) for r in refused), refused
    return {"cases": cases, "refused": refused}


def record_retune():
    out = []
    for name, n, precision, ranks, weights, opts, calls in SCENARIOS:
        with nbx.Group(n, precision, n_ranks=ranks, devices=[0] * ranks, weights=weights, weighted=True, **opts) as g:
            g.upload(nbx.initial_conditions(n, precision))
            cus = g.info(0)[2]["cu_count"]
            b0, c0, _ = g.shares(timings=False)
            steps = []
            for ms in calls:
                ms = [float(t) for t in ms]
                changed = g.retune(ms)
                b, c, _ = g.shares(timings=False)
                steps.append({"force_ms": ms, "changed": int(changed), "begin": b, "count": c})
        out.append({"name": name, "n": n, "precision": precision, "ranks": ranks, "weights": _floats(weights), "opts": opts,
                    "begin": b0, "count": c0, "calls": steps})
        print("%-70s %s" % (name, [(s["changed"], s["count"]) for s in steps]), flush=True)
    return cus, out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "group_shares.json")
    part = record_partition()
    cus, retune = record_retune()
    doc = {"about": "Shares of the groups, recorded by tools/record_group_shares.py from the library before the share planner moved to "
                    "csrc/nbx_shares.hpp.  partition: nbx_partition (equal), nbx_partition_weighted (weighted; begin and count of every rank "
                    "asked, n and 0 for the dropped ones) and nbx_tune_weights (tuned, from the weighted counts of the used ranks and "
                    "force_ms), or [code, text] where they refuse.  retune: nbx_group_retune on an MI355X, logical ranks on device 0; the "
                    "changed flag and nbx_group_shares after every call.",
           "cu_count": cus, "partition": part, "retune": retune}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in doc.items() if k not in ("partition", "retune")))
        f.write(",\n\"partition\": {\"cases\": [\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in part["cases"]))
        f.write("\n], \"refused\": [\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in part["refused"]))
        f.write("\n]},\n\"retune\": [\n" + ",\n".join(json.dumps(s, separators=(",", ":")) for s in retune) + "\n]}\n")
    json.load(open(path))
    print("wrote %s: %d partition cases, %d refusals, %d retune scenarios, cu_count %d" % (path, len(part["cases"]), len(part["refused"]), len(retune), cus))
