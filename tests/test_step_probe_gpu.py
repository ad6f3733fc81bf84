"""The zero-velocity probe: every step kernel, per body, against a high-precision direct sum (tests/force_ref.py).

Upload a state with all velocities zero and take one step.  euler_update rounds like the reference, so v1 = fl(a dt) exactly,
where a is the acceleration the STEP kernel applied to that body: v1 / dt gives it back to half an ulp.  That makes the per-body
acceleration of every compiled step instance observable through the public API -- row epilogue, time-sliced and prefetch loops,
two records per operation, one-launch kernels, LDS, fp64, slabs plus integrate_kernel, slices through nbx_step_local / nbx_commit,
ensemble members -- where nbx_accel only ever launches the slab form with the plain hand-scheduled loop.

Per case: nbx_stats names the intended instance; K_i = max_c |a_i - truth| / (u_T A_i) stays under the gate 2 max(K_ref, 16)
(force_ref: K_ref is the CPU oracle's K on the same state and bodies, never a kernel's) on every owned body (n <= 16384) or on
256 sampled bodies (large shapes); p1 == fl(p0 + fl(v1 dt)) bit for bit; the returned energy equals 0.5 sum m v1^2 of the
downloaded velocities to 1e-13; the same bodies through nbx_accel under the same gate; and v1 == fl(accel dt) bit for bit where
step and accel kernels share the summation order (one-launch kernels, single-split shapes).

Measured on an MI355X when this module was written (every K on the device was unmeasured before it): the worst K / gate of
all cases is 0.53.  Reference-order shapes sit at K_ref to three digits (n = 262144 default: 406.2 against 406.2; 131072 of
1048576: 4761 against 4760), tree-order shapes far below it (n = 262144 tree: 9.9).  v1 == fl(accel dt) held on every case,
the split shapes included.  The fp64 kernels failed it as first written -- K = 38.4 against the gate 32 on bodies 18 and 40 of
the adversarial n = 63 state, whose acceleration is one dominant term: one Newton step on v_rsq_f64 left 4e-15 on the
inverse cube -- and pass at K <= 6.7 there since gm_inv_cube<double> (csrc/nbx_pair.hpp).  The module runs in 11 s.

CASES is also fed to the host-only planner by tests/test_step_probe_cpu.py, which checks that it reaches all 56 step instances.
Every case's K_max, median K, K_ref, gate and instance go to step_probe.json in the GPU suite's report directory (OUT of
tests/test_parity_gpu.py).
"""
import json
import os

import numpy as np
import pytest

import energy_ref
import force_ref as R

pytestmark = pytest.mark.gpu

# nbx.h values, spelled out so that the table can be read without the library
KV_LDS, KV_SGPR, KV_SGPRW, KV_JLANE = 1, 2, 3, 6
ORDER_REFERENCE, ORDER_TREE = 1, 2
INST_FORCE, INST_JLANE, INST_EXACT = 0, 1, 2
JSRC_LDS, JSRC_SGPR = 1, 2
EPI_SLAB, EPI_ROW = 0, 1
LOOP_CXX, LOOP_ASM, LOOP_TS, LOOP_PF = 0, 1, 2, 3  # the plan's; nbx_opts.inner_loop and nbx_stats say loop + 1

OPT_FIELDS = ("i_begin", "i_count", "n_alloc", "bodies_per_lane", "j_split", "kernel_variant", "fused_epilogue", "use_graph",
              "external_stream", "summation_order", "inner_loop")


def step_instances():
    """The 56 step instances of csrc/nbx_plan.hpp (kInstances without the four INST_EXACT rows), as
    (kind, precision, B, jsrc, epi, math, ws, loop), written out independently of the header."""
    out = []
    for prec, bs in ((32, (1,)), (64, (1, 2, 4)), (32, (2, 4))):  # compiled loop, wave split and plain
        for B in bs:
            math = 1 if (prec == 32 and B >= 2) else 0
            out.append((INST_FORCE, prec, B, JSRC_SGPR, EPI_SLAB, math, 1, LOOP_CXX))
            for jsrc in (JSRC_SGPR, JSRC_LDS):
                for epi in (EPI_ROW, EPI_SLAB):
                    out.append((INST_FORCE, prec, B, jsrc, epi, math, 0, LOOP_CXX))
    for jsrc in (JSRC_SGPR, JSRC_LDS):  # fp32, eight bodies per lane: no wave split
        for epi in (EPI_ROW, EPI_SLAB):
            out.append((INST_FORCE, 32, 8, jsrc, epi, 1, 0, LOOP_CXX))
    for epi in (EPI_ROW, EPI_SLAB):  # two j records per packed operation
        out.append((INST_FORCE, 32, 1, JSRC_SGPR, epi, 0, 0, LOOP_ASM))
    for B in (2, 4):  # hand-scheduled loops
        out.append((INST_FORCE, 32, B, JSRC_SGPR, EPI_SLAB, 1, 1, LOOP_ASM))
        for epi in (EPI_ROW, EPI_SLAB):
            out.append((INST_FORCE, 32, B, JSRC_SGPR, epi, 1, 0, LOOP_ASM))
        for loop in (LOOP_TS, LOOP_PF):
            out.append((INST_FORCE, 32, B, JSRC_SGPR, EPI_ROW, 1, 0, loop))
    for B in (2, 4, 8):  # one launch per step
        out.append((INST_JLANE, 32, B, 0, 0, 0, 0, LOOP_ASM))
        out.append((INST_JLANE, 32, B, 0, 0, 0, 0, LOOP_CXX))
        out.append((INST_JLANE, 64, B, 0, 0, 0, 0, LOOP_CXX))
    out.append((INST_JLANE, 32, 16, 0, 0, 0, 0, LOOP_CXX))
    return out


def instance_name(k):
    kind, prec, B, jsrc, epi, math, ws, loop = k
    lp = ("cxx", "asm", "ts", "pf")[loop]
    if kind == INST_JLANE:
        return "jlane-f%d-nb%d-%s" % (prec, B, lp)
    return "force-f%d-b%d-%s%s-%s-%s" % (prec, B, "lds" if jsrc == JSRC_LDS else "sgpr", "w" if ws else "", "row" if epi == EPI_ROW else "slab", lp)


def instance_from_stats(st):
    """The kernel instance nbx_stats describes (plan_instance of nbx_plan.hpp, from the public fields)."""
    loop = st["inner_loop"] - 1
    if st["kernel_variant"] == KV_JLANE:
        return (INST_JLANE, st["precision"], st["bodies_per_lane"], 0, 0, 0, 0, loop)
    B = st["bodies_per_lane"]
    return (INST_FORCE, st["precision"], B, JSRC_LDS if st["kernel_variant"] == KV_LDS else JSRC_SGPR, st["fused_epilogue"],
            1 if (st["precision"] == 32 and B >= 2) else 0, 1 if st["kernel_variant"] == KV_SGPRW else 0, loop)


def shape_opts(k, n_alloc, single_split_slab=False):
    """nbx_opts that make nbx_create plan instance k for a record array of n_alloc."""
    kind, prec, B, jsrc, epi, math, ws, loop = k
    o = dict(bodies_per_lane=B, inner_loop=loop + 1)
    if kind == INST_JLANE:
        o["kernel_variant"] = KV_JLANE
    elif ws:  # the hand-scheduled loop needs j_per_split % 256 == 0: one tile per split; the compiled one takes ragged splits
        o.update(kernel_variant=KV_SGPRW, j_split=(n_alloc // 256 if loop == LOOP_ASM else 3))
    else:
        o["kernel_variant"] = KV_LDS if jsrc == JSRC_LDS else KV_SGPR
        if epi == EPI_ROW:
            o["summation_order"] = ORDER_REFERENCE
        elif single_split_slab:  # one chain per body into one slab, integrate_kernel on top
            o.update(summation_order=ORDER_REFERENCE, fused_epilogue=2)
        else:
            o.update(summation_order=ORDER_TREE, j_split=3, fused_epilogue=2)
    return o


def _round_up(a, b):
    return -(-a // b) * b


SLICE = dict(i_begin=1000, i_count=2077, n_alloc=4608)  # of n = 4099: ragged on both ends, one spare tile of records


def instance_cases(idx, k):
    """The probes of one instance: below a tile, ragged with all five families, a whole multiple of 256, and a slice."""
    small = 5 if idx % 2 else 63
    cases = []
    for n, fams, sl, single in ((small, ("seed42", "adversarial"), {}, False), (4099, R.FAMILIES, {}, False),
                                (1024, ("seed42", "adversarial"), {}, True), (4099, ("seed42", "adversarial"), SLICE, False)):
        n_alloc = sl.get("n_alloc", _round_up(n, 256))
        opts = dict(shape_opts(k, n_alloc, single), **sl)
        for fam in fams:
            cases.append(dict(n=n, precision=k[1], family=fam, opts=opts, inst=k))
    return cases


# Shapes as nbx_create picks them with no option given, where every owned body is still affordable
DEFAULT_CASES = [dict(n=n, precision=prec, family=fam, opts={}, inst=inst)
                 for n, prec, inst in ((16384, 32, (INST_FORCE, 32, 4, JSRC_SGPR, EPI_SLAB, 1, 1, LOOP_ASM)),
                                       (4099, 32, (INST_JLANE, 32, 2, 0, 0, 0, 0, LOOP_CXX)),
                                       (4099, 64, (INST_JLANE, 64, 2, 0, 0, 0, 0, LOOP_CXX)))
                 for fam in ("seed42", "adversarial")]

# Large shapes as they run in production, 256 sampled owned bodies each (`stats`: what nbx_stats must show besides the instance)
LARGE_CASES = [
    dict(id="n262144-default", n=262144, precision=32, family="seed42", opts={}, inst=(INST_FORCE, 32, 2, JSRC_SGPR, EPI_ROW, 1, 0, LOOP_TS),
         stats=dict(kernel_variant=KV_SGPR, fused_epilogue=EPI_ROW, inner_loop=LOOP_TS + 1, force_grid_x=512, force_grid_y=1)),
    dict(id="n262144-default-adversarial", n=262144, precision=32, family="adversarial", opts={},
         inst=(INST_FORCE, 32, 2, JSRC_SGPR, EPI_ROW, 1, 0, LOOP_TS), stats=dict(force_grid_x=512)),
    dict(id="131072-of-1048576", n=1048576, precision=32, family="seed42", opts=dict(i_begin=917504, i_count=131072),
         inst=(INST_FORCE, 32, 2, JSRC_SGPR, EPI_ROW, 1, 0, LOOP_PF), stats=dict(force_grid_x=256)),
    dict(id="65536-of-262144", n=262144, precision=32, family="seed42", opts=dict(i_begin=65536, i_count=65536),
         inst=(INST_FORCE, 32, 1, JSRC_SGPR, EPI_ROW, 0, 0, LOOP_ASM), stats=dict(force_grid_x=256)),
    dict(id="32768-of-262144", n=262144, precision=32, family="seed42", opts=dict(i_begin=229376, i_count=32768),
         inst=(INST_FORCE, 32, 1, JSRC_SGPR, EPI_ROW, 0, 0, LOOP_ASM), stats=dict(force_grid_x=128)),
    dict(id="n262144-tree", n=262144, precision=32, family="seed42", opts=dict(summation_order=ORDER_TREE),
         inst=(INST_FORCE, 32, 4, JSRC_SGPR, EPI_SLAB, 1, 1, LOOP_ASM), stats=dict(j_split=8)),
    dict(id="n65536-default", n=65536, precision=32, family="seed42", opts={}, inst=(INST_FORCE, 32, 4, JSRC_SGPR, EPI_SLAB, 1, 1, LOOP_ASM),
         stats=dict(kernel_variant=KV_SGPRW, j_split=2)),
    dict(id="f64-n16384", n=16384, precision=64, family="seed42", opts={}, inst=(INST_FORCE, 64, 4, JSRC_SGPR, EPI_SLAB, 0, 1, LOOP_CXX), stats={}),
]

INSTANCES = step_instances()
CASES = [c for idx, k in enumerate(INSTANCES) for c in instance_cases(idx, k)] + DEFAULT_CASES + LARGE_CASES


def planner_row(case):
    """The case as a line of tests/plan_driver.cpp's stdin."""
    o = case["opts"]
    return "%d %d %s 0" % (case["n"], case["precision"], " ".join(str(o.get(f, 0)) for f in OPT_FIELDS))


def bodies_per_workgroup(k):
    kind, prec, B, jsrc, epi, math, ws, loop = k
    return 4 * B if kind == INST_JLANE else (64 if ws else 256) * B


def sample_bodies(i_begin, i_count, per_wg, count=256, seed=5):
    """`count` owned bodies: the first and last of the slice and of the first and last workgroups, both neighbours of every
    tile edge next to those, and seeded random ones in between."""
    lo, hi = i_begin, i_begin + i_count
    last_wg = lo + (i_count - 1) // per_wg * per_wg
    s = {lo, hi - 1, lo + per_wg - 1, lo + per_wg, last_wg - 1, last_wg, lo + 255, lo + 256, hi - 257, hi - 256}
    s.update((_round_up(lo + 1, 256) - 1, _round_up(lo + 1, 256), (hi - 1) // 256 * 256 - 1, (hi - 1) // 256 * 256))
    s = {i for i in s if lo <= i < hi}
    rng = np.random.default_rng([seed, i_begin, i_count])
    while len(s) < min(count, i_count):
        s.update(int(i) for i in rng.integers(lo, hi, count - len(s)))
    return np.array(sorted(s), dtype=np.int64)


# ---- truth, cached per (family, n, precision) -------------------------------------------------------------------------------------
_STATES, _REFS = {}, {}
RECORDS = []


def state_of(oracle, family, n, precision):
    key = (family, n, precision)
    if key not in _STATES:
        _STATES[key] = R.make_state(oracle, family, n, precision)
    return _STATES[key]


def reference_of(oracle, family, n, precision, rows=None):
    """(truth, K of the oracle per body) for all bodies (rows None) or for the sampled `rows`."""
    key = (family, n, precision, None if rows is None else rows.tobytes())
    if key not in _REFS:
        st = state_of(oracle, family, n, precision)
        tr = R.state_truth(st, rows)
        _REFS[key] = (tr, R.k_metric(R.oracle_accel(oracle, st, rows), tr, precision))
    return _REFS[key]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    from test_parity_gpu import OUT  # where the GPU suite leaves its reports
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "step_probe.json"), "w") as f:
        json.dump({"gate": "K_max <= %g * max(K_ref, %g)" % (R.M, R.K_TERM), "cases": RECORDS}, f, indent=1)


def _xyz(d, pre, rows):
    return np.stack([np.asarray(d[pre + c])[rows] for c in "xyz"], axis=1)


def check_gate(label, K, rows, k_ref, rec, what):
    g = R.gate(k_ref)
    rec.update({what + "_K_max": float(K.max()), what + "_K_median": float(np.median(K))})
    print("%-70s %-5s K_max %8.1f  median %6.1f  K_ref %7.1f  gate %7.1f" % (label, what, K.max(), np.median(K), k_ref, g))
    bad = np.flatnonzero(~(K <= g))
    assert bad.size == 0, "%s (%s): %d bodies over the gate %.1f (K_ref %.1f); worst %s" % (
        label, what, bad.size, g, k_ref, [(int(rows[i]), float(K[i])) for i in bad[np.argsort(-K[bad])][:10]])


def probe(nbx, oracle, case, rows=None, label=None):
    n, precision, family, opts, inst = case["n"], case["precision"], case["family"], case["opts"], case["inst"]
    st0 = state_of(oracle, family, n, precision)
    lo = opts.get("i_begin", 0)
    cnt = opts.get("i_count", 0) or n - lo
    sliced = (lo, cnt) != (0, n)
    label = label or "%s n=%d%s %s" % (instance_name(inst), n, " [%d,+%d)" % (lo, cnt) if sliced else "", family)
    with nbx.Context(n, precision, **opts) as c:
        st = c.stats()
        assert instance_from_stats(st) == inst, (label, instance_name(instance_from_stats(st)), st)
        for f, v in case.get("stats", {}).items():
            assert st[f] == v, (label, f, st[f], v)
        if rows is None:
            assert n <= 16384
            tr_all, kref_all = reference_of(oracle, family, n, precision)
            rows = np.arange(lo, lo + cnt)
            tr, kref = tuple(t[rows] for t in tr_all), kref_all[rows]
        else:
            assert rows.min() >= lo and rows.max() < lo + cnt
            tr, kref = reference_of(oracle, family, n, precision, rows)
        k_ref = float(kref.max())
        c.upload(st0)
        acc = c.accel()
        if sliced:
            c.step_local()
            c.commit()
            ke = 0.5 * c.kenergy_partial()
        else:
            ke = c.step(1)
        d = c.download()
    rec = dict(case=label, instance=instance_name(inst), n=n, precision=precision, family=family, i_begin=lo, i_count=cnt,
               bodies=int(len(rows)), K_ref=k_ref, gate=R.gate(k_ref), j_split=st["j_split"])
    RECORDS.append(rec)
    # the step kernel, per body
    v1 = _xyz(d, "vel_", rows)
    check_gate(label, R.k_metric(R.accel_from_v1(v1, precision), tr, precision), rows, k_ref, rec, "step")
    # the position update is an identity in T
    own = np.arange(lo, lo + cnt)
    for ax in "xyz":
        want = R.position_identity(st0["pos_" + ax][own], d["vel_" + ax][own], precision)
        bad = np.flatnonzero(d["pos_" + ax][own] != want)
        assert bad.size == 0, (label, "pos_" + ax, "p1 != fl(p0 + fl(v1 dt)) at bodies", (own[bad][:10]).tolist())
    rest = np.setdiff1d(np.arange(n), own)
    for ax in "xyz":
        assert np.array_equal(d["pos_" + ax][rest], st0["pos_" + ax][rest]), (label, "a body outside the slice moved")
    # the energy the step returned is the one of the velocities it left behind
    want_ke = energy_ref.diagnostics(dict(d, mass=st0["mass"]), lo, cnt, potential_too=False)["kenergy"]
    rec["kenergy_rel_err"] = abs(ke - want_ke) / want_ke if want_ke else float(ke != 0)
    assert abs(ke - want_ke) <= 1e-13 * abs(want_ke), (label, ke, want_ke)
    # the slab form nbx_accel launches, under the same gate
    a = np.stack([np.asarray(x)[rows] for x in acc], axis=1)
    check_gate(label, R.k_metric(a, tr, precision), rows, k_ref, rec, "accel")
    T = st0["mass"].dtype.type
    same = np.array_equal((a * T(R.DT)).astype(T), v1)
    rec["v1_equals_accel_dt"] = bool(same)
    if inst[0] == INST_JLANE or st["j_split"] == 1:  # same summation order in both kernels
        assert same, (label, "v1 != fl(accel dt) at bodies", rows[np.flatnonzero(((a * T(R.DT)).astype(T) != v1).any(axis=1))][:10].tolist())
    return rec


# ---- every step instance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(INSTANCES)), ids=[instance_name(k) for k in INSTANCES])
def test_step_instance_per_body(nbx, oracle, idx):
    """K on every owned body of every probe of this instance, then the hand-placed systems with closed forms."""
    k = INSTANCES[idx]
    for case in instance_cases(idx, k):
        probe(nbx, oracle, case)
    # hand-placed systems with closed forms; a body nothing pulls at (A == 0) must stay exactly at rest
    for name, st0, want in R.hand_placed(k[1]):
        n = len(st0["mass"])
        with nbx.Context(n, k[1], **shape_opts(k, 256)) as c:
            assert instance_from_stats(c.stats()) == k, (name, c.stats())
            c.upload(st0)
            c.step(1)
            d = c.download()
        tr = R.state_truth(st0)
        assert R.k_metric(want, tr, k[1]).max() <= 4, (name, "the closed form itself")
        K = R.k_metric(R.accel_from_v1(_xyz(d, "vel_", np.arange(n)), k[1]), (want, np.zeros_like(want), tr[2]), k[1])
        assert (K <= R.gate(0)).all(), (instance_name(k), name, K.tolist())
        for ax in "xyz":
            assert np.array_equal(d["pos_" + ax], R.position_identity(st0["pos_" + ax], d["vel_" + ax], k[1])), (instance_name(k), name, ax)


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=["n%d-f%d-%s" % (c["n"], c["precision"], c["family"]) for c in DEFAULT_CASES])
def test_default_shapes_per_body(nbx, oracle, case):
    probe(nbx, oracle, case)


@pytest.mark.parametrize("case", LARGE_CASES, ids=[c["id"] for c in LARGE_CASES])
def test_large_shapes_as_they_run_in_production(nbx, oracle, case):
    """256 sampled owned bodies: the first and last body of the slice and of the first and last workgroups, both neighbours of
    the tile edges, the rest seeded."""
    lo = case["opts"].get("i_begin", 0)
    cnt = case["opts"].get("i_count", 0) or case["n"] - lo
    rows = sample_bodies(lo, cnt, bodies_per_workgroup(case["inst"]))
    assert len(rows) == 256 and {lo, lo + cnt - 1, lo + 255, lo + 256} <= set(rows.tolist())
    probe(nbx, oracle, case, rows, label=case["id"])


# ---- ensemble members -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, dict(bodies_per_lane=16)], ids=["default", "nb16"])
def test_ensemble_members_per_body(nbx, oracle, opts):
    """Five members of n = 2000, one family each (adversarial last), one step from rest: every body of every member under the gate."""
    n, fams = 2000, ("seed42", "offset1000", "lattice", "signedbox", "adversarial")
    states = [state_of(oracle, f, n, 32) for f in fams]
    with nbx.Ensemble(n, len(fams), 32, **opts) as e:
        st = e.stats()
        if opts:
            assert st["bodies_per_lane"] == opts["bodies_per_lane"], st
        e.upload(states)
        ke = e.step(1)
        d = e.download()
    inst = (INST_JLANE, 32, st["bodies_per_lane"], 0, 0, 0, 0, st["inner_loop"] - 1)
    assert inst in INSTANCES, st
    rows = np.arange(n)
    for m, fam in enumerate(fams):
        tr, kref = reference_of(oracle, fam, n, 32)
        label = "ensemble[%s] member %d %s n=%d" % (instance_name(inst), m, fam, n)
        rec = dict(case=label, instance="ensemble-" + instance_name(inst), n=n, precision=32, family=fam, i_begin=0, i_count=n, bodies=n,
                   K_ref=float(kref.max()), gate=R.gate(kref.max()), j_split=1)
        RECORDS.append(rec)
        dm = {f: d[f][m] for f in d}
        check_gate(label, R.k_metric(R.accel_from_v1(_xyz(dm, "vel_", rows), 32), tr, 32), rows, float(kref.max()), rec, "step")
        for ax in "xyz":
            assert np.array_equal(dm["pos_" + ax], R.position_identity(states[m]["pos_" + ax], dm["vel_" + ax], 32)), (label, ax)
        want_ke = energy_ref.diagnostics(dict(dm, mass=states[m]["mass"]), potential_too=False)["kenergy"]
        assert abs(ke[m] - want_ke) <= 1e-13 * abs(want_ke), (label, ke[m], want_ke)
