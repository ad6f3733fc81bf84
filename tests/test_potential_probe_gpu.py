"""The heavy-body probe: the potential-energy kernels (csrc/nbx_diag_body.hpp), per body and per pair, against a high-precision
direct sum (tests/potential_ref.py).

nbx_diag_t has one potential, the total; upload a state in which body k has mass 1 and every other body about 2^-40 and that
total is the row of k (the lane that holds k reading every record) plus the column of k (every other lane reading record k).
One pair dropped, doubled or wrongly masked moves it by 2^23 / n units of 2^-24 -- 2046 at n = 4099 -- where the gate is 32.
The launch shape depends on (i_count, n, precision) only, so one context per shape, uploaded again for every k, runs the
kernel as it runs in production: every probe is one nbx_upload and one nbx_diagnostics.

Per case K = |U - truth| / (u_T |truth|) <= 2 max(K_ref, 16) (force_ref.gate; K_ref is the K of potential_ref.Restatement, a numpy
restatement of the documented arithmetic, never a device value) on every body (n = 63, 1100), on about 160 positions -- body 0
and n - 1, both sides of every tile, column, lane-seam and j-split edge, seeded random ones -- of three bases at n = 2050 and
4099, and on slices with k inside and outside.  mass, kenergy == 0 and momentum == 0 hold exactly, mass_moment to 1e-12.  Then
single pairs against the closed form, the totals of the five force_ref families under the K gate, ensemble and ragged members
bit for bit against the contexts, and rank groups.

Measured on an MI355X when this module was written (no device value of K for the potential existed before it): nothing
failed, no kernel was changed.  The worst K / gate of all cases is 0.54, on the fp64 slice of one body, (5000, 300, 1): K = 20.1
against K_ref = 18.5, gate 37 -- one row, whose tile sum adds up to 255 light terms onto the heavy one and rounds each at its
size (tests/test_potential_probe_cpu.py explains and bounds it); it is the only case whose K_ref is above the 16-unit floor.
Everywhere else K / gate <= 0.18: heavy bodies K_max 3.2 in fp32 (K_ref 1.6 to 3.0, medians 0.2 to 0.7) and 5.9 in fp64 (K_ref
2.9 to 4.9, medians 1.1 to 1.6); family totals 2.2 and 2.7; rank groups 0.8 and 3.0.  The single pairs, i.e. the accuracy of one
pair term of the potential: K_max 1.97 in fp32 and 3.54 in fp64 (medians 0.49 and 1.07).  csrc/nbx_pair.hpp allows the one
Newton step on v_rsq_f64 a residual of up to 12 units; on these 64 pairs -- coincident, 1e-7 and 3e3 apart, masses 1 and 1e6 --
it stays under 4, so the fp64 branch of diag_tile keeps rsq() as it is.  The module runs in 9 s.

Every case's K_max, median K, K_ref and gate go to potential_probe.json in the GPU suite's report directory (OUT of
tests/test_parity_gpu.py).
"""
import json
import os

import numpy as np
import pytest

import force_ref as R
import potential_ref as P

pytestmark = pytest.mark.gpu

SLICE = dict(i_begin=1000, i_count=2077, n_alloc=4608)  # of n = 4099: SLICE of tests/test_step_probe_gpu.py


def _case(kind, n, precision, base, count=None, **sl):
    return dict(kind=kind, n=n, precision=precision, base=base, count=count, opts=sl)


EVERY_BODY = [_case("every body", n, p, "seed42") for n in (63, 1100) for p in (32, 64)]
SAMPLED = [_case("sampled", n, p, b, count=160) for n in (2050, 4099) for b in ("seed42", "offset1000", "adversarial") for p in (32, 64)]
SLICES = [_case("slice", n, p, "seed42", count=64, **sl) for n, sl in ((4099, SLICE), (5000, dict(i_begin=300, i_count=1))) for p in (32, 64)]
CASES = EVERY_BODY + SAMPLED + SLICES
FAMILY_CASES = [(n, p, f) for n in (63, 1100, 4099) for p in (32, 64) for f in R.FAMILIES]


def case_id(c):
    lo, cnt = case_slice(c)
    return "n%d-f%d-%s%s" % (c["n"], c["precision"], c["base"], "-%d+%d" % (lo, cnt) if c["opts"] else "")


def case_slice(c):
    lo = c["opts"].get("i_begin", 0)
    return lo, c["opts"].get("i_count", c["n"] - lo)


def case_positions(c):
    """The bodies k a case probes: all of them, or the edges of its launch shape plus seeded random ones."""
    lo, cnt = case_slice(c)
    return np.arange(c["n"]) if c["count"] is None else P.sample_positions(c["n"], lo, cnt, count=c["count"])


def case_reference(oracle, c, ks):
    """(truth (hi, lo), K_ref) of the heavy-body states of a case."""
    lo, cnt = case_slice(c)
    base = base_of(oracle, c["base"], c["n"], c["precision"])
    tr = P.truth_heavy(base, ks, c["precision"], lo, cnt)
    k_ref = P.k_metric(P.Restatement(base, c["precision"], lo, cnt).heavy_totals(ks), tr, c["precision"])
    return tr, float(k_ref.max())


# ---- shared state ------------------------------------------------------------------------------------------------------------------
_BASES, _CTX = {}, {}
RECORDS = []


def base_of(oracle, family, n, precision):
    key = (family, n, precision)
    if key not in _BASES:
        _BASES[key] = R.make_state(oracle, family, n, precision)
    return _BASES[key]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    from test_parity_gpu import OUT  # where the GPU suite leaves its reports
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "potential_probe.json"), "w") as f:
        json.dump({"gate": "K_max <= %g * max(K_ref, %g)" % (R.M, R.K_TERM), "cases": RECORDS}, f, indent=1)


def check_gate(label, n, precision, ks, K, k_ref):
    g = R.gate(k_ref)
    K = np.atleast_1d(K)
    RECORDS.append(dict(label=label, n=n, precision=precision, bodies=int(len(K)), K_max=float(K.max()), K_median=float(np.median(K)),
                        K_ref=float(k_ref), gate=g))
    print("%-44s n %5d fp%d  %4d probes  K_max %7.2f  median %6.2f  K_ref %6.2f  gate %5.1f" % (
        label, n, precision, len(K), K.max(), np.median(K), k_ref, g))
    bad = np.flatnonzero(~(K <= g))
    assert bad.size == 0, "%s: %d probes over the gate %.1f (K_ref %.2f); worst %s" % (
        label, bad.size, g, k_ref, [(ks[i], float(K[i])) for i in bad[np.argsort(-K[bad])][:10]])


def check_other_fields(label, k, d, st, lo, cnt):
    own = slice(lo, lo + cnt)
    m = st["mass"][own].astype(np.float64)
    assert d["mass"] == float(m.sum()), (label, k, d["mass"], float(m.sum()))  # every sum of these masses is exact in fp64
    assert d["kenergy"] == 0.0 and d["momentum"] == [0.0, 0.0, 0.0], (label, k, d)
    assert d["i_count"] == cnt and d["steps_done"] == 0, (label, k, d)
    for got, f in zip(d["mass_moment"], P.POS):
        x = st[f][own].astype(np.float64)
        assert abs(got - float((m * x).sum())) <= 1e-12 * float((m * np.abs(x)).sum()), (label, k, f, got)


def probe(nbx, oracle, c):
    n, precision = c["n"], c["precision"]
    lo, cnt = case_slice(c)
    label = "%s %s" % (c["kind"], case_id(c))
    ks = case_positions(c)
    tr, k_ref = case_reference(oracle, c, ks)
    got = np.zeros(len(ks))
    with nbx.Context(n, precision, device=0, **c["opts"]) as ctx:  # one context per shape
        for a, (k, st) in enumerate(P.heavy_states(base_of(oracle, c["base"], n, precision), ks, precision)):
            ctx.upload(st)
            d = ctx.diagnostics()
            got[a] = d["potential"]
            check_other_fields(label, k, d, st, lo, cnt)
            if not c["opts"]:
                _CTX[(c["base"], n, precision, k)] = d
    check_gate(label, n, precision, ks.tolist(), P.k_metric(got, tr, precision), k_ref)


def context_value(nbx, oracle, family, n, precision, k):
    """What a default context of n bodies returns for heavy_state(base, k): from the sweeps above where they ran, else asked now."""
    key = (family, n, precision, int(k))
    if key not in _CTX:
        with nbx.Context(n, precision, device=0) as ctx:
            ctx.upload(P.heavy_state(base_of(oracle, family, n, precision), int(k), precision))
            _CTX[key] = ctx.diagnostics()
    return _CTX[key]


# ---- heavy bodies ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EVERY_BODY, ids=case_id)
def test_every_body(nbx, oracle, case):
    """Every k of a one-tile system and of one with three columns, the last ragged: every lane t of a column, for both b."""
    probe(nbx, oracle, case)


@pytest.mark.parametrize("case", SAMPLED, ids=case_id)
def test_sampled_positions(nbx, oracle, case):
    """Two and four j splits with a ragged last split, a last column of 2 and of 3 bodies.  The adversarial base lends its
    positions only (coincident bodies, the outlier at 3e3); the masses are the probe's."""
    ks = set(case_positions(case).tolist())
    n, per = case["n"], P.diag_shape(case["n"], case["n"])[3]
    assert {0, n - 1, 255, 256, 511, 512, 767, 768, per * 256 - 1, per * 256, n // 512 * 512 - 1, n // 512 * 512} <= ks and len(ks) == 160
    probe(nbx, oracle, case)


@pytest.mark.parametrize("case", SLICES, ids=case_id)
def test_slices(nbx, oracle, case):
    """k at and next to both slice ends, inside and outside; for k outside, the partial is the owned part of k's column."""
    lo, cnt = case_slice(case)
    ks = set(case_positions(case).tolist())
    assert {lo - 1, lo, lo + cnt - 1, lo + cnt} <= ks and (cnt == 1 or {lo + 1, lo + cnt - 2} <= ks)
    probe(nbx, oracle, case)


# ---- single pairs ------------------------------------------------------------------------------------------------------------------
# n = 4099: 17 tiles, j splits of 5, 5, 5 and 2 tiles.  (k, j): one tile; the two bodies of one lane (j = k + 256), in the first and
# in a later column; across the lane seam and tile edge; across a column edge; first and last record of a split; across a split
# edge; first and last record of the ragged last split
PAIRS = [(10, 200), (5, 261), (767, 1023), (255, 256), (511, 512), (0, 1279), (1279, 1280), (3840, 4098)]
SEPARATIONS = (None, 0.0, 1e-7, 3e3)  # as the base places them; coincident; closer than eps by far; r >> eps
PAIR_CASES = [(k, j, sep, (1.0, 1e6) if (a + b) % 2 else (1e6, 1.0)) for a, (k, j) in enumerate(PAIRS) for b, sep in enumerate(SEPARATIONS)] + \
             [(k, j, sep, (1.0, 1.0)) for k, j in PAIRS for sep in SEPARATIONS]


@pytest.mark.parametrize("precision", [32, 64])
def test_single_pairs_against_the_closed_form(nbx, oracle, precision):
    """All masses 0 but two: U = -1/2 (m_k G m_j + m_j G m_k) / sqrt(r^2 + eps^2), gate 2 max(0, 16) = 32."""
    n = 4099
    base = base_of(oracle, "seed42", n, precision)
    assert len(PAIR_CASES) == 64
    K = np.zeros(len(PAIR_CASES))
    with nbx.Context(n, precision, device=0) as ctx:
        for a, (k, j, sep, (mk, mj)) in enumerate(PAIR_CASES):
            st = P.pair_state(base, k, j, precision, mk, mj, sep)
            ctx.upload(st)
            d = ctx.diagnostics()
            K[a] = P.k_metric(d["potential"], P.pair_truth(st, k, j), precision)[0]
            assert d["mass"] == mk + mj and d["kenergy"] == 0.0, (k, j, d)
    check_gate("single pairs", n, precision, PAIR_CASES, K, 0.0)


# ---- whole families ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,precision,family", FAMILY_CASES, ids=["n%d-f%d-%s" % c for c in FAMILY_CASES])
def test_family_totals(nbx, oracle, n, precision, family):
    """The total of a force_ref family with its own masses, under the K gate where tests/test_diagnostics_gpu.py asks 1e-5 / 1e-12."""
    st = base_of(oracle, family, n, precision)
    tr = P.truth_total(st, precision)
    k_ref = P.k_metric(P.restated(st, precision), tr, precision)[0]
    with nbx.Context(n, precision, device=0) as ctx:
        ctx.upload(st)
        d = ctx.diagnostics()
    check_gate("family total %s" % family, n, precision, [family], P.k_metric(d["potential"], tr, precision), k_ref)


# ---- batch objects and groups ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_return_the_contexts_bits(nbx, oracle, precision):
    n, ks = 1100, (0, 255, 256, 511, 512, 1023, 1024, 1099)
    base = base_of(oracle, "seed42", n, precision)
    with nbx.Ensemble(n, len(ks), precision) as e:
        e.upload([P.heavy_state(base, k, precision) for k in ks])
        d = e.diagnostics()
    for m, k in enumerate(ks):
        assert d[m] == context_value(nbx, oracle, "seed42", n, precision, k), (m, k)


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_return_the_contexts_bits(nbx, oracle, precision):
    sizes = (63, 1100, 2050, 513)
    bases = [base_of(oracle, "seed42", n, precision) for n in sizes]
    with nbx.Ragged(sizes, precision) as r:
        # first bodies; lane seam, column edge, split edge, tile edge; the other side of each; last bodies
        for ks in ((0, 0, 0, 0), (31, 511, 1279, 255), (32, 512, 1280, 256), (62, 1099, 2049, 512)):
            r.upload([P.heavy_state(b, k, precision) for b, k in zip(bases, ks)])
            d = r.diagnostics()
            for m, (n, k) in enumerate(zip(sizes, ks)):
                assert d[m] == context_value(nbx, oracle, "seed42", n, precision, k), (m, n, k)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("form", ["equal", "weighted"])
def test_rank_groups(nbx, oracle, form, precision):
    """Three logical ranks, k at each rank's first and last owned body: the group's total under the gate of the whole system."""
    n = 4099
    base = base_of(oracle, "seed42", n, precision)
    kw = dict(weights=[1, 2, 1]) if form == "weighted" else {}
    with nbx.Group(n, precision, n_ranks=3, devices=[0, 0, 0], **kw) as g:
        begin, count, _ = g.shares(timings=False)
        assert len(begin) == 3 and sum(count) == n
        ks = sorted({b for b in begin} | {b + c - 1 for b, c in zip(begin, count)})
        got = np.zeros(len(ks))
        for a, (k, st) in enumerate(P.heavy_states(base, ks, precision)):
            g.upload(st)
            d = g.diagnostics()
            got[a] = d["potential"]
            check_other_fields("group", k, d, st, 0, n)
    tr = P.truth_heavy(base, ks, precision)
    k_ref = P.k_metric(P.Restatement(base, precision).heavy_totals(ks), tr, precision).max()
    check_gate("group %s %s" % (form, list(zip(begin, count))), n, precision, ks, P.k_metric(got, tr, precision), k_ref)
