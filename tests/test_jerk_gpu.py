"""The acceleration of every body and its time derivative on the device (include/nbx_jerk.h) against the numpy reference
tests/jerk_ref.py, as a context, as members of an ensemble and as members of one ragged ensemble.

What is asked of every result (jerk_ref.compare): every component of acc and jerk within its gate, K = |got - truth| / (u scale)
<= 2 max(K_ref, floor, 16), K_ref that of the restatement in T on the same state and floor the per-term bound the header
derives, never a device value; where the scale is 0 an exact zero.  acc is bit for bit field()'s at the bodies' own positions;
a member's six arrays are a lone context's.  The largest K seen per precision and output goes to profiles/jerk_error.json with
its gate.

Shapes, the smallest at which each part can go wrong: n = 1, 2, 3, 5; 257 (one column, two tiles with 255 padding records), 513
(a second column of one body), 2049 (five columns, two splits of 5 and 4 tiles), 4097 (nine columns, four splits, the last one
short), an ensemble of 3 x 2049, a ragged ensemble of (5, 2049, 257, 1, 513), and the lattice of 35 937 bodies (71 columns x 15
splits) in v = H x + Omega x x, in natural and permuted order, at about 1000 sampled rows, and the lattice of 531 441 bodies (1038
columns of one split) at 256 rows in fp32 and 64 in fp64."""
import ctypes
import json
import os
import sys
import zlib

import numpy as np
import pytest

import jerk_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

ERROR_FILE = os.path.join(ROOT, "profiles", "jerk_error.json")
_ctx, _worst = {}, {}


def same(a, b, keys=R.KEYS):
    """Bit for bit (values compared as bytes: -0.0 and 0.0 differ, NaN equals itself)."""
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)


def context_values(nbx, precision, n, family):
    """What a default context of n bodies holding the family's state returns, asked once: the bits the members are held to.  Two
    calls in a row give the same bits, and acc is field()'s at the bodies' own positions on the same object."""
    key = (precision, n, family)
    if key not in _ctx:
        st = R.case(precision, n, family)["state"]
        with nbx.Context(n, precision) as ctx:
            ctx.upload(st)
            got = ctx.jerk()
            assert same(ctx.jerk(), got), key
            assert same(ctx.field(st["pos_x"], st["pos_y"], st["pos_z"]), got, R.ACC), key
        _ctx[key] = got
    return _ctx[key]


def _record(precision, ks, gates, where):
    for k, v in ks.items():
        key = "fp%d %s" % (precision, k)
        if v > _worst.get(key, {"K": -1.0})["K"]:
            _worst[key] = {"K": v, "gate": gates[k], "case": where}
    out = {"what": ("largest K = |got - truth| / (u scale) of nbx_jerk / nbx_ensemble_jerk / nbx_ragged_jerk against the reference "
                    "tests/jerk_ref.py seen by tests/test_jerk_gpu.py, per precision and output, with the gate of the case it was seen "
                    "in: force_ref.M * max(K_ref, floor, force_ref.K_TERM)")}
    if os.path.exists(ERROR_FILE):
        with open(ERROR_FILE) as f:
            out.update({k: v for k, v in json.load(f).items() if k != "what"})
    for k, v in _worst.items():
        if v["K"] >= out.get(k, {"K": -1.0})["K"]:
            out[k] = v
    os.makedirs(os.path.dirname(ERROR_FILE), exist_ok=True)
    with open(ERROR_FILE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def check(got, c, precision, where):
    n = len(c["state"]["mass"])
    assert all(got[k].dtype == R.DTYPE[precision] and got[k].shape == (n,) for k in R.KEYS)
    problems, ks = R.compare(R.at_rows(got, c["truth"]["rows"]), c["truth"], c["gates"], precision)
    print("fp%d %s: K %s; gates %s" % (precision, where, {k: round(v, 2) for k, v in ks.items()}, {k: round(v, 1) for k, v in c["gates"].items()}))
    _record(precision, ks, c["gates"], where)
    assert not problems, (precision, where, problems)


@pytest.mark.parametrize("n,family", R.context_cases())
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference_and_acc_is_the_fields(nbx, precision, n, family):
    c = R.case(precision, n, family)
    got = context_values(nbx, precision, n, family)
    check(got, c, precision, "%s(%d)" % (family, n))
    if family == "rest":  # a state at rest: exact zeros
        assert all((got[k] == 0).all() for k in R.JERK) and any((got[k] != 0).any() for k in R.ACC)
    if n == 1:
        assert all((got[k] == 0).all() for k in R.KEYS)


@pytest.mark.parametrize("precision", [32, 64])
def test_one_exactly_representable_velocity_added_to_every_body_changes_no_bit(nbx, precision):
    n = 2049
    st = R.case(precision, n, "grid")["state"]
    with nbx.Context(n, precision) as ctx:
        ctx.upload(R.shifted(st))
        assert same(ctx.jerk(), context_values(nbx, precision, n, "grid"))


@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_reference_and_have_the_bits_of_a_context(nbx, precision):
    S, n = R.ENSEMBLE
    cases = [R.case(precision, n, f) for f in R.ENSEMBLE_FAMILIES]
    with nbx.Ensemble(n, S, precision) as e:
        e.upload([c["state"] for c in cases])
        full = e.jerk()
        assert same(e.jerk(), full) and all(full[k].shape == (S, n) for k in R.KEYS)
        for m, f in enumerate(R.ENSEMBLE_FAMILIES):
            got = {k: full[k][m] for k in R.KEYS}
            check(got, cases[m], precision, "ensemble %s(%d)" % (f, n))
            assert same(got, context_values(nbx, precision, n, f)), (precision, f)
        fld = e.field(*[np.stack([c["state"][p] for c in cases]) for p in R.POS])
        assert same(fld, full, R.ACC)
        for first, count in ((1, 2), (0, 1), (1, 1), (2, 1), (0, 2), (S, 0), (0, 0)):  # whatever range a member is asked in
            part = e.jerk(first=first, count=count)
            assert same(part, {k: full[k][first:first + count] for k in R.KEYS}), (first, count)


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = R.RAGGED_SIZES
    S = len(sizes)
    cases = [R.case(precision, n, "cloud") for n in sizes]
    with nbx.Ragged(sizes, precision) as r:
        r.upload([c["state"] for c in cases])
        full = r.jerk()
        assert len(full) == S and all(same(a, b) for a, b in zip(r.jerk(), full))
        for m, n in enumerate(sizes):
            check(full[m], cases[m], precision, "ragged cloud(%d)" % n)
            assert same(full[m], context_values(nbx, precision, n, "cloud")), (precision, n)
        for first, count in ((3, 2), (1, 3), (S - 1, 1), (0, 1), (2, 2), (S, 0), (3, 0)):
            part = r.jerk(first=first, count=count)
            assert len(part) == count and all(same(a, b) for a, b in zip(part, full[first:first + count])), (first, count)
        # the layout is end to end, member `first` at element 0; a NULL array is skipped alone; nothing is written behind the last member
        first, count = 1, 3
        total = sum(sizes[first:first + count])
        flat = {k: np.full(total + 8, -7, dtype=R.DTYPE[precision]) for k in R.KEYS}
        a = [flat[k].ctypes.data for k in R.KEYS]
        out = nbx.JerkOut((ctypes.c_void_p * 3)(a[0], None, a[2]), (ctypes.c_void_p * 3)(None, a[4], a[5]))
        assert nbx.load().nbx_ragged_jerk(r._h, first, count, ctypes.byref(out)) == nbx.NBX_OK
        for k in R.KEYS:
            if k in ("acc_y", "jerk_x"):
                assert (flat[k] == -7).all(), k  # never written
                continue
            assert np.array_equal(flat[k][:total], np.concatenate([full[m][k] for m in range(first, first + count)])), k
            assert (flat[k][total:] == -7).all(), k
        assert nbx.load().nbx_ragged_jerk(r._h, 0, S, ctypes.byref(nbx.JerkOut())) == nbx.NBX_OK  # nothing asked for
    with nbx.Ragged(sizes[::-1], precision) as r:  # the same systems in another order: other offsets, other rows, the same bits
        r.upload([c["state"] for c in cases][::-1])
        assert all(same(a, b) for a, b in zip(r.jerk(), full[::-1]))


@pytest.mark.parametrize("precision", [32, 64])
def test_a_velocity_that_is_not_finite_in_the_next_member_does_not_reach_the_member_before_it(nbx, precision):
    """257 bodies: 255 padding records whose velocities, were they loaded, would be the next member's first ones."""
    n = 257
    st = R.case(precision, n, "cloud")["state"]
    bad = {k: v.copy() for k, v in st.items()}
    bad["vel_x"][0], bad["vel_y"][0], bad["vel_z"][0] = np.inf, np.nan, -np.inf
    want = context_values(nbx, precision, n, "cloud")
    with nbx.Ensemble(n, 2, precision) as e:
        e.upload([st, bad])
        got = e.jerk()
        assert same({k: got[k][0] for k in R.KEYS}, want)
        assert not np.isfinite(got["jerk_x"][1]).all()  # unspecified, for that system alone
    with nbx.Ragged([n, n], precision) as r:
        r.upload([st, bad])
        assert same(r.jerk()[0], want) and same(r.jerk(first=0, count=1)[0], want)


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_of_71_columns_and_15_splits_in_hubble_flow_and_rotation(nbx, precision, perm):
    n = R.LATTICE_K ** 3
    assert R.FR.field_shape(n, n) == (71, 141, 15, 10)
    c = R.lattice_case(precision, perm)
    rows = c["truth"]["rows"]
    assert 900 <= len(rows) <= 1100 and {0, n - 1, 511, 512, 10 * 256 - 1, 10 * 256} <= set(rows.tolist())
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        got = ctx.jerk()
    check(got, c, precision, "lattice perm=%d (%d)" % (perm, n))


@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_of_1038_columns_of_one_split(nbx, precision):
    """531 441 bodies: one split of 2076 tiles, so a body's sums are 531 456 sequential terms in T -- K_ref, the restatement's, says
    what that order costs, and the gate follows it."""
    n = R.LARGE_K ** 3
    assert R.FR.field_shape(n, n) == (1038, 2076, 1, 2076)
    c = R.large_case(precision)
    rows = c["truth"]["rows"]
    assert len(rows) == R.LARGE_ROWS[precision] and {0, n - 1, 511, 512, 1037 * 512 - 1, 1037 * 512} <= set(rows.tolist())
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        got = ctx.jerk()
    check(got, c, precision, "lattice (%d)" % n)


def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


@pytest.mark.parametrize("precision", [32, 64])
def test_the_call_leaves_the_trajectory_and_the_counters_alone_and_is_ordered_after_the_steps(nbx, precision):
    n, dt = 2049, 1.0 / 4096
    st = R.case(precision, n, "cloud")["state"]
    with nbx.Context(n, precision) as ctx:
        ctx.upload(st)
        ctx.step(3, dt, kenergy=False)  # asynchronous: nothing waits for the steps before the call
        got = ctx.jerk()
        before, down = ctx.stats(), ctx.download()
        again = ctx.jerk()
        after, down2 = ctx.stats(), ctx.download()
        assert same(got, again) and before["steps_done"] == after["steps_done"] == 3 and _crc(down.values()) == _crc(down2.values())
        assert not same(got, context_values(nbx, precision, n, "cloud"), R.JERK)  # the state after the steps
        ke_a = ctx.step(3, dt)
        a = ctx.download()
    with nbx.Context(n, precision) as ctx:
        ctx.upload(st)
        ctx.step(3, dt)
        mid = ctx.download()
        ke_b = ctx.step(3, dt)
        b = ctx.download()
    assert _crc(a.values()) == _crc(b.values()) and ke_a == ke_b  # a following step is as without the call
    with nbx.Context(n, precision) as ctx:  # the state the asynchronous steps led to, uploaded: the same bits
        ctx.upload(dict(mid, mass=st["mass"]))
        assert same(ctx.jerk(), got)


def test_state_and_argument_errors(nbx):
    n = 2049
    st = R.case(32, n, "cloud")["state"]
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.jerk()
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_jerk: nbx_upload has not been called" in str(err.value)
        c.upload(R.make_state(32, 300, "cloud"))
        assert np.isfinite(c.jerk()["jerk_x"]).all()
        assert nbx.load().nbx_jerk(c._h, None) == nbx.NBX_ERR_ARG and nbx.load().nbx_last_error().decode() == "nbx_jerk: out is NULL"
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.jerk()
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_jerk: a local step awaits nbx_commit" in str(err.value)
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # the velocities of the others are not resident in a slice
        with nbx.Context(n, 32, i_begin=i_begin, i_count=i_count, n_alloc=2304) as ctx:
            ctx.upload(st)
            with pytest.raises(nbx.NbxError) as err:
                ctx.jerk()
            assert err.value.code == nbx.NBX_ERR_STATE
            assert "nbx_jerk: the context owns a slice of the bodies (the velocities of the others are not resident)" in str(err.value)
    with nbx.Ensemble(300, 4, 32) as e:
        with pytest.raises(nbx.NbxError) as err:
            e.jerk()
        assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value)
        for first, count in ((-1, 1), (0, 5), (4, 1)):
            with pytest.raises(nbx.NbxError) as err:
                e.jerk(first=first, count=count)
            assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value)


def test_hermite_on_an_ensemble_is_of_fourth_order_and_follows_the_numpy_restatement(nbx):
    """An fp64 ensemble of the two systems of the CPU test, T = 0.25 in 16 and in 32 steps against 256 steps (dt / 16), all on the
    device: the error ratio of a fourth-order scheme is 16 and of a second-order one 4; 8, their geometric mean, separates
    them.  The end state is the numpy restatement's at the same dt to within the restatement's own distance from its dt / 16
    run: rounding differences between the two evaluations of a and adot are many orders below that."""
    states = [R.hermite_state(seed) for seed in R.HERMITE_SEEDS]
    n, n1 = len(states[0]["mass"]), R.HERMITE_STEPS
    ends = {}
    with nbx.Ensemble(n, 2, 64) as e:
        for steps in (n1, 2 * n1, 16 * n1):
            e.upload(states)
            done = e.stats()["steps_done"]
            out = nbx.hermite(e, R.HERMITE_T / steps, steps)
            assert e.stats()["steps_done"] == done  # not counted
            down = e.download()
            assert all(np.array_equal(down[f], out[0][f]) for f in R.POS + R.VEL)  # the corrected state is resident
            ends[steps] = [{f: down[f][m] for f in R.POS + R.VEL} for m in range(2)]
        assert nbx.hermite(e, 0.01, 0) is None
    for m, seed in enumerate(R.HERMITE_SEEDS):
        e1, e2 = (R.state_error(ends[s][m], ends[16 * n1][m]) for s in (n1, 2 * n1))
        ref1 = R.hermite(states[m], R.HERMITE_T / n1, n1)
        own = R.state_error(ref1, R.hermite(states[m], R.HERMITE_T / (16 * n1), 16 * n1))
        away = R.state_error(ends[n1][m], ref1)
        print("seed %d: device errors %.3g %.3g ratio %.1f; from the numpy restatement %.3g, whose own error is %.3g" % (seed, e1, e2, e1 / e2, away, own))
        assert e1 / e2 >= 8.0, (seed, e1, e2)
        assert away <= own, (seed, away, own)
    # a context and a ragged ensemble take the same steps: the same jerk bits and the same host arithmetic give the same end state
    with nbx.Context(n, 64) as c:
        c.upload(states[0])
        nbx.hermite(c, R.HERMITE_T / n1, n1)
        down = c.download()
        assert all(np.array_equal(down[f], ends[n1][0][f]) for f in R.POS + R.VEL)
    with nbx.Ragged([n, n], 64) as r:
        r.upload(states)
        nbx.hermite(r, R.HERMITE_T / n1, n1)
        for m, down in enumerate(r.download()):
            assert all(np.array_equal(down[f], ends[n1][m][f]) for f in R.POS + R.VEL), m


def test_jerk_dt_of_a_device_result_is_the_first_order_criterion(nbx):
    got = context_values(nbx, 32, 513, "cloud")
    dt = nbx.jerk_dt(got, 0.02)
    a = np.sqrt(sum(got[k].astype(np.float64) ** 2 for k in R.ACC))
    j = np.sqrt(sum(got[k].astype(np.float64) ** 2 for k in R.JERK))
    assert dt.shape == (513,) and np.array_equal(dt, 0.02 * a / j) and (dt > 0).all()
    assert np.isinf(nbx.jerk_dt(context_values(nbx, 32, 513, "rest"), 0.02)).all()


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32: one batch call against 16
    nbx_jerk calls on contexts created and uploaded beforehand, in this process, rounds alternated (tools/jerk_cost.py).
    ratio <= 1.0, the condition every batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jerk_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = jerk_cost.measure(nbx, kind)
        print("%s fp32: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["batch_us"], r["contexts_us"], r["ratio"]))
        cells[kind] = r
    jerk_cost.write(jerk_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_bits_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
