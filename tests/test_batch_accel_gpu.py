"""nbx_ensemble_accel and nbx_ragged_accel on the device (include/nbx_batch_accel.h): every member's accelerations must be the
bits nbx_accel returns for a single one-launch context of the same shape, before and after steps and for every kernel
instance; a range must be the concatenation of its members, whatever was asked before; skipped arrays are never written; every
body of every member must lie under the project's per-body gate against a high-precision direct sum (tests/force_ref.py) that
does not involve the library; a call must leave no trace in the trajectory, the energies or the counters; the documented errors;
and one call over all members must cost no more than one nbx_accel call per member."""
import os
import sys

import numpy as np
import pytest

import force_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

ARRAYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z")

# n = 1 and 5: shadow bodies past the end of the only wave; 63, 64, 65: one wave's bodies short, full and one over; 257 (K = 8
# records per lane: one trip of the generated loop), 700 (K = 12: a trip plus the compiled remainder), 63 ... 256 (K = 4: no whole
# trip); 2048: more than one workgroup for every bodies-per-wave
ENSEMBLE_SIZES = (1, 5, 63, 64, 65, 257, 700, 2048)
RAGGED_MIXES = ((1, 63, 64, 65, 257, 700, 2048), (2048, 5, 2048, 700))

# every instance of kEnsembleInstances, by name, and the planner's own choice in each precision
OPTIONS = ([(32, dict(bodies_per_lane=NB, inner_loop="LOOP_CXX")) for NB in (2, 4, 8, 16)] +
           [(32, dict(bodies_per_lane=NB, inner_loop="LOOP_ASM")) for NB in (2, 4, 8)] +
           [(64, dict(bodies_per_lane=NB)) for NB in (2, 4, 8)] + [(32, {}), (64, {})])
OPTION_IDS = ["f%d-%s" % (p, "-".join(str(v).replace("LOOP_", "").lower() for v in o.values()) or "auto") for p, o in OPTIONS]


def _opts(nbx, opts):
    return {k: (getattr(nbx, v) if isinstance(v, str) else v) for k, v in opts.items()}


def member_states(nbx, sizes, precision):
    """As member_states of test_ragged_gpu.py: member k = the next sizes[k] bodies of the seed-42 system of sum(sizes) bodies; the
    last member is the seed-42 system of its own size."""
    big = nbx.initial_conditions(sum(sizes), precision)
    at = np.concatenate([[0], np.cumsum(sizes)])
    states = [{f: big[f][at[k]:at[k + 1]].copy() for f in nbx.FIELDS} for k in range(len(sizes))]
    states[-1] = nbx.initial_conditions(sizes[-1], precision)
    return states


def context_accels(nbx, n, precision, state, NB, loop, steps):
    """[ax, ay, az] of a one-launch context of that shape at the uploaded state and after `steps` steps."""
    with nbx.Context(n, precision, kernel_variant=nbx.KERNEL_JLANE, bodies_per_lane=NB, inner_loop=loop, use_graph=2) as c:
        st = c.stats()
        assert st["kernel_variant"] == nbx.KERNEL_JLANE and st["bodies_per_lane"] == NB and st["inner_loop"] == loop
        assert st["force_grid_x"] == -(-(-(-n // NB)) // 4) and st["force_grid_y"] == 1
        c.upload(state)
        a0 = c.accel()
        c.step(steps, kenergy=False)
        a1 = c.accel()
    return a0, a1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def per_member(nbx, batch, acc):
    """Ensemble.accel's three (count, n) arrays as Ragged.accel's list of [ax, ay, az] per member."""
    if isinstance(batch, nbx.Ensemble):
        return [[a[m] for a in acc] for m in range(acc[0].shape[0])]
    return acc


def make_batch(nbx, sizes, precision, **opts):
    """An ensemble where all sizes are equal and the caller asks for one (sizes given as (n, members)), else a ragged ensemble."""
    if isinstance(sizes, tuple) and len(sizes) == 2 and sizes[0] == "ensemble":
        n, S = sizes[1]
        return nbx.Ensemble(n, S, precision, **opts), [n] * S
    return nbx.Ragged(sizes, precision, **opts), list(sizes)


def assert_members_equal_contexts(nbx, spec, precision, opts, steps=3):
    batch, sizes = make_batch(nbx, spec, precision, **_opts(nbx, opts))
    states = member_states(nbx, sizes, precision)
    with batch:
        st = batch.stats()
        for k, v in _opts(nbx, opts).items():
            assert st[k] == v, (k, st)
        batch.upload(states)
        a0 = per_member(nbx, batch, batch.accel())
        batch.step(steps, kenergy=False)
        a1 = per_member(nbx, batch, batch.accel())
    NB, loop = st["bodies_per_lane"], st["inner_loop"]
    done = {}
    for m, n in enumerate(sizes):
        assert [x.shape for x in a0[m]] == [(n,)] * 3 and [x.dtype for x in a1[m]] == [states[m]["mass"].dtype] * 3
        c0, c1 = context_accels(nbx, n, precision, states[m], NB, loop, steps)
        for c in range(3):
            assert same_bits(a0[m][c], c0[c]), (spec, m, n, "xyz"[c], NB, loop, "after 0 steps")
            assert same_bits(a1[m][c], c1[c]), (spec, m, n, "xyz"[c], NB, loop, "after %d steps" % steps)
        done[n] = float(max(np.abs(x).max() for x in c1))
    assert all(v > 0 for n, v in done.items() if n > 1)  # not zeros against zeros
    return st


@pytest.mark.parametrize("precision,opts", OPTIONS, ids=OPTION_IDS)
def test_ensemble_members_are_bit_equal_to_a_single_context(nbx, precision, opts):
    for n in ENSEMBLE_SIZES:
        assert_members_equal_contexts(nbx, ("ensemble", (n, 3)), precision, opts)


@pytest.mark.parametrize("sizes", RAGGED_MIXES, ids=["seven-sizes", "two-large-twice"])
@pytest.mark.parametrize("precision,opts", OPTIONS, ids=OPTION_IDS)
def test_ragged_members_are_bit_equal_to_a_single_context(nbx, precision, opts, sizes):
    st = assert_members_equal_contexts(nbx, sizes, precision, opts)
    assert st["grid_x"] > len(sizes)  # members of more than one workgroup


# ---------------------------------------------------------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------------------------------------------------------
RANGE_BATCHES = [(("ensemble", (700, 5)), 32), (("ensemble", (65, 4)), 64), ((257, 1, 700, 2048, 5), 32), ((2048, 5, 2048, 700), 64)]
RANGE_IDS = ["ensemble-f32", "ensemble-f64", "ragged-f32", "ragged-f64"]


@pytest.mark.parametrize("spec,precision", RANGE_BATCHES, ids=RANGE_IDS)
def test_a_range_is_the_concatenation_of_its_members_whatever_was_asked_before(nbx, spec, precision):
    batch, sizes = make_batch(nbx, spec, precision)
    M = len(sizes)
    states = member_states(nbx, sizes, precision)
    with batch:
        batch.upload(states)
        batch.step(2, kenergy=False)
        last_first = per_member(nbx, batch, batch.accel(M - 1, 1))  # the first call of the object's life is a range at the end
        full = per_member(nbx, batch, batch.accel())
        singles = [per_member(nbx, batch, batch.accel(k, 1))[0] for k in range(M)]
        middle = per_member(nbx, batch, batch.accel(1, 2))          # "[1, 3)"
        tail = per_member(nbx, batch, batch.accel(first=2))         # count = None: all from `first`
        again = per_member(nbx, batch, batch.accel())
        empty = batch.accel(1, 0)
    assert len(full) == M and len(middle) == 2 and len(tail) == M - 2 and len(last_first) == 1
    if isinstance(batch, nbx.Ensemble):
        assert [a.shape for a in empty] == [(0, sizes[0])] * 3
    else:
        assert empty == []
    for k in range(M):
        for c in range(3):
            assert same_bits(full[k][c], singles[k][c]) and same_bits(full[k][c], again[k][c]), (k, c)
    for c in range(3):
        assert same_bits(last_first[0][c], full[M - 1][c]), c
        for j in range(2):
            assert same_bits(middle[j][c], full[1 + j][c]), (j, c)
        for j in range(M - 2):
            assert same_bits(tail[j][c], full[2 + j][c]), (j, c)
    assert all(np.abs(np.stack(full[k])).max() > 0 for k in range(M) if sizes[k] > 1)


@pytest.mark.parametrize("spec,precision", RANGE_BATCHES, ids=RANGE_IDS)
def test_skipped_arrays_and_empty_ranges_are_never_written(nbx, spec, precision):
    """Through the C entry point itself, with host arrays prefilled with a sentinel."""
    batch, sizes = make_batch(nbx, spec, precision)
    states = member_states(nbx, sizes, precision)
    first, count = 1, 2
    total = sum(sizes[first:first + count])
    T = states[0]["mass"].dtype
    sentinel = T.type(-7.25)
    with batch:
        batch.upload(states)
        full = per_member(nbx, batch, batch.accel(first, count))
        want = [np.concatenate([full[j][c] for j in range(count)]) for c in range(3)]

        def call(first, count, mask):
            arrs = [np.full(total + 3, sentinel, dtype=T) for _ in range(3)]
            batch._accel(first, count, [a if keep else None for a, keep in zip(arrs, mask)])
            return arrs

        for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
            arrs = call(first, count, mask)
            for c in range(3):
                if mask[c]:
                    assert same_bits(arrs[c][:total], want[c]), (mask, c)
                    assert (arrs[c][total:] == sentinel).all(), (mask, c, "written past the range")
                else:
                    assert (arrs[c] == sentinel).all(), (mask, c, "a skipped array was written")
        for first_, count_, mask in ((first, count, (0, 0, 0)), (first, 0, (1, 1, 1)), (len(sizes), 0, (1, 1, 1)), (0, 0, (0, 0, 0))):
            arrs = call(first_, count_, mask)  # NBX_OK
            assert all((a == sentinel).all() for a in arrs), (first_, count_, mask)


# ---------------------------------------------------------------------------------------------------------------------------
# independent of the library: every body of every member against the high-precision direct sum
# ---------------------------------------------------------------------------------------------------------------------------
def probe_population(oracle, precision):
    """(label, state) per member: the families with coincident bodies, a dominant close pair and twelve decades of mass
    (adversarial, at a size below a wave's worth of records per lane and at one with a remainder), cancelling sums (lattice),
    lost low bits (offset1000), both signs (signedbox), the reference's own cloud, and the four hand-placed systems."""
    pop = [("%s n=%d" % (fam, n), R.make_state(oracle, fam, n, precision))
           for fam, n in (("adversarial", 63), ("adversarial", 700), ("seed42", 257), ("lattice", 343), ("offset1000", 300), ("signedbox", 65))]
    return pop + [(name, st) for name, st, _ in R.hand_placed(precision)]


_REFS = {}


def reference_of(oracle, label, state, precision):
    """(truth, K of the CPU oracle per body), computed once per member and left unchanged."""
    key = (label, precision)
    if key not in _REFS:
        tr = R.state_truth(state)
        _REFS[key] = (tr, R.k_metric(R.oracle_accel(oracle, state), tr, precision))
    return _REFS[key]


def check_member(oracle, label, state, acc, precision):
    tr, kref = reference_of(oracle, label, state, precision)
    k_ref = float(kref.max())
    K = R.k_metric(np.stack(acc, axis=1), tr, precision)
    g = R.gate(k_ref)
    print("%-34s f%d  K_max %8.2f  median %6.2f  K_ref %7.2f  gate %7.2f" % (label, precision, K.max(), np.median(K), k_ref, g))
    bad = np.flatnonzero(~(K <= g))
    assert bad.size == 0, "%s: %d bodies over the gate %.1f (K_ref %.1f); worst %s" % (
        label, bad.size, g, k_ref, [(int(i), float(K[i])) for i in bad[np.argsort(-K[bad])][:10]])


@pytest.mark.parametrize("precision", [32, 64])
def test_every_body_of_every_ragged_member_against_the_direct_sum(nbx, oracle, precision):
    pop = probe_population(oracle, precision)
    with nbx.Ragged([len(st["mass"]) for _, st in pop], precision) as r:
        r.upload([st for _, st in pop])
        acc = r.accel()
    for (label, st), a in zip(pop, acc):
        check_member(oracle, label, st, a, precision)


@pytest.mark.parametrize("precision", [32, 64])
def test_every_body_of_every_ensemble_member_against_the_direct_sum(nbx, oracle, precision):
    n = 700
    fams = ("adversarial", "seed42", "lattice", "offset1000", "signedbox")
    states = [R.make_state(oracle, f, n, precision) for f in fams]
    with nbx.Ensemble(n, len(fams), precision) as e:
        e.upload(states)
        acc = e.accel()
    for m, fam in enumerate(fams):
        check_member(oracle, "%s n=%d" % (fam, n), states[m], [a[m] for a in acc], precision)


# ---------------------------------------------------------------------------------------------------------------------------
# no side effects
# ---------------------------------------------------------------------------------------------------------------------------
def counters(st):
    return st["steps_done"], st["launches_timed"]  # the step kernel's: the accel launch is neither a step nor timed


@pytest.mark.parametrize("spec,precision", RANGE_BATCHES, ids=RANGE_IDS)
def test_a_call_leaves_no_trace(nbx, spec, precision):
    """A twin that never calls accel: the energies step(0) reports, the counters, and positions, velocities and the energy trace
    of 10 further steps are the same bits."""
    a, sizes = make_batch(nbx, spec, precision)
    b, _ = make_batch(nbx, spec, precision)
    states = member_states(nbx, sizes, precision)
    M = len(sizes)
    with a, b:
        for o in (a, b):
            o.upload(states)
            o.profile(True)
        a.accel()                                         # before any step: there are no partials yet
        assert same_bits(a.step(0), np.zeros(M)) and same_bits(b.step(0), np.zeros(M))
        for o in (a, b):
            o.step(3, kenergy=False)
        before, st_before = a.step(0), a.stats()
        a.accel(1, 2)
        a.accel()
        after, st_after = a.step(0), a.stats()
        assert same_bits(before, after) and same_bits(before, b.step(0)) and (before > 0).any()
        assert st_before == st_after and counters(st_after) == counters(b.stats()) == (3, 3)
        ke_a = a.step_trace(5)
        a.accel(M - 1, 1)                                 # between steps as well
        ke_a = np.concatenate([ke_a, a.step_trace(5)])
        ke_b = b.step_trace(10)
        out_a, out_b = a.download(), b.download()
        a.accel()
        assert same_bits(a.step(0), b.step(0))
        assert counters(a.stats()) == counters(b.stats()) == (13, 13)
    assert same_bits(ke_a, ke_b)
    if isinstance(a, nbx.Ensemble):
        assert all(same_bits(out_a[f], out_b[f]) for f in ARRAYS)
    else:
        assert all(same_bits(out_a[m][f], out_b[m][f]) for m in range(M) for f in ARRAYS)


# ---------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,precision", RANGE_BATCHES[::2], ids=RANGE_IDS[::2])
def test_range_and_state_errors(nbx, spec, precision):
    batch, sizes = make_batch(nbx, spec, precision)
    M = len(sizes)
    states = member_states(nbx, sizes, precision)
    name = batch._prefix + "_accel"
    with batch:
        batch.upload(states[:2])
        batch.upload(states[3:], first=3)                 # member 2 is missing
        for first, count in ((-1, 1), (0, M + 1), (M, 1), (M + 1, 0), (1, -1), (2, M - 1)):
            with pytest.raises(nbx.NbxError) as err:
                batch.accel(first, count)
            assert err.value.code == nbx.NBX_ERR_ARG and name + ": " in str(err.value), (first, count, str(err.value))
        for first, count in ((0, M), (2, 1), (1, 2), (2, M - 2)):
            with pytest.raises(nbx.NbxError) as err:
                batch.accel(first, count)
            assert err.value.code == nbx.NBX_ERR_STATE and name + ": member 2 has not been uploaded" in str(err.value), str(err.value)
        with pytest.raises(nbx.NbxError) as err:           # the state is looked at before the arrays: all three NULL is no way round it
            batch._accel(2, 1, [None, None, None])
        assert err.value.code == nbx.NBX_ERR_STATE
        # members outside the range need not have been uploaded
        low = per_member(nbx, batch, batch.accel(0, 2))
        high = per_member(nbx, batch, batch.accel(3, M - 3))
        assert per_member(nbx, batch, batch.accel(2, 0)) == [] and batch.accel(M, 0) is not None
        batch.upload(states[2:3], first=2)
        full = per_member(nbx, batch, batch.accel())
    for c in range(3):
        assert all(same_bits(low[k][c], full[k][c]) for k in range(2)) and all(same_bits(high[k][c], full[3 + k][c]) for k in range(M - 3))


# ---------------------------------------------------------------------------------------------------------------------------
# cost
# ---------------------------------------------------------------------------------------------------------------------------
def _cost_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import batch_accel_cost
    return batch_accel_cost


def test_one_ensemble_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 fp32: one nbx_ensemble_accel over all members against 16 nbx_accel calls on 16 contexts that were created and
    uploaded beforehand, in this process, rounds alternated (tools/batch_accel_cost.py).  The contexts are not charged for
    download, create or upload, so the gate has no further margin: ratio <= 1.0."""
    tool = _cost_tool()
    r = tool.measure_gate_ensemble(nbx)
    print("16 x 2048 fp32: ensemble %.1f us, 16 contexts %.1f us, ratio %.3f" % (r["batch_us"], r["contexts_us"], r["ratio"]))
    tool.write(tool.OUT, gate_ensemble=r)
    assert r["members"] == 16 and r["n_min"] == r["n_max"] == 2048 and r["arms_agree_to_rounding"], r
    assert r["ratio"] <= 1.0, r


def test_one_ragged_call_costs_no_more_than_one_call_per_context(nbx):
    """16 members spread evenly over 512 ... 4096, fp32: one nbx_ragged_accel against one nbx_accel call per member, as above."""
    tool = _cost_tool()
    r = tool.measure_gate_ragged(nbx)
    print("16 sizes over 512 ... 4096 fp32: ragged %.1f us, 16 contexts %.1f us, ratio %.3f" % (r["batch_us"], r["contexts_us"], r["ratio"]))
    tool.write(tool.OUT, gate_ragged=r)
    assert r["members"] == 16 and (r["n_min"], r["n_max"]) == (512, 4096) and r["arms_agree_to_rounding"], r
    assert r["ratio"] <= 1.0, r
