"""Clumps under a caller-supplied label on the device (include/nbx_clumps.h) against the numpy reference tests/clumps_ref.py, as
a context, as members of an ensemble and as members of one ragged ensemble.

What is asked of every result (clumps_ref.compare): members EQUALS the reference; every value within its gate, K = |got - truth|
/ (u scale) <= force_ref.M * max(K_ref, floor, force_ref.K_TERM), K_ref that of a sequential restatement in T and floor the
per-term bound the header derives (4.5 u and 53.5 u for phi and energy), never a device value; all members of a clump return the
same bits for members, gm, centre and velocity; a body alone is at itself exactly with phi = energy = 0; a body in no clump
returns zeros.  The largest K seen per precision and quantity goes to profiles/clumps_error.json with its gate.

Shapes, the smallest at which each part can go wrong: n = 1 and 2, 255, 256, 257 (one column, one split; one tile, a full tile,
two tiles with 255 padding records), 511, 512, 513 (the second body of a lane; two columns), 1025, 2049 (five columns, two splits
of 5 and 4 tiles), 4097 (nine columns, four splits, the last one short), an ensemble of 3 x 2049, a ragged ensemble of
neighbours_ref.RAGGED_SIZES, and the lattice of 35 937 bodies (71 columns x 15 splits) with `blocks` labels."""
import ctypes
import json
import os
import sys
import zlib

import numpy as np
import pytest

import clumps_ref as R
import fof_ref as FOF
import neighbours_ref as NB
from conftest import ROOT

pytestmark = pytest.mark.gpu

ERROR_FILE = os.path.join(ROOT, "profiles", "clumps_error.json")
_ctx, _worst = {}, {}


def same(a, b, keys=R.KEYS):
    """Bit for bit (values compared as bytes: -0.0 and 0.0 differ, NaN equals itself)."""
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)


def context_values(nbx, precision, n, family):
    """What a default context of n bodies holding cloud(n) returns under the family's labels, asked once: the bits the members
    are held to.  Two calls in a row and a bijective renaming of the labels give the same bits."""
    key = (precision, n, family)
    if key not in _ctx:
        c = R.case(precision, n, family)
        with nbx.Context(n, precision) as ctx:
            ctx.upload(c["state"])
            got = ctx.clumps(c["label"])
            assert same(ctx.clumps(c["label"]), got)
            assert same(ctx.clumps(R.renamed(c["label"])), got), (precision, n, family)
        _ctx[key] = got
    return _ctx[key]


def _record(precision, ks, gates, where):
    for k, v in ks.items():
        key = "fp%d %s" % (precision, k)
        if v > _worst.get(key, {"K": -1.0})["K"]:
            _worst[key] = {"K": v, "gate": gates[k], "case": where}
    out = {"what": ("largest K = |got - truth| / (u scale) of nbx_clumps / nbx_ensemble_clumps / nbx_ragged_clumps against the reference "
                    "tests/clumps_ref.py seen by tests/test_clumps_gpu.py, per precision and quantity, with the gate of the case it was "
                    "seen in: force_ref.M * max(K_ref, floor, force_ref.K_TERM)")}
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
    assert got["members"].dtype == np.int32 and all(got[k].dtype == R.DTYPE[precision] and got[k].shape == (n,) for k in R.FLOAT_KEYS)
    problems, ks = R.compare(got, c["truth"], c["gates"], c["state"], c["label"], precision)
    print("fp%d %s: K %s; gates %s" % (precision, where, {k: round(v, 2) for k, v in ks.items()}, {k: round(v, 1) for k, v in c["gates"].items()}))
    _record(precision, ks, c["gates"], where)
    assert not problems, (precision, where, problems)


@pytest.mark.parametrize("n,family", R.context_cases())
@pytest.mark.parametrize("precision", [32, 64])
def test_a_context_matches_the_reference(nbx, precision, n, family):
    c = R.case(precision, n, family)
    got = context_values(nbx, precision, n, family)
    check(got, c, precision, "%s(%d)" % (family, n))
    if family == "one" and n > 1:  # the potential energy of the whole system, 1/2 sum m_i phi_i
        m = c["state"]["mass"].astype(np.float64)
        phi, scale = c["truth"]["phi"]
        want = 0.5 * float((m * phi.astype(np.float64)).sum())
        bound = c["gates"]["phi"] * R.U[precision] * 0.5 * float((m * scale).sum())
        assert abs(0.5 * float((m * got["phi"].astype(np.float64)).sum()) - want) <= bound
    if family == "stripes" and n >= 255:
        assert (got["members"] == 0).sum() == (n + 1) // 11  # every 11th body is in no clump


@pytest.mark.parametrize("precision", [32, 64])
def test_with_the_labels_of_fof_members_is_its_size(nbx, precision):
    n = 2049
    st = R.cloud(n, precision)
    with nbx.Context(n, precision) as c:
        c.upload(st)
        groups = c.fof(FOF.target_radius(n, 1.0))
        got = c.clumps(groups["label"])
    assert np.array_equal(got["members"], groups["size"]) and 1 < groups["groups"] < n and (groups["size"] == 1).any()
    assert not R.same_bits_problems(got, groups["label"])


ENSEMBLE_FAMILIES = ("stripes", "fof", "blocks")


@pytest.mark.parametrize("precision", [32, 64])
def test_ensemble_members_match_the_reference_and_have_the_bits_of_a_context(nbx, precision):
    S, n = R.ENSEMBLE
    cases = [R.case(precision, n, f) for f in ENSEMBLE_FAMILIES]
    labels = np.stack([c["label"] for c in cases])
    with nbx.Ensemble(n, S, precision) as e:
        e.upload([c["state"] for c in cases])
        full = e.clumps(labels)
        assert same(e.clumps(labels), full) and all(full[k].shape == (S, n) for k in R.KEYS)
        for m, f in enumerate(ENSEMBLE_FAMILIES):
            got = {k: full[k][m] for k in R.KEYS}
            check(got, cases[m], precision, "ensemble %s(%d)" % (f, n))
            assert same(got, context_values(nbx, precision, n, f)), (precision, f)
        for first, count in ((1, 2), (0, 1), (1, 1), (2, 1), (0, 2), (S, 0), (0, 0)):  # whatever range a member is asked in
            part = e.clumps(labels[first:first + count], first=first, count=count)
            assert same(part, {k: full[k][first:first + count] for k in R.KEYS}), (first, count)
        assert same(e.clumps(labels), full)


@pytest.mark.parametrize("precision", [32, 64])
def test_ragged_members_match_the_reference_and_have_the_bits_of_a_context_of_their_size(nbx, precision):
    sizes = NB.RAGGED_SIZES
    S = len(sizes)
    cases = [R.case(precision, n, "stripes") for n in sizes]
    labels = [c["label"] for c in cases]
    with nbx.Ragged(sizes, precision) as r:
        r.upload([c["state"] for c in cases])
        full = r.clumps(labels)
        assert len(full) == S and all(same(a, b) for a, b in zip(r.clumps(labels), full))
        for m, n in enumerate(sizes):
            check(full[m], cases[m], precision, "ragged stripes(%d)" % n)
            assert same(full[m], context_values(nbx, precision, n, "stripes")), (precision, n)
        for first, count in ((3, 2), (2, 5), (S - 1, 1), (4, 1), (0, 1), (1, 3), (5, 3), (S, 0), (3, 0)):
            part = r.clumps(labels[first:first + count], first=first, count=count)
            assert len(part) == count and all(same(a, b) for a, b in zip(part, full[first:first + count])), (first, count)
        # the layout is end to end, member `first` at element 0; a NULL array is skipped alone; nothing is written behind the last member
        first, count = 2, 4
        total = sum(sizes[first:first + count])
        T = R.DTYPE[precision]
        flat = {k: np.full(total + 8, -7, dtype=np.int32 if k == "members" else T) for k in R.KEYS}
        a = [flat[k].ctypes.data for k in R.KEYS]
        out = nbx.ClumpsOut(a[0], None, (ctypes.c_void_p * 3)(*a[2:5]), (ctypes.c_void_p * 3)(a[5], None, a[7]), a[8], a[9])
        lab = np.ascontiguousarray(np.concatenate(labels[first:first + count]))
        assert nbx.load().nbx_ragged_clumps(r._h, first, count, lab.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out)) == nbx.NBX_OK
        for k in R.KEYS:
            if k in ("gm", "velocity_y"):
                assert (flat[k] == -7).all(), k  # never written
                continue
            assert np.array_equal(flat[k][:total], np.concatenate([full[m][k] for m in range(first, first + count)])), k
            assert (flat[k][total:] == -7).all(), k
        none = nbx.ClumpsOut()
        assert nbx.load().nbx_ragged_clumps(r._h, 0, S, lab.ctypes.data_as(ctypes.c_void_p), ctypes.byref(none)) == nbx.NBX_OK  # nothing asked for
    with nbx.Ragged(sizes[::-1], precision) as r:  # the same systems in another order: other offsets, other rows, the same bits
        r.upload([c["state"] for c in cases][::-1])
        assert all(same(a, b) for a, b in zip(r.clumps(labels[::-1]), full[::-1]))


@pytest.mark.parametrize("precision", [32, 64])
def test_the_lattice_of_71_columns_and_15_splits_with_block_labels(nbx, precision):
    n = R.LATTICE_K ** 3
    assert R.FR.field_shape(n, n) == (71, 141, 15, 10)
    rows = R.lattice_rows()
    c = R.case(precision, n, "blocks", state=R.lattice(precision), rows=rows, name="lattice")
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        got = ctx.clumps(c["label"])
    assert 900 <= len(rows) <= 1100
    check(got, c, precision, "lattice blocks(%d)" % n)  # phi and energy on `rows`, the group sums and members on all bodies


CONTEXT_OPTIONS = (
    [dict(kernel_variant=v, summation_order=o, bodies_per_lane=b) for v in ("KERNEL_LDS", "KERNEL_SGPR") for o in ("ORDER_TREE", "ORDER_REFERENCE")
     for b in (1, 4)] +
    [dict(kernel_variant="KERNEL_SGPRW", bodies_per_lane=2), dict(kernel_variant="KERNEL_JLANE", bodies_per_lane=4)] +
    [dict(j_split=s) for s in (1, 4, 32)] + [dict(kernel_variant="KERNEL_LDS", j_split=4)])


@pytest.mark.parametrize("precision", [32, 64])
def test_the_bits_do_not_depend_on_the_contexts_options_and_a_sliced_context_is_refused(nbx, precision):
    n = 2049
    c = R.case(precision, n, "stripes")
    want = context_values(nbx, precision, n, "stripes")
    made = []
    for o in CONTEXT_OPTIONS:
        opts = {k: getattr(nbx, v) if isinstance(v, str) else v for k, v in o.items()}
        try:
            ctx = nbx.Context(n, precision, **opts)
        except nbx.NbxError as e:
            assert e.code == nbx.NBX_ERR_ARG, (o, str(e))  # not a shape this precision has
            continue
        with ctx:
            ctx.upload(c["state"])
            st = ctx.stats()
            assert same(ctx.clumps(c["label"]), want), (o, st)
            made.append((st["kernel_variant"], st["summation_order"], st["bodies_per_lane"], st["j_split"]))
    assert {m[0] for m in made} >= {nbx.KERNEL_LDS, nbx.KERNEL_SGPR} and len(set(made)) >= 6
    for i_begin, i_count in ((0, 512), (512, 1537), (1024, 300)):  # the velocities of the others are not resident in a slice
        with nbx.Context(n, precision, i_begin=i_begin, i_count=i_count, n_alloc=2304) as ctx:
            ctx.upload(c["state"])
            with pytest.raises(nbx.NbxError) as err:
                ctx.clumps(c["label"])
            assert err.value.code == nbx.NBX_ERR_STATE and "nbx_clumps: the context owns a slice of the bodies" in str(err.value)


def _crc(arrays):
    return ["%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes()) for a in arrays]


@pytest.mark.parametrize("precision", [32, 64])
def test_the_call_leaves_the_trajectory_and_the_counters_alone(nbx, precision):
    n, dt = 2049, 1.0 / 4096
    c = R.case(precision, n, "stripes")
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        ctx.step(3, dt)
        before, down = ctx.stats(), ctx.download()
        got = ctx.clumps(c["label"])
        after, again = ctx.stats(), ctx.download()
        assert before["steps_done"] == after["steps_done"] == 3 and _crc(down.values()) == _crc(again.values())
        assert not same(got, context_values(nbx, precision, n, "stripes"), ("phi",))  # the state after the steps
        ke_a = ctx.step(3, dt)
        a = ctx.download()
    with nbx.Context(n, precision) as ctx:
        ctx.upload(c["state"])
        ctx.step(3, dt)
        ke_b = ctx.step(3, dt)
        b = ctx.download()
    assert _crc(a.values()) == _crc(b.values()) and np.array_equal(ke_a, ke_b)  # a following step is as without the call


def test_state_and_argument_errors(nbx):
    lab = np.zeros(300, dtype=np.int32)
    with nbx.Context(300, 32) as c:
        with pytest.raises(nbx.NbxError) as err:
            c.clumps(lab)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_clumps: nbx_upload has not been called" in str(err.value)
        c.upload(R.cloud(300, 32))
        assert c.clumps(lab)["members"].tolist() == [300] * 300
        out = nbx.ClumpsOut()
        assert nbx.load().nbx_clumps(c._h, None, ctypes.byref(out)) == nbx.NBX_ERR_ARG
        assert nbx.load().nbx_clumps(c._h, lab.ctypes.data_as(ctypes.c_void_p), None) == nbx.NBX_ERR_ARG
        with pytest.raises(nbx.NbxError):
            c.clumps(lab[:299])
        c.step_local(1.0 / 256)
        with pytest.raises(nbx.NbxError) as err:
            c.clumps(lab)
        assert err.value.code == nbx.NBX_ERR_STATE and "nbx_clumps: a local step awaits nbx_commit" in str(err.value)
    with nbx.Ensemble(300, 4, 32) as e:
        with pytest.raises(nbx.NbxError) as err:
            e.clumps(np.zeros((4, 300), dtype=np.int32))
        assert err.value.code == nbx.NBX_ERR_STATE and "member 0 has not been uploaded" in str(err.value)
        for first, count in ((-1, 1), (0, 5), (4, 1)):
            with pytest.raises(nbx.NbxError) as err:
                e.clumps(np.zeros((max(count, 0), 300), dtype=np.int32), first=first, count=count)
            assert err.value.code == nbx.NBX_ERR_ARG and "outside [0, members)" in str(err.value)


@pytest.mark.parametrize("kind", ["context", "ensemble"])
@pytest.mark.parametrize("precision", [32, 64])
def test_unbind_removes_the_interloper_then_its_companion_as_the_reference_predicts(nbx, precision, kind):
    st = R.unbind_state(precision)
    n = R.UNBIND_N
    start = np.zeros(n, dtype=np.int32)
    want, iterations, margin = R.unbind(st, start, precision)
    assert iterations >= 3 and want[n - 2] == want[n - 1] == -1 and (want[:64] == 0).sum() >= 32
    if kind == "context":
        with nbx.Context(n, precision) as c:
            c.upload(st)
            label, result, its = nbx.unbind(c, start)
            first = c.clumps(start)
    else:
        with nbx.Ensemble(n, 2, precision) as e:
            e.upload([st, st])
            label, result, its = nbx.unbind(e, np.zeros((2, n), dtype=np.int32))
            first = {k: v[0] for k, v in e.clumps(np.zeros((2, n), dtype=np.int32)).items()}
            assert np.array_equal(label[0], label[1])
            label, result = label[1], {k: v[1] for k, v in result.items()}
    assert its == iterations and np.array_equal(label, want)
    assert first["energy"][n - 2] > 0 and first["energy"][n - 1] < 0  # the companion is bound while the interloper counts
    assert (result["energy"][label >= 0] < 0).all() and np.array_equal(result["members"] > 0, label >= 0)
    cat = nbx.clump_catalogue(label, result, st["mass"])
    assert cat["label"].tolist() == [0] and cat["members"][0] == cat["bound"][0] == (want >= 0).sum() and cat["virial"][0] < 2.0


def test_one_call_costs_no_more_than_one_call_per_context(nbx):
    """16 x 2048 as an ensemble and 16 sizes spread over 512 ... 4096 as a ragged ensemble, fp32: one batch call against 16
    nbx_clumps calls on contexts created and uploaded beforehand, in this process, rounds alternated (tools/clumps_cost.py).
    ratio <= 1.0, the condition every batch call carries."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import clumps_cost
    cells = {}
    for kind in ("ensemble", "ragged"):
        r = clumps_cost.measure(nbx, kind)
        print("%s fp32: batch %.1f us, 16 contexts %.1f us, ratio %.3f" % (kind, r["batch_us"], r["contexts_us"], r["ratio"]))
        cells[kind] = r
    clumps_cost.write(clumps_cost.OUT, cells)
    for kind, r in cells.items():
        assert r["members"] == 16 and r["same_values_from_both_arms"], kind
        assert (r["n_min"], r["n_max"]) == ((2048, 2048) if kind == "ensemble" else (512, 4096))
        assert r["ratio"] <= 1.0, r
