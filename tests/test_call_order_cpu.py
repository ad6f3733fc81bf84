"""What tests/test_call_order_gpu.py relies on, and why it sees what the module tests cannot (tests/call_order_ref.py); no GPU.

Layout facts, from the shape functions and, for field_shape, from the header itself through tests/field_shape_driver.cpp: the
split and column counts of the five ragged sizes, the strides of the ranges asked, the passes of the paircount arguments, the
totals of the nlist radii, and that no clean state is ambiguous for the comparisons truth_check() borrows.

The host model (call_order_ref.Model) with each planted fault, driven by OLD_ORDER -- a fresh object whose allocation reads as
zeros, the full range first, the same call again, then sub-ranges that start at member 0: the part of the module tests' order the
blind spot rests on -- and by the sequence of the GPU module.  Which numbered comparison first catches which fault, on the
ragged shape (1, 4, 1, 2, 1) / on the ensemble of 3 x 2 splits / on a context of 4 splits:

  (a) the finish walks the range's row_splits, not the member's own        passes OLD_ORDER; 3.3 range (0, 2) / never / never
  (b) the finish strides by the member's own splits                         fails OLD_ORDER at its first call; 2 / never / never
  (c) the member table is built from the first call's `first`               passes OLD_ORDER; 2 (clean: 3.1) / no table / no table
  (d) the finish uses the layout (k, passes, m) of the previous call        passes OLD_ORDER; 2 (clean: 3.4 small) on every kind
  (e) a grown buffer keeps its old capacity figure                          passes OLD_ORDER; 2 (clean: 3.1) on every kind

(a) needs a row that another call left nonzero: member 0's unowned rows after member 1 was asked alone (3.2).  (b) is the one
fault of the five that is no blind spot: where the members' split counts differ, a ragged ensemble's first full-range call has it
already -- the module tests meet it -- and where they are equal, own and range's strides are one number and it is no fault.  On an
ensemble and a context (a) and (b) cannot arise and (c) has no table to build.  The model keeps every fault that the old order
passes and the new sequence catches on at least one kind of object; that is asserted below, fault by fault.
"""
import os
import subprocess

import numpy as np
import pytest

import binaries_ref as B
import call_order_ref as R
import field_ref as FR
import fof_ref as FOF
import neighbours_ref as NB
import nlist_ref as NL
import paircount_ref as PC
from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")
MODEL_SPLITS = {"ragged": R.RAGGED_SPLITS, "ensemble": (2, 2, 2), "context": (4,)}
NAMES = ("small", "large", "middle")
FIRST_CATCH = {  # fault -> kind -> the first label of the sequence whose result is wrong (None: never)
    "a": {"ragged": "3.3 range (0, 2)", "ensemble": None, "context": None},
    "b": {"ragged": "2", "ensemble": None, "context": None},
    "c": {"ragged": "2", "ensemble": None, "context": None},
    "d": {"ragged": "2", "ensemble": "2", "context": "2"},
    "e": {"ragged": "2", "ensemble": "2", "context": "2"},
}
FIRST_CLEAN_CATCH = {"a": "3.3 range (0, 2)", "b": "3.1", "c": "3.1", "d": "3.4 small", "e": "3.1"}  # on the ragged shape, steps 3.x and 4 alone


def test_the_split_and_column_counts_of_the_ragged_sizes_and_the_strides_of_the_ranges(tmp_path):
    shapes = R.ragged_shapes()
    assert tuple(s for _, s in shapes) == R.RAGGED_SPLITS == (1, 4, 1, 2, 1)
    assert len({c for c, _ in shapes}) > 1 and [c for c, _ in shapes] == [1, 9, 1, 5, 2]
    strides = [R.range_stride(*r) for r in ((0, 5), (2, 1), (3, 2), (0, 1))]
    assert strides == [4, 1, 2, 1]
    # (2, 1) and (0, 1) have one split each but members of other sizes: the strides IN RECORDS -- splits x bodies -- all differ
    records = [R.range_stride(f, c) * max(R.RAGGED_SIZES[f:f + c]) for f, c in ((0, 5), (2, 1), (3, 2), (0, 1))]
    assert len(set(records)) == 4
    assert all(R.range_stride(*r) in (1, 2, 4) for r in R.RANGES["ragged"]) and {R.range_stride(*r) for r in R.RANGES["ragged"]} == {2, 4}
    # an ensemble of 3 x 2049 and the contexts: more than one split, the last one short
    assert FR.field_shape(2049, 2049) == (5, 9, 2, 5) and FR.field_shape(4097, 4097) == (9, 17, 4, 5)
    for m in R.POINTS.values():  # the points' shapes: other columns, the bodies' splits
        assert [FR.field_shape(m, n)[2] for n in R.RAGGED_SIZES] == [1, 4, 1, 2, 1]
    assert [FR.field_shape(m, 2049)[0] for m in (3, 1500, 513)] == [1, 3, 2]
    pairs = sorted({(n, n) for n in R.RAGGED_SIZES} | {(m, n) for m in R.POINTS.values() for n in R.RAGGED_SIZES})
    exe = str(tmp_path / "field_shape_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "field_shape_driver.cpp"), "-o", exe])
    lines = subprocess.run([exe] + [str(v) for mn in pairs for v in mn], capture_output=True, text=True, check=True).stdout.splitlines()
    assert [tuple(int(v) for v in line.split()) for line in lines[:-1]] == [(m, n) + FR.field_shape(m, n) for m, n in pairs]


def test_the_arguments_change_the_layout():
    assert [len(PC.pass_slots(len(r))) for r in (R.PAIRCOUNT_RADII[k] for k in NAMES)] == [1, 2, 1]
    assert PC.pass_slots(20) == [(0, 16, 16), (16, 4, 4)] and PC.pass_slots(3) == [(0, 3, 4)] and PC.pass_slots(1) == [(0, 1, 4)]
    assert R.FAMILIES["knn"].args((5,), 32) == {"small": 1, "large": 16}
    for fam in R.FAMILIES.values():
        assert fam.names()[-1 if len(fam.names()) < 3 else 1] == "large" and set(fam.dirt) <= set(fam.keys)
    assert [f for f, fam in R.FAMILIES.items() if not fam.takes_argument] == ["diagnostics", "timescale", "accel", "tidal_bodies", "jerk"]
    # the sequence: the narrowest call first, the widest second, and every comparison of the module docstring
    labels = [s[0] for s in R.sequence("ragged", NAMES)]
    assert labels[:3] == ["1", "2", "3.1"] and labels[-3:] == ["3.5", "3.6", "4"] and "3.4 middle" in labels and len(labels) == 16
    assert R.sequence("ragged", NAMES)[0][2:] == ("small", 2, 1) and R.sequence("context", ("large",))[0][2:] == ("large", 0, None)
    assert [s[0] for s in R.sequence("context", ("small", "large"))] == ["1", "2", "3.1", "3.4 small", "3.5", "3.6", "4"]


@pytest.mark.parametrize("precision", [32, 64])
def test_the_clean_states_are_unambiguous_and_the_nlist_totals_are_8_times_apart(precision):
    for key in R.CLEAN_SEEDS:
        st = R.clean_state(key, precision)
        assert B.ambiguity(st, precision) == 0, key  # binaries_ref.compare holds the partner on every body
        dirty = R.dirty_state(key, precision)
        assert all(np.array_equal(dirty[f], st[f]) is False for f in B.POS + ("mass",)) and all((dirty[f] != 0).any() for f in B.VEL)
    for kind in R.KINDS:
        sizes = R.sizes_of(kind)
        clean = R.states(sizes, precision)[0]
        radii = R.FAMILIES["neighbours"].args(sizes, precision)
        assert radii["small"] != radii["large"]
        for st in clean:
            for r in radii.values():
                assert NB.ambiguity(st, r, precision) == (0, 0) and not FOF.ambiguous(st, r, precision)
        radii = R.FAMILIES["nlist"].args(sizes, precision)
        totals = {k: sum(NL.nlist(st, r, precision)["total"] for st in clean) for k, r in radii.items()}
        assert all(not NL.ambiguous(st, r, precision) for st in clean for r in radii.values())
        assert totals["small"] > 0 and totals["large"] >= 8 * totals["small"], (kind, totals)


def test_the_model_without_a_fault_passes_every_order():
    for kind, splits in MODEL_SPLITS.items():
        assert R.Model(splits).run(R.sequence(kind, NAMES), R.MODEL_ITEMS) == []
        assert R.Model(splits).run(R.OLD_ORDER, R.MODEL_ITEMS) == []


@pytest.mark.parametrize("fault", list(R.FAULTS))
def test_a_planted_fault_slips_past_the_old_order_and_is_caught_by_the_sequence(fault):
    old = {kind: R.Model(splits, fault).run(R.OLD_ORDER, R.MODEL_ITEMS) for kind, splits in MODEL_SPLITS.items()}
    new = {kind: R.Model(splits, fault).run(R.sequence(kind, NAMES), R.MODEL_ITEMS) for kind, splits in MODEL_SPLITS.items()}
    print(fault, R.FAULTS[fault], "\n old:", old, "\n new:", new)
    if fault == "b":  # no blind spot: see the module docstring
        assert old["ragged"][0] == "full" and old["ensemble"] == old["context"] == []
    else:
        assert old == {"ragged": [], "ensemble": [], "context": []}
    assert {kind: (bad[0] if bad else None) for kind, bad in new.items()} == FIRST_CATCH[fault]
    assert new["ragged"], "a fault the sequence does not catch: extend the sequence"
    clean_steps = [label for label in new["ragged"] if label[0] in "34"]  # a comparison with the fresh expectation
    assert clean_steps and clean_steps[0] == FIRST_CLEAN_CATCH[fault]


def test_differences_sees_one_bit_a_sign_of_zero_a_dtype_and_a_missing_array():
    fam = R.FAMILIES["neighbours"]
    a = [{"index": np.arange(4, dtype=np.int32), "r2": np.array([0.0, 1.0, 2.0, np.nan], dtype=np.float32), "within": None}]
    same = [{k: (None if v is None else v.copy()) for k, v in a[0].items()}]
    assert R.differences(fam, a, same) == [] and R.clean_keys(fam, a, same) == list(fam.dirt)
    for key, value in (("r2", np.array([-0.0, 1.0, 2.0, np.nan], dtype=np.float32)), ("r2", a[0]["r2"].astype(np.float64)),
                       ("r2", np.nextafter(a[0]["r2"], np.float32(9))), ("index", np.array([0, 1, 2, 4], dtype=np.int32)),
                       ("within", np.zeros(4, dtype=np.int32))):
        assert R.differences(fam, a, [dict(same[0], **{key: value})]) == ["member 0: " + key]
    assert R.differences(fam, a, same + same) == ["1 members against 2"]
    fof = R.FAMILIES["fof"]
    g = [{"label": np.zeros(3, np.int32), "size": np.full(3, 3, np.int32), "groups": np.asarray(1), "largest": np.asarray(3), "passes": np.asarray(2)}]
    w = [dict(g[0], passes=np.asarray(3))]
    assert R.differences(fof, g, w) == ["member 0: passes"] and R.differences(fof, g, w, full_range=False) == []
    assert R.differences(fof, w, g, full_range=False) == ["member 0: passes = 3 outside [1, 2]"]


def test_truth_check_passes_the_references_own_results_and_rejects_a_planted_error():
    """One member of 257 bodies, fp32: results made on the host by the modules' references pass; one wrong entry does not."""
    import jerk_ref as J
    import knn_ref as KN
    sizes, precision = (257,), 32
    st = R.states(sizes, precision)[0][0]
    knn = KN.knn(st, 16, precision)
    made = {"knn": {"index": knn["index"], "r2": knn["r2"].astype(np.float32)},
            "paircount": {"counts": PC.counts(st, PC.RADII, precision)},
            "jerk": J.restate(st, precision)}
    for family, res in made.items():
        assert R.truth_check(family, "context", precision, [res], sizes=sizes) == [], family
    wrong = {k: v.copy() for k, v in made["knn"].items()}
    wrong["index"][100, 3] = wrong["index"][100, 4]
    assert R.truth_check("knn", "context", precision, [wrong], sizes=sizes)
    wrong = {"counts": made["paircount"]["counts"].copy()}
    wrong["counts"][17] += np.uint64(40)
    assert R.truth_check("paircount", "context", precision, [wrong], sizes=sizes)
    wrong = {k: v.copy() for k, v in made["jerk"].items()}
    wrong["jerk_y"][256] *= np.float32(1.001)
    assert R.truth_check("jerk", "context", precision, [wrong], sizes=sizes)
