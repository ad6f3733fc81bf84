"""What tests/test_poison_gpu.py relies on, and that its comparisons bind (tests/poison_ref.py); no GPU.

The catalogue's bit patterns; the seeds of the new sizes; on the project's own references, for every state Tier B poisons, that
body b of the FAR control is nobody's nearest neighbour, in nobody's k = 8 row, in no list, within none of the finite radii of
anybody, nobody's friend, nobody's most bound partner and in nobody's bound count -- so that a kept row under the poison has the
far control's bits to equal -- and that the freed rows are at most 5 % of a case's.

The host model (poison_ref.Model) of a member-major pair call with each planted fault, under the comparisons of both tiers at the
module's shapes and poisons.  The case that catches each:

  (a) the velocity j loop reads 8 records past n_alloc, weight 0       Tier A, 3 x 256, vel_y in body 0 of member 1: member 0's sum
  (b) the finish merges the rows of the range's largest member         Tier A, 3 x n, the FIRST member poisoned (ONCE): members 1, 2;
                                                                       the ragged ensemble, member 3 (2049 bodies, the largest)
  (c) the nearest-neighbour merge compares r2 as a signed integer      Tier B, pos_x = the sign-bit NaN: the smallest integer wins
                                                                       every kept row; the quiet NaN, a large positive one, does not
  (d) within is computed as not (r2 > h2)                              Tier B, pos_x = NaN: within of every kept row is one more
  (e) the scalar reduce takes its minimum across the range's members   Tier A, vel_y = +inf: the poisoned member's 0 is everyone's

The cases of tests/test_jerk_gpu.py's velocity-poison test -- two members of 257 bodies, the second one's body 0, member 0's
velocity-reading sums -- catch (a), which reads member 1's first records there too, and none of (b) to (e).  The model without a
fault passes every case.
"""
import os
import re

import numpy as np
import pytest

import binaries_ref as B
import call_order_ref as R
import fof_ref as FOF
import knn_ref as KN
import neighbours_ref as NB
import nlist_ref as NL
import paircount_ref as PC
import poison_ref as P
from conftest import PKG

TARGET_KEYS = ((257, 0), (257, 1), (2049, 0), (2049, 1))  # the states Tier B poisons: TARGETS_B of tests/test_poison_gpu.py
TARGET_SIZES = {(257, 0): (257,), (257, 1): (257,) * 3, (2049, 0): (2049,), (2049, 1): (2049,) * 3}


def test_the_catalogue_is_what_it_says():
    assert len(P.POISONS) == 12 and len(P.POSITION_POISONS) == 5
    for precision, bits, nan_bits in ((32, 0xffc00001, 0x7fc00000), (64, 0xfff8000000000001, 0x7ff8000000000000)):
        T, U = B.DTYPE[precision], P.SIGNED_NAN_BITS[precision][0]
        v = {name: np.array([P.value(name, precision)], dtype=T) for name in P.VALUES}
        assert all(a.dtype == T for a in v.values())
        assert int(v["-nan"].view(U)[0]) == bits and int(v["nan"].view(U)[0]) == nan_bits and np.isnan(v["-nan"][0])
        assert v["-nan"].view({32: np.int32, 64: np.int64}[precision])[0] < 0 < v["nan"].view({32: np.int32, 64: np.int64}[precision])[0]
        assert v["+inf"][0] == np.inf and v["-inf"][0] == -np.inf
        with np.errstate(over="ignore"):
            assert np.isfinite(v["big"][0]) and np.isinf(v["big"][0] * v["big"][0])
        far = T(P.FAR)
        assert np.isfinite(far ** 4) and far == P.FAR
        st = R.clean_state((5, 0), precision)
        s = P.poisoned(st, "pos_x", "-nan", 4, precision)  # the payload survives the copy and the stacking an upload does
        stacked = np.ascontiguousarray(np.stack([np.asarray(s["pos_x"]), st["pos_x"]]), dtype=T)
        assert int(stacked.view(U)[0, 4]) == bits and np.array_equal(stacked[1], st["pos_x"]) and not np.isnan(st["pos_x"]).any()
    text = open(os.path.join(PKG, "csrc", "nbx_plan.hpp")).read()
    a, b, c = (int(g) for g in re.search(r"constexpr int kSgprOverread = (\d+) \+ (\d+) \* (\d+);", text).groups())
    assert a + b * c == P.OVERREAD


def test_the_placements_give_every_clean_member_a_poisoned_neighbour_before_it_and_behind_it():
    for members in (3, 5):
        pl = P.placements(members)
        assert {m for m, *_ in pl} == set(range(members))
        assert sum(1 for m, *_ in pl if m in (0, members - 1)) == 2 and len(pl) == (members - 2) * 24 + 2
        for m in range(members):
            for q in (m - 1, m + 1):
                if 0 <= q < members:
                    assert (q, "pos_x", "nan", "first" if q > m else "last") in pl
    assert P.ranges_a(3, 1) == [(0, 3), (0, 1), (2, 1)]
    assert P.ranges_a(5, 2) == [(0, 5), (0, 1), (1, 1), (3, 1), (4, 1), (0, 2), (3, 2)]
    assert P.ranges_a(5, 0) == [(0, 5), (1, 1), (2, 1), (3, 1), (4, 1), (1, 4)] and P.ranges_a(3, 2) == [(0, 3), (0, 1), (1, 1), (0, 2)]


@pytest.mark.parametrize("precision", [32, 64])
def test_the_new_seeds_are_unambiguous(precision):
    for key in P.SEEDS:
        assert B.ambiguity(R.clean_state(key, precision), precision) == 0, key
    assert len({tuple(R.clean_state(k, precision)["pos_x"][:4]) for k in ((256, 0), (256, 1), (256, 2))}) == 3


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("which", P.BODIES)
@pytest.mark.parametrize("key", TARGET_KEYS, ids=lambda k: "%dv%d" % k)
def test_in_the_far_control_body_b_is_nobodys_neighbour_friend_or_partner(key, which, precision):
    n = key[0]
    sizes = TARGET_SIZES[key]
    b = P.body_of(which, n)
    st = P.far(R.clean_state(key, precision), b)
    others = np.arange(n) != b
    radii = {f: R.FAMILIES[f].args(sizes, precision)["large"] for f in ("neighbours", "nlist", "fof")}
    finite = max(list(radii.values()) + list(PC.RADII))
    x = [np.asarray(st[k], dtype=np.float64) for k in B.POS]
    r2 = sum((c - c[b]) ** 2 for c in x)
    assert r2[others].min() > 4.0 * NB.h2_of(finite, precision)          # within none of the finite radii of anybody
    nb = NB.neighbours(st, radii["neighbours"], precision)
    assert (nb["index"][others] != b).all() and nb["within"][b] == 0      # nobody's nearest neighbour
    assert (KN.knn(st, 8, precision)["index"][others] != b).all()         # in nobody's k = 8 row
    nl = NL.nlist(st, radii["nlist"], precision)
    assert (nl["index"] != b).all() and nl["offsets"][b + 1] == nl["offsets"][b]  # in no list, and its own is empty
    assert FOF.fof(st, radii["fof"], precision)["size"][b] == 1           # nobody's friend
    bn = B.binaries(st, precision)
    assert (bn["partner"][others] != b).all()                             # nobody's most bound partner
    i = np.arange(n)[others]
    e, mag = B.pair_energy(st, i, np.full(len(i), b))
    assert (e - B.GATE[precision] * B.U[precision] * mag > 0).all()       # in nobody's bound count, whatever the rounding
    # the rows a case frees, counted on the references: body b's own, the lists that hold b, the bodies b is the partner of
    lists = P.nlist_lists(nl, n)
    freed = {"neighbours": 1, "knn": 1, "fof": 1, "nlist": 1 + sum(1 for i in range(n) if i != b and (lists[i][0] == b).any()),
             "binaries": 1 + int((bn["partner"][others] == b).sum())}
    assert n >= 257 and max(freed.values()) == 1 and max(freed.values()) <= P.FREED_CAP * n, freed


def test_tier_b_keeps_and_frees_the_right_rows():
    n, b = 8, 3
    idx = np.array([1, 0, 1, 2, 5, 4, 7, 6], dtype=np.int32)
    want = {"index": idx, "r2": np.linspace(1, 2, n).astype(np.float32), "within": np.ones(n, dtype=np.int32)}
    got = {k: v.copy() for k, v in want.items()}
    got["index"][b], got["r2"][b], got["within"][b] = -1, np.inf, 0
    assert P.tier_b("neighbours", got, want, b, n) == ([], 1, {})
    got["r2"][5] = np.nextafter(got["r2"][5], np.float32(9))
    assert P.tier_b("neighbours", got, want, b, n)[0] == ["r2 of a kept row"]
    got["r2"][5], got["index"][b] = want["r2"][5], n
    assert P.tier_b("neighbours", got, want, b, n)[0] == ["index outside [-1, n)"]
    pw = {"partner": idx, "energy": want["r2"], "bound": want["within"]}
    pg = {k: v.copy() for k, v in pw.items()}
    pg["partner"][6], pg["energy"][6] = b, 9.0  # a body body b is the partner of: freed
    assert P.tier_b("binaries", pg, pw, b, n)[:2] == ([], 2)
    lw = {"offsets": np.array([0, 1, 2, 2, 2], dtype=np.int64), "index": np.array([1, 0], dtype=np.int32), "r2": np.ones(2, dtype=np.float32)}
    lg = {"offsets": np.array([0, 2, 3, 4, 4], dtype=np.int64), "index": np.array([1, 2, 0, 0], dtype=np.int32), "r2": np.ones(4, dtype=np.float32)}
    assert P.tier_b("nlist", lg, lw, 2, 4)[0] == [] and P.tier_b("nlist", lg, lw, 2, 4)[1] == 2  # bodies 0 (lists b) and 2 freed; 1 and 3 kept
    lg["r2"][2] = 2.0
    assert P.tier_b("nlist", lg, lw, 2, 4)[0] == ["the list of kept body 1"]
    lg["offsets"][4] = 5
    assert P.tier_b("nlist", lg, lw, 2, 4)[0] == ["offsets not ascending within the capacity"]
    c = {"counts": np.array([3, 10], dtype=np.uint64)}
    assert P.tier_b("paircount", {"counts": np.array([3, 13], dtype=np.uint64)}, c, 0, 4)[0] == []
    assert P.tier_b("paircount", {"counts": np.array([2, 10], dtype=np.uint64)}, c, 0, 4)[0] and P.tier_b("paircount", {"counts": np.array([3, 14], dtype=np.uint64)}, c, 0, 4)[0]
    f = lambda lab: {"label": np.array(lab, dtype=np.int32), "groups": 1, "largest": 1, "passes": 1}
    assert P.tier_b("fof", f([0, 0, 2, 3, 3]), f([0, 0, 0, 3, 3]), 2, 5)[0] == []   # body 2 joined a group or left it: the others' partition stands
    assert P.tier_b("fof", f([0, 1, 2, 3, 3]), f([0, 0, 2, 3, 3]), 2, 5)[0] == ["the partition of the other bodies"]
    assert P.tier_b("fof", f([0, 0, 2, 3, 5]), f([0, 0, 2, 3, 3]), 2, 5)[0] == ["label outside [0, n)", "the partition of the other bodies"]
    assert P.others_differ({"a": np.array([9.0, 1.0, 9.0])}, {"a": np.array([0.0, 1.0, 2.0])}, (0, 2), ["a"]) == []
    assert P.others_differ({"a": np.array([0.0, 1.5, 2.0])}, {"a": np.array([0.0, 1.0, 2.0])}, (0, 2), ["a"]) == ["a"]


MODEL_TARGETS = [((257,) * 3, 1), ((2049,) * 3, 1), (P.RAGGED_SIZES, 1), (P.RAGGED_SIZES, 3)]


def test_the_model_without_a_fault_passes_every_case():
    for kind, sizes in P.shapes():
        for p, field, name, which in P.placements(len(sizes)):
            assert P.model_tier_a(sizes, 32, None, p, field, name, which) == [], (sizes, p, field, name, which)
    for sizes, p in MODEL_TARGETS:
        for name in P.VALUES:
            for which in P.BODIES:
                assert P.model_tier_b(sizes, 32, None, p, name, which) == [], (sizes, p, name, which)
    for precision in (32, 64):
        assert P.model_jerk_cases(precision, None) == []
        assert P.model_tier_a((256,) * 3, precision, None, 1, "vel_y", "big", "first") == []


@pytest.mark.parametrize("precision", [32, 64])
def test_fault_a_is_caught_at_256_bodies_by_the_velocity_poison_in_body_0_of_the_next_member(precision):
    for name in ("nan", "-nan", "+inf", "-inf"):
        bad = P.model_tier_a((256,) * 3, precision, "a", 1, "vel_y", name, "first")
        assert bad and all("clean member 0: sum" in t for t in bad), (name, bad)
    assert P.model_tier_a((256,) * 3, precision, "a", 1, "vel_y", "big", "first") == []  # 0 times a finite value is 0
    assert P.model_tier_a((256,) * 3, precision, "a", 1, "vel_y", "nan", "last") == []  # 255 records further on: not reached
    assert P.model_tier_a((256,) * 3, precision, "a", 1, "pos_x", "nan", "first") == []  # the spare position records are there
    assert P.model_jerk_cases(precision, "a")  # the old test's 257 bodies: n_alloc + 8 is the next member's there too


@pytest.mark.parametrize("precision", [32, 64])
def test_fault_b_is_caught_where_the_first_or_the_largest_member_is_poisoned(precision):
    for n in (256, 257, 2049):
        bad = P.model_tier_a((n,) * 3, precision, "b", 0, *P.ONCE, "last")
        assert any("clean member 1: r2" in t for t in bad) and any("clean member 2: r2" in t for t in bad), (n, bad)
        assert P.model_tier_a((n,) * 3, precision, "b", 1, *P.ONCE, "last", ranges=[(0, 3)]) == []  # an interior member: nobody reads its rows
    bad = P.model_tier_a(P.RAGGED_SIZES, precision, "b", 3, "pos_x", "nan", "first")
    assert any("range (0, 5): clean member 0" in t for t in bad), bad
    assert P.model_jerk_cases(precision, "b") == []


@pytest.mark.parametrize("precision", [32, 64])
def test_fault_c_is_caught_by_the_nan_with_the_sign_bit_alone(precision):
    for sizes, p in MODEL_TARGETS[:1] + MODEL_TARGETS[2:3]:
        for which in P.BODIES:
            assert P.model_tier_b(sizes, precision, "c", p, "-nan", which) == ["index of a kept row", "r2 of a kept row"]
            for name in ("nan", "+inf", "-inf", "big"):
                assert P.model_tier_b(sizes, precision, "c", p, name, which) == [], name
    assert P.model_jerk_cases(precision, "c") == []


@pytest.mark.parametrize("precision", [32, 64])
def test_fault_d_is_caught_by_a_nan_position(precision):
    for sizes, p in MODEL_TARGETS[:1] + MODEL_TARGETS[2:3]:
        for name in ("nan", "-nan"):
            assert P.model_tier_b(sizes, precision, "d", p, name, "first") == ["within of a kept row"]
        for name in ("+inf", "-inf", "big"):
            assert P.model_tier_b(sizes, precision, "d", p, name, "first") == []
    assert P.model_jerk_cases(precision, "d") == []


@pytest.mark.parametrize("precision", [32, 64])
def test_fault_e_is_caught_by_a_velocity_whose_square_is_infinite(precision):
    for name in ("+inf", "-inf", "big"):
        bad = P.model_tier_a((257,) * 3, precision, "e", 1, "vel_y", name, "last")
        assert bad == ["range (0, 3): clean member 0: scalar", "range (0, 3): clean member 2: scalar"], (name, bad)
    assert P.model_tier_a((257,) * 3, precision, "e", 1, "vel_y", "+inf", "last", ranges=[(0, 1), (2, 1)]) == []  # a member alone has nobody to mix with
    assert P.model_jerk_cases(precision, "e") == []
