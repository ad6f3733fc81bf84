"""Poison probes: what a body that is not finite, or whose square overflows T, may touch (the "Unspecified results" sentences of the
public headers).  The catalogue, the shapes, the two controls, the comparisons of both tiers and a host model of a member-major
pair call.  Used by tests/test_poison_cpu.py and tests/test_poison_gpu.py; numpy only, no device.

POISONS: the values -- "nan" the default quiet NaN, "-nan" a NaN with the sign bit and a payload bit set (fp32 0xffc00001, fp64
0xfff8000000000001: the smallest signed integers but a few, as bit patterns), "+inf", "-inf" and "big", finite while its square
overflows T (2^100 in fp32, 2^600 in fp64) -- and the fields: pos_x and vel_y take every value, mass the quiet NaN and +inf.  The
poison goes into ONE body b of ONE system, b the first body or the last one.

Tier A, "another system is never touched": a batch object holds the clean states of call_order_ref.clean_state with one member
poisoned; a CLEAN CONTROL of the same kind, sizes and precision holds the same states with that member clean.  Every clean
member's result of every call must be the clean control's, bit for bit, over the ranges of ranges_a().
Tier B, "another body of the same system": the position poison against a FAR CONTROL, the same state with body b at pos_x = FAR,
a finite place where nothing overflows and where it is nobody's neighbour, friend or partner (held on the references in the CPU
test): every row the header's sentence does not free must be the far control's, bit for bit (tier_b()).

Shapes: ensembles of three members of 256 (no padding record: the next member's velocities follow at once), 257 (255 padding
records) and 2049 bodies (two splits: every finish merges rows); the ragged ensemble (256, 257, 5, 2049, 513); contexts of 257
and 2049.  Every interior member is poisoned in turn with the whole catalogue, the first and the last member once each (ONCE),
so that every clean member has a poisoned neighbour before it and behind it.
"""
import numpy as np

import binaries_ref as B
import call_order_ref as R
import field_ref as FR
from energy_ref import EPS2
import neighbours_ref as NB

# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
VALUES = ("nan", "-nan", "+inf", "-inf", "big")
SIGNED_NAN_BITS = {32: (np.uint32, 0xffc00001), 64: (np.uint64, 0xfff8000000000001)}
BIG_EXPONENT = {32: 100, 64: 600}


def value(name, precision):
    T = B.DTYPE[precision]
    if name == "-nan":
        u, bits = SIGNED_NAN_BITS[precision]
        return np.array([bits], dtype=u).view(T)[0]
    return T({"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "big": 2.0 ** BIG_EXPONENT[precision]}[name])


POISONS = tuple([("pos_x", v) for v in VALUES] + [("vel_y", v) for v in VALUES] + [("mass", "nan"), ("mass", "+inf")])
POSITION_POISONS = tuple(p for p in POISONS if p[0] == "pos_x")
BODIES = ("first", "last")
ONCE = ("pos_x", "nan")  # the poison of the first and of the last member: the body next to the neighbouring member


def body_of(which, n):
    return 0 if which == "first" else n - 1


def poisoned(state, field, name, b, precision):
    s = {k: v.copy() for k, v in state.items()}
    s[field][b] = value(name, precision)
    return s


FAR = 2.0 ** 13  # 2^12 system radii: the clouds fill [-1, 1]^3, inside a radius of 2


def far(state, b):
    """The far control: body b at pos_x = FAR, finite in both precisions with everything squared."""
    s = {k: v.copy() for k, v in state.items()}
    s["pos_x"][b] = s["pos_x"].dtype.type(FAR)
    return s


# ---- shapes and states -------------------------------------------------------------------------------------------------------------
ENSEMBLES = ((3, 256), (3, 257), (3, 2049))
RAGGED_SIZES = (256, 257, 5, 2049, 513)
CONTEXTS = (257, 2049)
# seeds of binaries_ref.cloud for the sizes call_order_ref has none for: the first from 300 + n at which no body's most bound
# partner is ambiguous in either precision (tests/test_poison_cpu.py holds them to it)
SEEDS = {(256, 0): 556, (256, 1): 557, (256, 2): 558, (257, 1): 557, (257, 2): 558}
R.CLEAN_SEEDS.update(SEEDS)
TRACERS = 300
POINTS = ("small", "middle")  # m = 3 and 513 of call_order_ref.POINTS


def shapes():
    """[(kind, sizes)] of the batch objects."""
    return [("ensemble", (n,) * s) for s, n in ENSEMBLES] + [("ragged", RAGGED_SIZES)]


def clean_states(sizes, precision):
    return [R.clean_state(k, precision) for k in R.member_keys(sizes)]


def placements(members):
    """[(poisoned member, field, value, body)]: the catalogue x both bodies in every interior member, ONCE in the first member's
    last body and in the last member's first."""
    out = [(m,) + p + (w,) for m in range(1, members - 1) for p in POISONS for w in BODIES]
    return out + [(0,) + ONCE + ("last",), (members - 1,) + ONCE + ("first",)]


def ranges_a(members, p):
    """[(first, count)] of Tier A: the full range, every clean member alone, the range that ends just before member p and the one
    that starts just behind it."""
    out = [(0, members)] + [(m, 1) for m in range(members) if m != p]
    for r in ((0, p), (p + 1, members - p - 1)):
        if r[1] > 0 and r not in out:
            out.append(r)
    return out


# ---- which family must show which poison ---------------------------------------------------------------------------------------------
# The families that read a field, timescale left out: its three scalars are a minimum and two maxima taken with compares that a
# NaN never passes, so the poisoned body may drop out of them without a trace.  nlist, paircount and fof show a position only
# where body b has a partner within the radius in the clean state (shows()).
READS = {"pos_x": ("diagnostics", "accel", "field", "neighbours", "paircount", "knn", "fof", "binaries", "tidal", "tidal_bodies", "clumps",
                   "nlist", "jerk"),
         "vel_y": ("diagnostics", "binaries", "clumps", "jerk"),
         "mass": ("diagnostics", "accel", "field", "binaries", "tidal", "tidal_bodies", "clumps", "jerk")}
WITHIN_RADIUS = ("nlist", "paircount", "fof")


def has_partner_within(state, b, radius, precision):
    x = [np.asarray(state[k], dtype=np.float64) for k in B.POS]
    r2 = sum((c - c[b]) ** 2 for c in x) + EPS2
    r2[b] = np.inf
    return bool((r2 <= NB.h2_of(radius, precision)).any())


def shows(family, field, state, b, arg, precision):
    """Whether the poisoned member's own result of `family` must differ from the clean control's."""
    if family.name not in READS[field]:
        return False
    if family.name in WITHIN_RADIUS:
        return has_partner_within(state, b, max(arg) if family.name == "paircount" else arg, precision)
    return True


def float_keys(family, result):
    return [k for k in family.keys if result[k] is not None and np.asarray(result[k]).dtype.kind == "f"]


def not_shown(family, got, want):
    """True where the poisoned member's result equals the clean one's in every float key (in every key, for a family without one)."""
    keys = float_keys(family, want) or list(family.keys)
    return all(R._same_value(got[k], want[k]) for k in keys if k not in family.call_wide)


# ---- Tier A ------------------------------------------------------------------------------------------------------------------------
class _Own:
    """A family's keys without the call's own (fof's passes)."""

    def __init__(self, family):
        self.keys, self.call_wide = tuple(k for k in family.keys if k not in family.call_wide), ()


def tier_a(family, got, want, first, count, p):
    """Where the clean members of the range [first, first + count) differ from the clean control's (call_order_ref.differences:
    integers by array_equal, floats as bytes), member numbers the object's.  The call's own keys are compared only where the
    range leaves member p out."""
    inside = first <= p < first + count
    if len(got) != count or len(want) != count:
        return ["%d and %d members against %d" % (len(got), len(want), count)]
    keep = [k for k in range(count) if first + k != p]
    bad = R.differences(_Own(family) if inside else family, [got[k] for k in keep], [want[k] for k in keep])
    out = []
    for t in bad:  # "member k: key", k counted within the clean members of the range
        k, key = t[len("member "):].split(": ", 1)
        out.append("range (%d, %d): clean member %d: %s" % (first, count, first + keep[int(k)], key))
    return out


def records_differ(got, want, p):
    """Lists of one dict of values per member (kinetic energies, clocks, downloads): the clean members' that differ in a bit."""
    return ["member %d: %s" % (m, k) for m, (g, w) in enumerate(zip(got, want)) if m != p for k in w
            if not R._same_value(np.asarray(g[k]), np.asarray(w[k]))] + ([] if len(got) == len(want) else ["members"])


# ---- Tier B ------------------------------------------------------------------------------------------------------------------------
TIER_B = {"neighbours": ("large",), "knn": (1, 8), "nlist": ("large",), "paircount": ("large",), "fof": ("large",), "binaries": (True,)}
FREED_CAP = 0.05  # of the rows of a case, at n >= 257


def nlist_lists(res, n):
    off = np.asarray(res["offsets"]).astype(np.int64)
    return [(res["index"][off[i]:off[i + 1]], res["r2"][off[i]:off[i + 1]]) for i in range(n)]


def first_appearance(label, skip):
    """The labels of every body but `skip`, renamed in the order of first appearance."""
    lab = np.delete(np.asarray(label), skip)
    _, first, inverse = np.unique(lab, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


def tier_b(name, got, want, b, n):
    """(problems, freed rows, record) of one system's result under the position poison in body b against the far control's: the
    rows the header's sentence keeps must be the far control's bit for bit, the freed ones well-formed."""
    bad, record = [], {}
    same = R._same_value
    rows = np.arange(n)
    if name in ("neighbours", "knn", "binaries"):
        first_key = "partner" if name == "binaries" else "index"
        idx = np.asarray(got[first_key])
        freed = rows == b
        if name == "binaries":  # "that body and the bodies it is a partner of"
            freed |= idx == b
        keep = ~freed
        for k, v in got.items():
            if v is not None and not same(np.asarray(v)[keep], np.asarray(want[k])[keep]):
                bad.append("%s of a kept row" % k)
        if not ((idx >= -1) & (idx < n)).all():
            bad.append("%s outside [-1, n)" % first_key)
        for k in ("within", "bound"):
            if got.get(k) is not None and not ((np.asarray(got[k]) >= 0) & (np.asarray(got[k]) <= n)).all():
                bad.append("%s outside [0, n]" % k)
        return bad, int(freed.sum()), record
    if name == "nlist":
        off = np.asarray(got["offsets"]).astype(np.int64)
        if not ((np.diff(off) >= 0).all() and off[0] == 0 and off[-1] <= len(got["index"]) and len(off) == n + 1):
            return ["offsets not ascending within the capacity"], n, record
        if len(got["index"]) and not ((got["index"] >= 0) & (got["index"] < n)).all():
            bad.append("index outside [0, n)")
        g, w = nlist_lists(got, n), nlist_lists(want, n)
        freed = [i for i in range(n) if i == b or (g[i][0] == b).any()]
        bad += ["the list of kept body %d" % i for i in range(n) if i not in freed and not (same(g[i][0], w[i][0]) and same(g[i][1], w[i][1]))][:4]
        return bad, len(freed), record
    if name == "paircount":
        g, w = np.asarray(got["counts"]).astype(np.int64), np.asarray(want["counts"]).astype(np.int64)
        if not ((w <= g) & (g <= w + n - 1)).all():
            bad.append("counts %r outside [far, far + n - 1] of %r" % (g.tolist(), w.tolist()))
        return bad, 0, record
    if name == "fof":
        lab = np.asarray(got["label"])
        if not ((lab >= 0) & (lab < n)).all():
            bad.append("label outside [0, n)")
        if not np.array_equal(first_appearance(lab, b), first_appearance(want["label"], b)):
            bad.append("the partition of the other bodies")
        record = {k: [int(got[k]), int(want[k])] for k in ("groups", "largest", "passes")}
        return bad, 1, record
    raise ValueError(name)


def others_differ(got, want, skip, keys):
    """Per-point or per-tracer arrays: the keys in which an entry other than `skip` differs in a bit."""
    keep = np.ones(np.asarray(want[keys[0]]).shape[-1], dtype=bool)
    keep[list(skip)] = False
    return [k for k in keys if not R._same_value(np.asarray(got[k])[..., keep], np.asarray(want[k])[..., keep])]


# ---- a host model of a member-major pair call --------------------------------------------------------------------------------------
TILE = 256
OVERREAD = 16 + 8 * 64  # kSgprOverread (csrc/nbx_plan.hpp): spare position records behind every member
FAULTS = {"a": "the velocity j loop reads 8 records past n_alloc, with weight 0",
          "b": "the finish merges the rows of the range's largest member for every member",
          "c": "the nearest-neighbour merge compares r2 as a signed integer bit pattern",
          "d": "within is computed as not (r2 > h2)",
          "e": "the scalar reduce takes its minimum across the members of the range"}
MODEL_KEYS = ("sum", "index", "r2", "within", "scalar")
MODEL_H = 0.25


class ModelFamily:
    name, keys, call_wide = "model", MODEL_KEYS, ()


class Model:
    """One batch object's pair call in plain numpy, laid out as the library lays its members out: positions {x, y, z, G m} at a
    stride of n_alloc + OVERREAD records, zero padded (n_alloc the member's n rounded up to the tile); velocities at a stride of
    n_alloc with NOTHING behind them, so that whatever is read past a member's n_alloc is the next member's.  call() gives per
    member of the range
      sum      per body  sum over j of w_j (vy_j - vy_i) / r2(i, j), w = G m: a velocity-reading sum, as the jerk's
      index, r2          the nearest neighbour, `c < best`, the lowest j first
      within   per body  the number of j with r2 <= h2
      scalar   per member  the minimum over the bodies of r2 / (1 + vy^2), `c < q`: a NaN is never selected
    in T throughout.  The pair pass leaves one partial row per split of the member's j range (field_shape(n, n)), member k of
    the range at row k * stride, stride the range's largest split count; the finish merges a member's own rows.  The mask is the
    kernels': j == i and j >= n are dropped.  An operation with a NaN operand gives that NaN, sign and payload kept, as the
    hardware does."""

    def __init__(self, sizes, precision, fault=None):
        assert fault is None or fault in FAULTS
        self.sizes, self.fault, self.T = tuple(sizes), fault, B.DTYPE[precision]
        self.bits = {32: np.int32, 64: np.int64}[precision]
        self.alloc = [-(-n // TILE) * TILE for n in self.sizes]
        self.pos_off = np.concatenate([[0], np.cumsum([a + OVERREAD for a in self.alloc])]).astype(int)
        self.vel_off = np.concatenate([[0], np.cumsum(self.alloc)]).astype(int)
        self.shape = [FR.field_shape(n, n) for n in self.sizes]  # (columns, tiles, splits, tiles per split)

    def upload(self, states, share=None):
        """share: a model of the same sizes, precision and fault whose partial rows serve every member that holds the very same
        state here (the pair pass of a member reads that member alone, but for fault "a")."""
        T = self.T
        self.states, self.share, self._rows = list(states), share, {}
        self.pos = np.zeros((self.pos_off[-1], 4), dtype=T)
        self.vel = np.zeros(self.vel_off[-1] + 8, dtype=T)  # + 8: what fault "a" reads behind the last member is not the model's business
        for m, st in enumerate(states):
            n = self.sizes[m]
            for c, f in enumerate(B.POS):
                self.pos[self.pos_off[m]:self.pos_off[m] + n, c] = st[f]
            self.pos[self.pos_off[m]:self.pos_off[m] + n, 3] = st["mass"]
            self.vel[self.vel_off[m]:self.vel_off[m] + n] = st["vel_y"]
        return self

    def _less(self, c, best):
        if self.fault == "c":
            return np.ascontiguousarray(c).view(self.bits) < np.ascontiguousarray(best).view(self.bits)
        with np.errstate(invalid="ignore"):
            return c < best

    def _merge(self, rows):
        """[(r2, j)] per split, ascending split order, into one: the strict compare keeps the earlier split on ties."""
        r2, j = rows[0][0].copy(), rows[0][1].copy()
        for c, cj in rows[1:]:
            take = self._less(c, r2)
            r2[take], j[take] = c[take], cj[take]
        return r2, j

    def _pair_pass(self, m, h2):
        if self.share is not None and self.fault != "a" and self.states[m] is self.share.states[m]:
            return self.share._pair_pass(m, h2)
        if (m, float(h2)) not in self._rows:
            self._rows[(m, float(h2))] = self._pair_rows(m, h2)
        return self._rows[(m, float(h2))]

    def _pair_rows(self, m, h2):
        """The partial rows of member m: per split (sum, (r2, index), within)."""
        T, n, alloc = self.T, self.sizes[m], self.alloc[m]
        splits, per = self.shape[m][2], self.shape[m][3]
        i = np.arange(n)
        p = self.pos[self.pos_off[m]:self.pos_off[m] + alloc + 8]
        v = self.vel[self.vel_off[m]:self.vel_off[m] + alloc + 8]
        out = []
        for s in range(splits):
            lo, hi = s * per * TILE, min(alloc, (s + 1) * per * TILE)
            stop = hi + 8 if self.fault == "a" and s == splits - 1 else hi
            jg = np.arange(lo, stop)
            with np.errstate(all="ignore"):
                r2 = np.full((n, stop - lo), T(EPS2), dtype=T)
                for c in range(3):
                    d = p[None, lo:stop, c] - p[i, None, c]
                    r2 = d * d + r2
                for c in range(3):  # a NaN operand comes out as it went in
                    nj, ni = np.isnan(p[lo:stop, c]), np.isnan(p[i, c])
                    r2[:, nj] = p[lo:stop, c][nj][None, :]
                    r2[ni, :] = p[i, c][ni][:, None]
                ok = (jg[None, :] < n) & (jg[None, :] != i[:, None])
                w = p[lo:stop, 3]
                total = ((w[None, :] * (v[None, lo:stop] - v[i, None])) / r2).sum(axis=1, dtype=T)
                within = ((~(r2 > h2) if self.fault == "d" else (r2 <= h2)) & ok).sum(axis=1).astype(np.int32)
            c = np.where(ok, r2, T(np.inf))
            best, bj = np.full(n, np.inf, dtype=T), np.full(n, -1, dtype=np.int32)
            key = c.view(self.bits) if self.fault == "c" else np.where(np.isnan(c), T(np.inf), c)
            at = key.argmin(axis=1)  # the first of equal values: the lowest j
            cand = c[i, at]
            take = self._less(cand, best)
            best[take], bj[take] = cand[take], jg[at][take]
            out.append((total, (best, bj), within))
        return out

    def call(self, first, count, h=MODEL_H):
        T = self.T
        h2 = T(T(h) * T(h) + T(EPS2))
        members = list(range(first, first + count))
        parts = {m: self._pair_pass(m, h2) for m in members}
        largest = max(members, key=lambda m: (self.sizes[m], -m))  # the first of the largest
        res, scalars = [], []
        for m in members:
            n = self.sizes[m]
            rows = [tuple(x[:n] if isinstance(x, np.ndarray) else (x[0][:n], x[1][:n]) for x in row) for row in parts[largest if self.fault == "b" else m]]
            with np.errstate(all="ignore"):
                total = rows[0][0].copy()
                for row in rows[1:]:
                    total = total + row[0]
                r2, j = self._merge([row[1] for row in rows])
                within = sum(row[2] for row in rows).astype(np.int32)
                vy = self.vel[self.vel_off[m]:self.vel_off[m] + n]
                cand = r2 / (T(1) + vy * vy)
                q = T(np.inf)
                for c in cand[~np.isnan(cand)]:
                    if c < q:
                        q = c
            scalars.append(q)
            res.append({"sum": total, "index": j, "r2": r2, "within": within})
        for k, r in enumerate(res):
            r["scalar"] = np.asarray(min(scalars) if self.fault == "e" else scalars[k])
        return res


_models = {}


def _control_model(sizes, precision, fault):
    key = (tuple(sizes), precision, fault)
    if key not in _models:
        _models[key] = Model(sizes, precision, fault).upload(clean_states(sizes, precision))
    return _models[key]


def model_tier_a(sizes, precision, fault, p, field, name, which, ranges=None):
    """Tier A on the model: the problems of the case, [] when the clean members are the clean control's over every range."""
    clean = clean_states(sizes, precision)
    b = body_of(which, sizes[p])
    states = list(clean)
    states[p] = poisoned(clean[p], field, name, b, precision)
    c = _control_model(sizes, precision, fault)
    o = Model(sizes, precision, fault).upload(states, share=c)
    bad = []
    for first, count in (ranges_a(len(sizes), p) if ranges is None else ranges):
        bad += tier_a(ModelFamily, o.call(first, count), c.call(first, count), first, count, p)
    return bad


def model_tier_b(sizes, precision, fault, p, name, which):
    """Tier B on the model: member p's kept rows under the position poison against the far control's (the neighbours rule)."""
    clean = clean_states(sizes, precision)
    b = body_of(which, sizes[p])
    states, control = list(clean), list(clean)
    states[p], control[p] = poisoned(clean[p], "pos_x", name, b, precision), far(clean[p], b)
    got = Model(sizes, precision, fault).upload(states).call(p, 1)[0]
    want = Model(sizes, precision, fault).upload(control).call(p, 1)[0]
    pick = lambda r: {k: r[k] for k in ("index", "r2", "within")}
    return tier_b("neighbours", pick(got), pick(want), b, sizes[p])[0]


# the cases of tests/test_jerk_gpu.py's velocity-poison test: two members of 257 bodies, the second one's body 0 poisoned, member
# 0's velocity-reading sums compared over the full range and over (0, 1)
def model_jerk_cases(precision, fault):
    sizes = (257, 257)
    clean = clean_states(sizes, precision)
    bad = []
    for name in ("+inf", "nan", "-inf"):
        states = [clean[0], poisoned(clean[1], "vel_y", name, 0, precision)]
        o, c = Model(sizes, precision, fault).upload(states), Model(sizes, precision, fault).upload(clean)
        for first, count in ((0, 2), (0, 1)):
            if not R._same_value(o.call(first, count)[0]["sum"], c.call(first, count)[0]["sum"]):
                bad.append((name, first, count))
    return bad
