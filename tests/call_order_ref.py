"""Call-order probes of the fourteen analysis calls (diagnostics, timescale, accel, field, neighbours, paircount, knn, fof, binaries,
tidal, tidal_bodies, clumps, nlist, jerk): the cases, the comparisons and a host model of the scratch they keep on the object.
Used by tests/test_call_order_cpu.py and tests/test_call_order_gpu.py; numpy only, no device.

Every call keeps device scratch on the object (csrc/nbx_object.hpp): partial rows, result records and scan arrays, grown and never
shrunk, and a ragged ensemble's member table, built by the first call.  The pair work writes only the rows a member owns, at the
stride of the range asked for; the finish must read exactly those.  The module tests make the full-range call first on a fresh
object, whose fresh allocation reads as zeros: a finish that reads a row too many, strides wrongly or looks a member up in the
wrong place can return the right bits there.  The headers promise the same bits for the same state "whatever range was asked,
wherever the member sits"; the sequence of test_call_order_gpu.py holds the library to it on an object whose history is
adversarial, and Model below shows on the host which planted fault which step of that sequence catches.

FAMILIES: per call how to make it on each kind of object -- the result is always a list of one dict of arrays per member of the
range, whatever the binding returns -- the keys compared, the keys in which a dirty state must show, and the arguments:
    field, tidal       m = 3 points, 1500, then 513 (other columns, another row length)
    knn                k = 1, 16
    paircount          1 radius, all 20 of paircount_ref.RADII (two passes), then 3
    nlist              a radius of about 0.5 neighbours per body, one of about 8 (the lists grow after the segments were sized)
    fof, neighbours    a radius of about 1.2 friends per body, one of about 4.5
    binaries           bound=False, bound=True
    clumps             the labels "blocks", "stripes" of clumps_ref
    the others         none
Shapes: a ragged ensemble of (5, 4097, 257, 2049, 513) -- 1, 4, 1, 2, 1 splits --, an ensemble of 3 x 2049, a context of 2049
bodies (4097 for the calls without an argument).  States: binaries_ref.cloud, a clean one per member -- seeds at which no body's
nearest neighbour or most bound partner is ambiguous in either precision, so that the modules' own comparisons apply -- and a
dirty one of the same size: another seed, positions scaled by 3, masses by 64.

truth_check() passes a full-range result for the clean states through the family's existing comparison with its existing gate
(jerk_ref.compare, clumps_ref.compare, binaries_ref.compare, field_ref.k_acc / k_phi and tidal_ref.k_metric under their gates,
knn_ref / nlist_ref / fof_ref / neighbours_ref.differs, paircount_ref.bracket, potential_ref.k_metric, force_ref.k_metric, and the
constants of tests/test_timescale_gpu.py and tests/test_diagnostics_gpu.py): no new tolerance.  For members above 513 bodies the
O(n^2) truths in the wide type are taken at sampled rows (both sides of every column and split seam, the ends, every 37th body).
"""
import numpy as np

import binaries_ref as B
import clumps_ref as C
import energy_ref as E
import field_ref as FR
import fof_ref as FOF
import force_ref as F
import jerk_ref as J
import knn_ref as KN
import neighbours_ref as NB
import nlist_ref as NL
import paircount_ref as PC
import potential_ref as P
import tidal_ref as TD
import timescale_ref as TS

KINDS = ("context", "ensemble", "ragged")
RAGGED_SIZES = (5, 4097, 257, 2049, 513)
RAGGED_SPLITS = (1, 4, 1, 2, 1)
ENSEMBLE = (3, 2049)
CONTEXT_N = {True: 2049, False: 4097}  # by "the family takes an argument"
DT = 1.0 / 64  # of the one step of the sequence: the accelerations are of the order of n, so every body moves by a visible amount
RANGES = {"ragged": ((0, 2), (2, 3), (3, 2)), "ensemble": ((0, 2), (1, 2), (2, 1)), "context": ()}
NARROW = (2, 1)  # the first call an object sees: a sub-range that does not start at 0
AXES = ("ax", "ay", "az")

# (n, variant) -> seed of binaries_ref.cloud: tests/test_call_order_cpu.py holds each to "nothing ambiguous, in either precision"
CLEAN_SEEDS = {(5, 0): 905, (257, 0): 163, (513, 0): 128, (2049, 0): 112, (2049, 1): 2112, (2049, 2): 3112, (4097, 0): 123}
DIRTY_OFFSET = 50000


def sizes_of(kind, takes_argument=True):
    return {"context": (CONTEXT_N[bool(takes_argument)],), "ensemble": (ENSEMBLE[1],) * ENSEMBLE[0], "ragged": RAGGED_SIZES}[kind]


def member_keys(sizes):
    """(n, variant) per member: equal sizes take variants 0, 1, 2, ...; a size met in several kinds of object is one state."""
    seen, out = {}, []
    for n in sizes:
        out.append((n, seen.get(n, 0)))
        seen[n] = seen.get(n, 0) + 1
    return out


_states = {}


def clean_state(key, precision):
    if ("clean", key, precision) not in _states:
        _states[("clean", key, precision)] = B.cloud(key[0], precision, seed=CLEAN_SEEDS[key])
    return _states[("clean", key, precision)]


def dirty_state(key, precision):
    """The same size from another seed, positions scaled by 3 and masses by 64 (exact in T), velocities as they come (nonzero)."""
    if ("dirty", key, precision) not in _states:
        s = {k: v.copy() for k, v in B.cloud(key[0], precision, seed=CLEAN_SEEDS[key] + DIRTY_OFFSET).items()}
        for f in B.POS:
            s[f] = s[f] * s[f].dtype.type(3)
        s["mass"] = s["mass"] * s["mass"].dtype.type(64)
        _states[("dirty", key, precision)] = s
    return _states[("dirty", key, precision)]


def states(sizes, precision):
    keys = member_keys(sizes)
    return [clean_state(k, precision) for k in keys], [dirty_state(k, precision) for k in keys]


def sample_rows(n):
    """None (every body) up to 513 bodies; else the ends, both sides of every column and split seam and every 37th body."""
    if n <= 513:
        return None
    columns, tiles, splits, per = FR.field_shape(n, n)
    rows = {0, n - 1}
    for s in [c * FR.COL for c in range(1, columns)] + [s * per * FR.TILE for s in range(1, splits)]:
        rows.update((s - 1, s))
    rows.update(range(5, n, 37))
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


# ---- shapes the sequence relies on ---------------------------------------------------------------------------------------------------
def ragged_shapes(sizes=RAGGED_SIZES):
    """[(columns, splits)] of the bodies-on-bodies pair work of every member: field_shape(n, n)."""
    return [(FR.field_shape(n, n)[0], FR.field_shape(n, n)[2]) for n in sizes]


def range_stride(first, count, sizes=RAGGED_SIZES):
    """The row stride of a ragged call over [first, first + count): the largest split count of the range."""
    return max(FR.field_shape(n, n)[2] for n in sizes[first:first + count])


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
POINTS = {"small": 3, "large": 1500, "middle": 513}
NLIST_DEGREES = {"small": 0.5, "large": 8.0}
FRIEND_DEGREES = {"small": 1.2, "large": 4.5}
PAIRCOUNT_RADII = {"small": PC.RADII[7:8], "large": PC.RADII, "middle": PC.RADII[5:16:5]}
_args = {}


def _radius(sizes, precision, degree):
    """One radius for all clean members of the object: fof_ref.pick_radius, the middle of the widest gap between pair r2 values."""
    key = ("radius", tuple(sizes), precision, degree)
    if key not in _args:
        _args[key] = FOF.pick_radius(states(sizes, precision)[0], FOF.target_radius(2049, degree))
    return _args[key]


def _points(sizes, precision, m):
    key = ("points", tuple(sizes), precision, m)
    if key not in _args:
        # seeded by the state, not by the member's place: one state has one set of points in every kind of object
        _args[key] = [FR.make_points(precision, st, m, "box", seed=k[1]) for k, st in zip(member_keys(sizes), states(sizes, precision)[0])]
    return _args[key]


def _labels(sizes, precision, family):
    return [C.labels(family, st, precision) for st in states(sizes, precision)[0]]


# ---- one result form for every kind of object ----------------------------------------------------------------------------------------
def _rng(kind, first, count):
    return {} if kind == "context" else {"first": first, "count": count}


def _by_member(res, kind, count):
    """A context's dict, an ensemble's dict of (count, ...) arrays or a ragged ensemble's list of dicts as a list of dicts."""
    if kind == "context":
        return [res]
    if isinstance(res, dict):
        return [{k: (None if v is None else v[m]) for k, v in res.items()} for m in range(count)]
    return list(res)


def _plain(name, argument=False):
    def call(o, kind, sizes, arg, first, count):
        a = (arg,) if argument else ()
        return _by_member(getattr(o, name)(*a, **_rng(kind, first, count)), kind, count)
    return call


def _scalars(name, drop):
    def call(o, kind, sizes, arg, first, count):
        res = getattr(o, name)(**_rng(kind, first, count))
        return [{k: np.asarray(v) for k, v in d.items() if k not in drop} for d in ([res] if kind == "context" else res)]
    return call


def _accel(o, kind, sizes, arg, first, count):
    a = o.accel(**_rng(kind, first, count))
    if kind == "context":
        return [dict(zip(AXES, a))]
    if kind == "ensemble":
        return [dict(zip(AXES, [c[m] for c in a])) for m in range(count)]
    return [dict(zip(AXES, m)) for m in a]


def _at_points(name):
    def call(o, kind, sizes, arg, first, count):
        if kind == "context":
            return [getattr(o, name)(*arg[0])]
        p = [np.stack([arg[m][c] for m in range(first, first + count)]) for c in range(3)]
        return _by_member(getattr(o, name)(*p, first=first, count=count), "ensemble", count)
    return call


def _tidal_bodies(o, kind, sizes, arg, first, count):
    res = o.tidal_bodies(**_rng(kind, first, count))
    if kind != "ragged":
        return _by_member(res, kind, count)
    at = np.concatenate([[0], np.cumsum(sizes[first:first + count])]).astype(int)  # one array per key, the members end to end
    assert all(len(v) == at[-1] for v in res.values())
    return [{k: v[at[m]:at[m + 1]] for k, v in res.items()} for m in range(count)]


def _clumps(o, kind, sizes, arg, first, count):
    if kind == "context":
        return [o.clumps(arg[0])]
    lab = arg[first:first + count]
    return _by_member(o.clumps(np.stack(lab) if kind == "ensemble" else lab, first=first, count=count), kind, count)


def _nlist(o, kind, sizes, arg, first, count):
    """One result for the range, offsets running across the members: cut into the members' own (offsets from 0)."""
    res = o.nlist(arg, **_rng(kind, first, count))
    assert res["index"] is not None and int(res["offsets"][-1]) == res["total"] == len(res["index"]) == len(res["r2"])
    out, at = [], 0
    for n in (sizes if kind == "context" else sizes[first:first + count]):
        off = res["offsets"][at:at + n + 1]
        lo, hi = int(off[0]), int(off[-1])
        out.append({"offsets": off - lo, "index": res["index"][lo:hi], "r2": res["r2"][lo:hi], "total": np.asarray(hi - lo)})
        at += n
    assert at + 1 == len(res["offsets"])
    return out


def _fof(o, kind, sizes, arg, first, count):
    """"passes" is the call's -- the largest of its members' own -- and is kept with every member of the result."""
    res = o.fof(arg, **_rng(kind, first, count))
    if kind == "ensemble":
        res = [{"label": res["label"][m], "size": res["size"][m], "groups": res["groups"][m], "largest": res["largest"][m],
                "passes": res["passes"]} for m in range(count)]
    return [{k: np.asarray(v) for k, v in d.items()} for d in ([res] if kind == "context" else res)]


def _paircount(o, kind, sizes, arg, first, count):
    res = o.paircount(arg, **_rng(kind, first, count))
    return [{"counts": res}] if kind == "context" else [{"counts": res[m]} for m in range(count)]


def _binaries(o, kind, sizes, arg, first, count):
    return _by_member(o.binaries(bound=arg, **_rng(kind, first, count)), kind, count)


class Family:
    def __init__(self, name, call, keys, dirt=None, args=None, names=("small", "large"), call_wide=()):
        self.name, self.call, self.keys = name, call, keys
        self._names = names if args else ("large",)  # the arguments in the order small, large, middle, as far as the family has them
        self.dirt = keys if dirt is None else dirt  # the keys a dirty state must show in
        self._args = args                            # (sizes, precision) -> {"small", "large"[, "middle"]}, or None
        self.call_wide = call_wide                   # keys that are the call's, not the member's: compared on full ranges only

    @property
    def takes_argument(self):
        return self._args is not None

    def names(self):
        return self._names

    def args(self, sizes, precision):
        return self._args(sizes, precision) if self._args else {"large": None}


DIAG_KEYS = ("mass", "kenergy", "potential", "momentum", "mass_moment", "i_count", "etotal")
FAMILIES = {f.name: f for f in (
    # steps_done is the object's counter, not a function of the state: the fresh object of step 4 has taken no step
    Family("diagnostics", _scalars("diagnostics", ("steps_done",)), DIAG_KEYS, dirt=("mass", "kenergy", "potential", "momentum", "mass_moment", "etotal")),
    Family("timescale", _scalars("timescale", ("steps_done",)), TS.KEYS + ("n",), dirt=TS.KEYS),
    Family("accel", _accel, AXES),
    Family("field", _at_points("field"), FR.KEYS, names=("small", "large", "middle"), args=lambda s, p: {k: _points(s, p, m) for k, m in POINTS.items()}),
    Family("neighbours", _plain("neighbours", True), NB.KEYS, args=lambda s, p: {k: _radius(s, p, d) for k, d in FRIEND_DEGREES.items()}),
    Family("paircount", _paircount, ("counts",), names=("small", "large", "middle"), args=lambda s, p: dict(PAIRCOUNT_RADII)),
    Family("knn", _plain("knn", True), KN.KEYS, args=lambda s, p: {"small": 1, "large": 16}),
    Family("fof", _fof, ("label", "size", "groups", "largest", "passes"), dirt=("label", "size"), call_wide=("passes",),
           args=lambda s, p: {k: _radius(s, p, d) for k, d in FRIEND_DEGREES.items()}),
    Family("binaries", _binaries, B.KEYS, args=lambda s, p: {"small": False, "large": True}),
    Family("tidal", _at_points("tidal"), TD.KEYS, names=("small", "large", "middle"), args=lambda s, p: {k: _points(s, p, m) for k, m in POINTS.items()}),
    Family("tidal_bodies", _tidal_bodies, TD.KEYS),
    # "members" is a function of the labels alone: the dirty state, under the same labels, cannot show in it
    Family("clumps", _clumps, C.KEYS, dirt=C.FLOAT_KEYS, args=lambda s, p: {"small": _labels(s, p, "blocks"), "large": _labels(s, p, "stripes")}),
    Family("nlist", _nlist, NL.KEYS, dirt=("offsets", "index", "r2"), args=lambda s, p: {k: _radius(s, p, d) for k, d in NLIST_DEGREES.items()}),
    Family("jerk", _plain("jerk"), J.KEYS),
)}
assert len(FAMILIES) == 14


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
def _same_value(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind in "iub":
        return bool(np.array_equal(a, b))
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()  # -0.0 and 0.0 differ, NaN equals itself


def differences(family, got, want, full_range=True):
    """Where two results -- lists of one dict per member -- differ in a bit: ["member 1: r2", ...]; integers by np.array_equal,
    floats as bytes.  A key that is the call's (fof's passes) is compared where both calls had the full range; on a sub-range it
    may not exceed the full range's."""
    if len(got) != len(want):
        return ["%d members against %d" % (len(got), len(want))]
    out = []
    for m, (g, w) in enumerate(zip(got, want)):
        for k in family.keys:
            if k in family.call_wide and not full_range:
                if not 1 <= int(g[k]) <= int(w[k]):
                    out.append("member %d: %s = %d outside [1, %d]" % (m, k, int(g[k]), int(w[k])))
            elif not _same_value(g[k], w[k]):
                out.append("member %d: %s" % (m, k))
    return out


def clean_keys(family, got, want):
    """The keys of family.dirt in which `got` does NOT differ from `want` anywhere (all members taken together): empty when the
    dirt is dirt."""
    return [k for k in family.dirt if all(_same_value(g[k], w[k]) for g, w in zip(got, want))]


# ---- the existing comparisons --------------------------------------------------------------------------------------------------------
_truths = {}


def _cached(key, make):
    if key not in _truths:
        _truths[key] = make()
    return _truths[key]


def _gate_constants():
    import test_diagnostics_gpu as TDG  # the constants and the check the module tests themselves use
    import test_timescale_gpu as TTG
    return TDG._check_against_ref, TTG.RATE_GATE, TTG.R2_GATE


def _check_member(name, precision, key, st, got, arg, oracle):
    """Problems (a list of texts) of one member's result against the family's own reference."""
    n, u = key[0], F.U[precision]
    rows = sample_rows(n)
    at = np.arange(n) if rows is None else rows
    tag = (name, precision, key) + ((tuple(arg) if isinstance(arg, list) else arg,) if name in ("knn", "nlist", "fof", "neighbours", "paircount") else ())
    if name == "jerk":
        c = J.case(precision, n, "cloud", state=st, rows=rows, name="call order %r" % (key,))
        return J.compare(J.at_rows(got, c["truth"]["rows"]), c["truth"], c["gates"], precision)[0]
    if name == "clumps":
        c = C.case(precision, n, "stripes", state=st, rows=rows, name="call order %r" % (key,))
        assert np.array_equal(c["label"], arg)
        return C.compare(got, c["truth"], c["gates"], st, c["label"], precision)[0]
    if name == "binaries":
        assert B.ambiguity(st, precision) == 0
        want = _cached(tag, lambda: B.binaries(st, precision, rows=rows))
        return B.compare(got, want, st, precision, bound=True, rows=rows)[0]
    if name == "accel":
        tr, gate = _cached(tag, lambda: (lambda tr: (tr, F.gate(F.k_metric(F.oracle_accel(oracle, st, rows), tr, precision).max())))(F.state_truth(st, rows)))
        k = F.k_metric(np.stack([got[a][at] for a in AXES], axis=1), tr, precision).max()
        return [] if k <= gate else ["K = %.3g above the gate %.3g" % (k, gate)]
    if name == "field":
        def make():
            tr = FR.truth(st, arg, precision)
            return tr, F.gate(FR.k_acc(FR.oracle_acc(oracle, st, arg), tr, precision).max()), F.gate(FR.k_phi(FR.phi_sequential(st, arg, precision), tr, precision).max())
        tr, gate_acc, gate_phi = _cached(tag, make)
        ka, kp = FR.worst(got, {"truth": tr}, precision)
        zero = tr["acc"][2] == 0
        bad = [k for k in FR.KEYS[:3] if (got[k][zero] != 0).any()]
        return (["acc K = %.3g above %.3g" % (ka, gate_acc)] if not ka <= gate_acc else []) + (["phi K = %.3g above %.3g" % (kp, gate_phi)] if not kp <= gate_phi else []) + bad
    if name in ("tidal", "tidal_bodies"):
        bodies = name == "tidal_bodies"
        pts, r = (TD.positions(st), rows) if bodies else (arg, None)
        def make():
            tr = TD.truth(st, pts, precision, bodies=bodies, rows=r)
            return tr, TD.gate(TD.k_metric(TD.sequential(st, pts, precision, bodies=bodies, rows=r), tr, precision).max(), precision)
        tr, gate = _cached(tag, make)
        k = TD.k_metric(got, tr, precision, rows=r).max()
        return [] if k <= gate else ["K = %.3g above the gate %.3g" % (k, gate)]
    if name == "knn":
        want, gap = _cached(tag, lambda: (KN.knn(st, arg, precision), KN.first_gap(st, precision)))
        return KN.differs(got, want, st, precision, gap=gap)
    if name == "nlist":
        assert not NL.ambiguous(st, arg, precision)
        return NL.differs(got, _cached(tag, lambda: NL.nlist(st, arg, precision)), precision)
    if name == "fof":
        assert not FOF.ambiguous(st, arg, precision)
        return FOF.differs(got, _cached(tag, lambda: FOF.fof(st, arg, precision)), passes=False)
    if name == "neighbours":
        assert NB.ambiguity(st, arg, precision) == (0, 0)
        return ["differs from neighbours_ref.neighbours"] if NB.differs(got, _cached(tag, lambda: NB.neighbours(st, arg, precision)), precision) else []
    if name == "paircount":
        lo, hi = _cached(tag, lambda: PC.bracket(st, arg, precision, PC.pair_r2(st)))
        c = np.asarray(got["counts"])
        ok = c.dtype == np.uint64 and c.shape == (len(arg),) and (lo <= c).all() and (c <= hi).all() and (np.diff(c.astype(np.int64)) >= 0).all()
        return [] if ok else ["counts %r outside [%r, %r]" % (c.tolist(), lo.tolist(), hi.tolist())]
    check_against_ref, rate_gate, r2_gate = _gate_constants()
    if name == "diagnostics":
        tr, gate, ref, scale = _cached(tag, lambda: (lambda tr: (tr, F.gate(P.k_metric(P.restated(st, precision), tr, precision)[0]), E.diagnostics(st), E.momentum_scale(st)))(P.truth_total(st, precision)))
        k = float(np.max(P.k_metric(got["potential"], tr, precision)))
        check_against_ref(got, ref, scale, 1e-5 if precision == 32 else 1e-12)
        return ([] if k <= gate else ["potential K = %.3g above the gate %.3g" % (k, gate)]) + ([] if int(got["i_count"]) == n else ["i_count"])
    if name == "timescale":
        want = _cached(tag, lambda: TS.timescale(st))
        dev = {f: abs(float(got[f]) - want[f]) / want[f] / u for f in TS.KEYS}
        return ["%s %.3g u" % (f, d) for f, d in dev.items() if not d <= (r2_gate if f == "min_r2" else rate_gate[precision])] + ([] if int(got["n"]) == n else ["n"])
    raise ValueError(name)


def truth_check(family, kind, precision, result, oracle=None, sizes=None):
    """The full-range result of `family`'s large argument for the clean states of a `kind` object, member by member, through the
    family's existing comparison with its existing gate: a list of texts, empty when all is well.  oracle: the CPU restatement
    (conftest's fixture), whose K is K_ref of the accelerations of accel and field."""
    fam = FAMILIES[family] if isinstance(family, str) else family
    sizes = sizes_of(kind, fam.takes_argument) if sizes is None else sizes
    arg = fam.args(sizes, precision)["large"]
    per_member = fam.name in ("field", "tidal", "clumps")
    out = []
    for m, key in enumerate(member_keys(sizes)):
        got = {k: (None if result[m][k] is None else np.asarray(result[m][k])) for k in fam.keys}
        problems = _check_member(fam.name, precision, key, clean_state(key, precision), got, arg[m] if per_member else arg, oracle)
        out += ["member %d (%d bodies): %s" % (m, key[0], p) for p in problems]
    return out


# ---- the sequence --------------------------------------------------------------------------------------------------------------------
def sequence(kind, names):
    """The history of one object as [(label, state, argument, first, count)]; state "dirty", "clean" or "stepped"; count None: the
    full range.  Labels are the step numbers of the tests' docstrings.  names: the family's arguments (Family.names())."""
    small, large = names[0], "large"
    batch = kind != "context"
    S = len(sizes_of(kind))
    full = (0, None)
    out = [("1", "dirty", small) + (NARROW if batch else full), ("2", "dirty", large) + full, ("3.1", "clean", large) + full]
    if batch:
        out += [("3.2 member %d" % m, "clean", large, m, 1) for m in range(S)]
        out += [("3.3 range (%d, %d)" % r, "clean", large) + r for r in RANGES[kind]]
    out += [("3.4 %s" % a, "clean", a) + full for a in (small,) + names[2:] if a != large or len(names) == 1]
    out += [("3.5", "clean", large) + full, ("3.6", "clean", large) + full, ("4", "stepped", large) + full]
    return out


# ---- a host model of the scratch -------------------------------------------------------------------------------------------------------
FAULTS = {"a": "the finish walks the range's row_splits, not the member's own",
          "b": "the finish strides by the member's own splits",
          "c": "the member table is built from the first call's `first`, not from member 0",
          "d": "the finish uses the layout (k, passes, m) of the previous call",
          "e": "a grown buffer keeps its old capacity figure"}


class Model:
    """One object's partial rows as the pair-work kernels and their finish use them, in plain numpy.  `splits[m]` rows of `items`
    values belong to member m; a call over [first, first + count) lays member first + k at k * stride * items, stride the largest
    split count of the range; the pair pass writes only the rows a member owns, the finish adds them.  The scratch is never
    cleared: a fresh allocation reads as zeros (what hipMalloc hands out on a quiet machine), a grown one is a new allocation.
    The capacity figure bounds what the pass may write -- with fault "e" a write past the stale figure is dropped, where the
    device would write out of bounds, which no comparison of values models.  A value is a function of (state, member, split,
    item), an integer, so that sums are exact in any order; expect() is the sum over the member's own splits."""

    def __init__(self, splits, fault=None):
        assert fault is None or fault in FAULTS
        self.splits, self.fault = tuple(splits), fault
        self.mem, self.cap, self.table, self.last_items = np.zeros(0), 0, None, None

    @staticmethod
    def value(state, member, split, items):
        return ((state * 7919 + member * 104729 + split * 1299709 + items * 611953 + np.arange(items) * 15485863) % 1000003 + 1).astype(np.float64)

    def expect(self, state, first, count, items):
        return [sum(self.value(state, m, s, items) for s in range(self.splits[m])) for m in range(first, first + count)]

    def call(self, state, first, count, items):
        S = len(self.splits)
        if self.table is None:  # built by the first call, fixed for the object's life
            shift = first if self.fault == "c" else 0
            self.table = tuple(self.splits[(m + shift) % S] for m in range(S))
        own = [self.table[first + k] for k in range(count)]
        stride = max(own)
        need = count * stride * items
        if need > self.cap:  # free, allocate, new capacity
            self.mem = np.zeros(need)
            if self.fault != "e" or self.cap == 0:
                self.cap = need
        for k in range(count):  # the pair pass: the rows a member owns, nothing else
            for s in range(own[k]):
                at = (k * stride + s) * items
                if at + items <= self.cap:
                    self.mem[at:at + items] = self.value(state, first + k, s, items)
        fin_items = self.last_items if self.fault == "d" and self.last_items is not None else items
        self.last_items = items
        out = []
        for k in range(count):  # the finish
            walk = stride if self.fault == "a" else own[k]
            base = k * (own[k] if self.fault == "b" else stride) * fin_items
            rows = [self.mem[base + s * fin_items:base + s * fin_items + items] for s in range(walk)]
            out.append(sum(np.concatenate([r, np.zeros(items - len(r))]) for r in rows))
        return out

    def run(self, history, items_of, states_of={"dirty": 1, "clean": 2, "stepped": 3}):
        """The labels of `history` -- [(label, state, argument, first, count)] -- at which a call's result is not expect()'s."""
        S = len(self.splits)
        bad = []
        for label, state, arg, first, count in history:
            count = S - first if count is None else count
            if first + count > S:  # a range the object has no members for
                continue
            got = self.call(states_of[state], first, count, items_of[arg])
            want = self.expect(states_of[state], first, count, items_of[arg])
            if not all(np.array_equal(g, w) for g, w in zip(got, want)):
                bad.append(label)
        return bad


MODEL_ITEMS = {"small": 3, "large": 16, "middle": 7}
OLD_ORDER = [("full", "clean", "large", 0, None), ("again", "clean", "large", 0, None), ("range (0, 1)", "clean", "large", 0, 1),
             ("range (0, 2)", "clean", "large", 0, 2)]
