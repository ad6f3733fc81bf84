"""Every analysis call on an object whose scratch is dirty (tests/call_order_ref.py): fourteen families x context, ensemble, ragged
ensemble x fp32, fp64.  The module tests ask a fresh object for the full range first; here one object O goes through

  1    created, the DIRTY states uploaded, the narrowest call first: members (2, 1) -- a sub-range that does not start at 0 builds the
       ragged table and sizes every buffer -- with the small argument
  2    the widest call on the dirty states: full range, large argument.  The buffers grow; every row of the widest layout now
       holds values of the wrong state.  The result must differ from the clean expectation in every output array
  3    the clean states uploaded, then
  3.1  full range, large argument                3.2  every member alone, (m, 1)
  3.3  the ranges (0, 2), (2, 3), (3, 2) (an ensemble of three members: (0, 2), (1, 2), (2, 1))
  3.4  full range, small argument, then the middle one where the family has three
  3.5  full range, large argument again          3.6  the same call once more
  4    O.step(1, dt, kenergy=False): the other position buffer is current.  The full-range call must equal that of a fresh
       object that was uploaded O.download() with the clean masses and asked once, and must differ from 3.1
  5    truth_check on result 3.1 of O -- the dirtied object -- so that the expectation below is not taken on trust

and every result of 3 is compared bit for bit (integers by np.array_equal, floats as bytes) with the FIRST call of a fresh
object of the same kind that holds the clean states and is asked for the same argument over the full range, then sliced.  For a
context the ranges fall away and the arguments stay.  fof's "passes" is the call's, the largest of its members' own: it is
compared on full ranges and may not exceed the full range's on a sub-range; diagnostics' and timescale's steps_done is the
object's counter and is left out.  One more test per kind: all fourteen families in turn on ONE object, dirtied and cleaned as
above, in list order and reversed -- the families share no scratch, and this pins that down.

Per-case wall time and number of calls go to call_order.json in the GPU suite's report directory (OUT of
tests/test_parity_gpu.py).

Measured on an MI355X, the module alone in a fresh process: 96 cases in 21 s of wall time, 1.5 s of it the first import and
library load; the slowest case (field, ragged, fp64) 1.6 s, every other under 1 s.  The 9 to 20 device calls of a case with
their comparisons take 3 to 170 ms (nlist on the ragged ensemble the most); the rest of a case is the truth check on the host.
An all-families case makes 56 or 70 calls in about 20 ms.  Nothing failed -- every comparison held bit for bit in every case --
and nothing in csrc/ had to be fixed.
"""
import json
import os
import time

import numpy as np
import pytest

import call_order_ref as R

pytestmark = pytest.mark.gpu

RECORDS = []
_fresh = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    from test_parity_gpu import OUT  # where the GPU suite leaves its reports
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "call_order.json"), "w") as f:
        json.dump({"what": "wall time in seconds and analysis calls made per case of tests/test_call_order_gpu.py", "cases": RECORDS,
                   "total_s": sum(r["seconds"] for r in RECORDS)}, f, indent=1)


def make(nbx, kind, sizes, precision):
    if kind == "context":
        return nbx.Context(sizes[0], precision)
    return nbx.Ensemble(sizes[0], len(sizes), precision) if kind == "ensemble" else nbx.Ragged(sizes, precision)


def upload(o, kind, states):
    o.upload(states[0] if kind == "context" else states)


def download(o, kind, masses):
    """The resident state as a list of state dicts, with the masses given."""
    d = o.download()
    if kind == "context":
        d = [d]
    elif kind == "ensemble":
        d = [{f: v[m] for f, v in d.items()} for m in range(len(masses))]
    return [dict(s, mass=st["mass"]) for s, st in zip(d, masses)]


def fresh(nbx, fam, kind, precision, sizes, name):
    """The first call of a fresh object that holds the clean states: the full range, argument `name`.  Asked once, left unchanged."""
    key = (fam.name, kind, precision, tuple(sizes), name)
    if key not in _fresh:
        with make(nbx, kind, sizes, precision) as e:
            upload(e, kind, R.states(sizes, precision)[0])
            _fresh[key] = fam.call(e, kind, sizes, fam.args(sizes, precision)[name], 0, len(sizes))
    return _fresh[key]


class Counted:
    """fam.call on one object, counted."""

    def __init__(self, o, kind, sizes, precision):
        self.o, self.kind, self.sizes, self.precision, self.calls = o, kind, sizes, precision, 0

    def __call__(self, fam, name, first=0, count=None):
        self.calls += 1
        count = len(self.sizes) - first if count is None else count
        return fam.call(self.o, self.kind, self.sizes, fam.args(self.sizes, self.precision)[name], first, count)


def dirty_calls(ask, fam, want_large, where):
    """Steps 1 and 2 on an object that holds the dirty states."""
    batch = ask.kind != "context"
    got = ask(fam, fam.names()[0], *(R.NARROW if batch else ()))
    assert len(got) == 1
    got = ask(fam, "large")
    assert not R.clean_keys(fam, got, want_large), (where, "step 2: the dirty state does not show in", R.clean_keys(fam, got, want_large))


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_the_same_state_gives_the_same_bits_whatever_the_object_has_been_asked_before(nbx, oracle, family, kind, precision):
    t0 = time.perf_counter()
    fam = R.FAMILIES[family]
    sizes = R.sizes_of(kind, fam.takes_argument)
    S = len(sizes)
    clean, dirty = R.states(sizes, precision)
    where = (family, kind, precision)
    want = {name: fresh(nbx, fam, kind, precision, sizes, name) for name in fam.names()}
    with make(nbx, kind, sizes, precision) as o:
        ask = Counted(o, kind, sizes, precision)
        upload(o, kind, dirty)
        dirty_calls(ask, fam, want["large"], where)
        upload(o, kind, clean)
        first_clean = None
        for label, state, name, first, count in R.sequence(kind, fam.names()):
            if state != "clean":
                continue
            count = S - first if count is None else count
            got = ask(fam, name, first, count)
            bad = R.differences(fam, got, want[name][first:first + count], full_range=count == S)
            assert not bad, (where, "step " + label, bad)
            if label == "3.1":
                first_clean = got
        o.step(1, R.DT, kenergy=False)
        stepped = ask(fam, "large")
        moved = download(o, kind, clean)
    with make(nbx, kind, sizes, precision) as e:
        upload(e, kind, moved)
        bad = R.differences(fam, stepped, fam.call(e, kind, sizes, fam.args(sizes, precision)["large"], 0, S))
    assert not bad, (where, "step 4", bad)
    assert R.differences(fam, stepped, first_clean), (where, "step 4: the step does not show")
    seconds_device = time.perf_counter() - t0
    problems = R.truth_check(fam, kind, precision, first_clean, oracle)
    RECORDS.append({"family": family, "kind": kind, "precision": precision, "calls": ask.calls + 1 + len(fam.names()),
                    "seconds": time.perf_counter() - t0, "seconds_before_the_truth_check": seconds_device})
    print(json.dumps(RECORDS[-1]))
    assert not problems, (where, "step 5", problems)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("order", ["list order", "reversed"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_all_fourteen_families_in_turn_on_one_object(nbx, kind, order, precision):
    """One object: every family's narrow and wide call on the dirty states, then, on the clean ones, every family's full-range
    large call, member 2 alone and the small argument, each against the fresh expectation.  A context has 2049 bodies here for
    every family."""
    t0 = time.perf_counter()
    fams = list(R.FAMILIES.values())[::-1 if order == "reversed" else 1]
    sizes = R.sizes_of(kind)
    S = len(sizes)
    clean, dirty = R.states(sizes, precision)
    want = {(f.name, name): fresh(nbx, f, kind, precision, sizes, name) for f in fams for name in ("large", f.names()[0])}
    with make(nbx, kind, sizes, precision) as o:
        ask = Counted(o, kind, sizes, precision)
        upload(o, kind, dirty)
        for f in fams:
            dirty_calls(ask, f, want[(f.name, "large")], (f.name, kind, order, precision))
        upload(o, kind, clean)
        for f in fams:
            where = (f.name, kind, order, precision)
            assert not R.differences(f, ask(f, "large"), want[(f.name, "large")]), where
            if kind != "context":
                first, count = R.NARROW
                bad = R.differences(f, ask(f, "large", first, count), want[(f.name, "large")][first:first + count], full_range=False)
                assert not bad, (where, bad)
            assert not R.differences(f, ask(f, f.names()[0]), want[(f.name, f.names()[0])]), where
    RECORDS.append({"family": "all, " + order, "kind": kind, "precision": precision, "calls": ask.calls, "seconds": time.perf_counter() - t0})
    print(json.dumps(RECORDS[-1]))
