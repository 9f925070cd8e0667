"""Characterisation of what the host does with a forward's GhCounters word ([D, overflow bits, reserved0, reserved1]) on the paths a CPU
can drive: the sync-free record (_queue_readback + check_overflow), a captured graph's word (check_overflow in graph mode) and an
explicit word (report_counter_word). Every value of overflow bits 0-4 goes through each path, for split and unsplit call shapes, with
and without a DepthBoundCache / learn24, at D = 0, D <= max_instances and D > max_instances. What comes out (exception class and
message, learned capacity and GH_FLAG_DEPTH24 verdict, geometry caches cleared or not, the bound's state and misses) is compared with
tests/golden/counter_word_outcomes.json.gz (JSON, one case per line). No GPU: the read-back's (pinned buffer, event) pair is a CPU
tensor and a stand-in event.

Regenerate the golden file (only for a deliberate change of this policy): python tests/test_counter_word_cpu.py"""
import gzip
import itertools
import json
import os
import sys

import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from guassianhand_amd import rasterizer as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "counter_word_outcomes.json.gz")
DEV = 91            # a device index of its own: the state is reset for every case
CAP = 100           # the call's max_instances
CAP0 = 1800         # the shape's learned capacity before the call: 1.5 * max(D, R0) + 1024 outgrows it, 1.5 * D + 1024 does not
R0 = 800            # reserved0 (a split call: the capacity that would have sufficed; an unsplit call leaves P there)
DS = (0, 50, 500)   # D: nothing listed, within max_instances, beyond it
WORDS = range(32)   # overflow bits 0-4


class _Event:
    def record(self):
        pass

    def synchronize(self):
        pass

    def query(self):
        return True


def _reset():
    st = R._state(DEV)
    st.capacity.clear()
    st.depth24.clear()
    st.pending.clear()
    st.graph_counters.clear()
    st.free_slots.clear()
    st.last_D = -1
    return st


def _key(split):
    return (10, 2, 16, 16, split)


def _word(d, bits):
    return torch.tensor([d, bits, R0, 0], dtype=torch.int32)


def _raised(fn):
    try:
        fn()
    except R.GhOverflowError as e:
        return [type(e).__name__, str(e)]
    return None


def _outcome(st, key, raised, cache, bound):
    return dict(raised=raised, capacity=st.capacity.get(key), depth24=st.depth24.get(key), caches_cleared=cache.ctx is None,
                bound=None if bound is None else [bound.valid, bound.misses], last_D=st.last_D)


def _setup(split, d24):
    st = _reset()
    key = _key(split)
    st.capacity[key] = CAP0
    if d24 is not None:
        st.depth24[key] = d24
    cache = R.GeometryCache()
    cache.ctx = "lists"
    return st, key, cache


def sync_free_cases():
    """One sync-free record resolved by check_overflow, then a second check (a told record is not raised again)."""
    for bits, split, learn24, with_bound, d, d24 in itertools.product(WORDS, (False, True), (False, True), (False, True), DS, (None, False)):
        st, key, cache = _setup(split, d24)
        bound = None
        if with_bound:
            bound = R.DepthBoundCache()
            bound.valid = True
        st.free_slots.append((torch.zeros(4, dtype=torch.int32), _Event()))
        R._queue_readback(st, _word(d, bits), CAP, key, bound, learn24)
        out = _outcome(st, key, _raised(lambda: R.check_overflow(dev=DEV)), cache, bound)
        out.update(again=_raised(lambda: R.check_overflow(dev=DEV)), pending=len(st.pending), free_slots=len(st.free_slots))
        yield f"sync_free bits={bits} split={split} learn24={learn24} bound={with_bound} d={d} depth24={d24}", out


def captured_cases():
    """A workspace registered in graph mode: check_overflow reads its word directly."""
    for bits, split, full, d in itertools.product(WORDS, (False, True), (False, True), DS):
        st, key, cache = _setup(split, None)
        st.graph_counters[1] = (_word(d, bits), CAP, key, full)
        out = _outcome(st, key, _raised(lambda: R.check_overflow(dev=DEV)), cache, None)
        yield f"captured bits={bits} split={split} full={full} d={d}", out
    _reset()


def report_cases():
    """report_counter_word with the default and with a caller's `where` (fit.CapturedFitStep.check passes its own)."""
    for bits, split, learn24, d, where in itertools.product(WORDS, (False, True), (False, True), DS, ("", " [where]")):
        st, key, cache = _setup(split, None)
        raised = _raised(lambda: R.report_counter_word(key, bits, d, CAP, R0, dev=DEV, where=where, learn24=learn24))
        yield f"report bits={bits} split={split} learn24={learn24} d={d} where={where!r}", _outcome(st, key, raised, cache, None)


def order_cases():
    """Two bad sync-free records: which one check_overflow raises first (one error per call), and the other at the next call."""
    for a, b, d in itertools.product(range(1, 16), range(1, 16), (50, 500)):
        st, key, cache = _setup(False, None)
        for bits in (a, b):
            st.free_slots.append((torch.zeros(4, dtype=torch.int32), _Event()))
            R._queue_readback(st, _word(d, bits), CAP, key, None, True)
        yield f"order a={a} b={b} d={d}", [_raised(lambda: R.check_overflow(dev=DEV)) for _ in range(3)]
    _reset()


def outcomes():
    return dict(itertools.chain(sync_free_cases(), captured_cases(), report_cases(), order_cases()))


def _golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def test_counter_word_outcomes_match_the_golden_record():
    golden = _golden()
    got = json.loads(json.dumps(outcomes()))
    assert got.keys() == golden.keys()
    bad = [k for k in golden if got[k] != golden[k]]
    assert not bad, "\n".join(f"{k}:\n  got      {got[k]}\n  expected {golden[k]}" for k in bad[:5]) + f"\n({len(bad)} cases differ)"


def test_the_golden_record_covers_every_word_on_every_path():
    golden = _golden()
    for path in ("sync_free", "captured", "report"):
        assert {int(k.split()[1][5:]) for k in golden if k.startswith(path + " ")} == set(WORDS), path
    assert sum(k.startswith("order ") for k in golden) == 15 * 15 * 2


if __name__ == "__main__":
    with gzip.open(GOLDEN, "wt") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in outcomes().items()) + "\n}\n")
    print(f"wrote {GOLDEN}")
