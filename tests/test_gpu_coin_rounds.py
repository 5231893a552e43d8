"""Streams long enough that DecideFame's j loop reaches diff = N (the coin branch,
hashgraph.go:643-649) at the widths the benchmark uses, against the live oracle.

The wide cases compare field by field with the scale-mode oracle (test_oracle_scale.py
pins it to the plain mode): N = 64 in one call (k_fame_decide_blk<1> on the one-call
path), in four calls (the same kernel through fame_decide, the timeline and the LCR
scan, rounds above the new LCR decided again) and through insert_events + one
run_consensus; N = 96 (k_fame_decide<2>); N = 128 (k_fame_decide_blk<2>, 146 rounds:
past the one-call path's 128); N = 192 (k_fame_decide_blk<3>).  N = 256 is left to
the kernel test (test_gpu_fame_kernel.py): a stream that long is too slow for the
suite.  Every case asserts that the oracle evaluated the coin branch and ordered more
than half the stream, so order, round received and timestamps downstream of the
re-decided fame are compared on something.

One-shot streams enter every coin round at wide N with a supermajority (coin_votes = 0:
DESIGN.md, testing); the three streams at N = 5 and N = 8 whose coin rounds do take
coin-bit votes run through run_case, every field per event."""
import functools
import os
import sys

import numpy as np
import pytest

from babble_amd.gossip import random_gossip
from parity import compare_golden, run_case

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

SEED = 79


@functools.lru_cache(maxsize=2)
def _stream(n, events):
    return random_gossip(n, events, seed=SEED)


@functools.lru_cache(maxsize=2)
def _oracle(n, events, calls):
    """(golden fields, DecideFame statistics) of the scale-mode oracle; shared, read only."""
    from make_golden import describe
    from oracle.oracle import replay
    dag = _stream(n, events)
    o, status, order, counts = replay(dag, np.array(calls, np.int64), scale=True)
    assert o.is_scale()
    g = describe(o, dag, status, order, counts, np.array(calls, np.int64))
    st = o.stats()
    o.close()
    assert st["coin_evals"] > 0
    assert 2 * len(order) > len(dag["creator"]), (len(order), len(dag["creator"]))
    return g, st


class _Online:
    """An engine fed by insert_events and one run_consensus, behind the replay call
    compare_golden makes (the stream has no rejected events: ids = submission indices)."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def replay(self, dag, calls):
        from babble_amd.engine import events_array
        assert len(calls) == 1 and calls[0] == len(dag["creator"])
        status = self._eng.insert_events(events_array(dag))
        order = self._eng.run_consensus()
        return status, order, np.array([len(order)], np.int64)


def _run(n, events, calls, online=False):
    from babble_amd.engine import Engine
    g, _ = _oracle(n, events, tuple(calls))
    eng = Engine(n, events + 64)
    try:
        compare_golden(_Online(eng) if online else eng, _stream(n, events), g)
    finally:
        eng.close()


def test_coin_rounds_n64_one_call():
    _run(64, 48000, [48000])


def test_coin_rounds_n64_four_calls():
    _run(64, 48000, [45000, 46000, 47000, 48000])


def test_coin_rounds_n64_online():
    _run(64, 48000, [48000], online=True)


@pytest.mark.parametrize("n,events", [(96, 125_000), (128, 230_000), (192, 560_000)])
def test_coin_rounds_wide_one_call(n, events):
    _run(n, events, [events])


@pytest.mark.parametrize("n,events,seed,op_lag", [(8, 2400, 5, 3), (5, 1500, 12, 3), (5, 10500, 4, 40)])
def test_coin_bit_votes_one_call(n, events, seed, op_lag):
    """DecideFame takes the middle bit of y's hash (hashgraph.go:647) on these streams."""
    from babble_amd.engine import Engine
    eng = Engine(n, events + 64)
    try:
        o, order = run_case(eng, random_gossip(n, events, seed=seed, op_lag=op_lag), events)
        assert o.stats()["coin_votes"] > 0
        assert 2 * len(order) > events
    finally:
        eng.close()
