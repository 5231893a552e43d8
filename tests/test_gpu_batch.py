"""The batch engine (hge_batch_*, hge_batch.hip: many independent hashgraphs, one
launch per stage) against the oracle, field by field: admission status, order,
per-call batches, every event's round and witness flag, the fame of every
(round, creator) slot, round received, consensus timestamps, the undetermined
list and the scalars (tests/golden/digest.py's state).

The graphs cover N from 1 to 64, forkers and fork cascades (every admission
error), call schedules from K = 1 to one call for the whole stream (a batch
past the LDS sort, the global-scratch path), other-parents that are not their
chain's head (op_lag), coin rounds (one call over the whole stream at N = 4, 32 and
64, the widest; at N = 4, 5 and 8 with coin-bit votes taken: COIN_CASES), and a second
run of the same batch.  The call schedule runs in bulk (hge_batch_bulk.hip); a graph past
the bulk fold's 256 rounds is replayed call by call by kb_consensus in the same
run, and HGB_SERIAL=1 puts every graph through kb_consensus.

Every stream here keeps random_gossip's own timestamps (1 us apart, in submission order)
and uniform S.  The timestamps of real clocks are test_gpu_batch_timestamps.py's, on the
shapes of ts_shapes.py at N = 4, 5, 32, 33 and 64, in bulk, under HGB_SERIAL=1 and with the
commit records delivered: median offsets outside int32 and on +-INT32_MAX (kb_median's
exact rank search, kb_consensus's twin of it, the register sort's filler value), call
buckets whose timestamps span 2^28 ns or more (kb_sort unpacked, every comparison from
HBM) or one less (the packed field's top bit), and keys equal down to S's last limb
(key_less past the first limb in every sort).  One branch no stream reaches: a call
bucket received over 16 rounds or more, the other half of kb_sort's packing condition.
test_gpu_sort_kernels.py drives kb_sort alone on such buckets (a round span of exactly 15,
16 and 40; tests/abi/hge_batch_sort_kernel_test.hip)."""
import os
import sys

import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

CASES = [
    # n, events, k, seed, forkers, fork_p, cascade_p, op_lag
    (4, 1000, 4, 1, 0, 0.0, 0.0, 0),
    (4, 1000, 1, 2, 0, 0.0, 0.0, 0),
    (4, 1500, 1500, 12, 0, 0.0, 0.0, 0),     # one call: coin rounds, a 1.4k-key batch (global sort)
    (1, 50, 5, 3, 0, 0.0, 0.0, 0),
    (1, 700, 5, 5, 0, 0.0, 0.0, 0),          # ~700 rounds: past the bulk fold, replayed by kb_consensus
    (2, 300, 2, 3, 0, 0.0, 0.0, 0),
    (5, 2000, 3, 13, 0, 0.0, 0.0, 0),
    (7, 3000, 7, 14, 2, 0.1, 0.5, 0),
    (16, 3000, 16, 2, 0, 0.0, 0.0, 0),
    (16, 4000, 50, 21, 0, 0.0, 0.0, 6),      # other-parents behind their chain's head
    (32, 3000, 32, 4, 10, 0.05, 0.5, 0),     # config 5's graph shape with cascades
    (32, 4000, 32, 16, 10, 0.05, 0.0, 0),
    (32, 2500, 2500, 22, 0, 0.0, 0.0, 0),    # one call at N = 32
    (32, 5000, 700, 25, 0, 0.0, 0.0, 0),     # 513-1,024-key batches: the LDS sort pads to 1,024
    (16, 4000, 900, 26, 2, 0.05, 0.5, 0),
    (33, 3000, 50, 17, 0, 0.0, 0.0, 3),
    (48, 5000, 48, 23, 5, 0.05, 0.5, 0),
    (64, 6000, 64, 18, 0, 0.0, 0.0, 0),
    (64, 3000, 7, 24, 0, 0.0, 0.0, 2),
    (8, 2400, 2400, 5, 0, 0.0, 0.0, 3),      # one call: coin-bit votes (hashgraph.go:647) at N = 8
    (5, 1500, 1500, 12, 0, 0.0, 0.0, 3),     # and at N = 5
    (32, 11000, 11000, 22, 0, 0.0, 0.0, 0),  # one call: coin rounds at config 5's width, 10k ordered
    (64, 48000, 48000, 79, 0, 0.0, 0.0, 0),  # and at the widest
]
# the cases whose oracle run must show the coin branch: what its statistics must count.
# (One-shot streams take no coin-bit vote at wide N: every coin round is entered with a
# supermajority, DESIGN.md's testing section.)  These must also stay in bulk (fame_pair):
# a silent fall to kb_consensus would hide it.
COIN_CASES = {CASES[-4]: "coin_votes", CASES[-3]: "coin_votes", CASES[-2]: "coin_evals", CASES[-1]: "coin_evals"}
_WANT = {}


def _stream(n, E, k, seed, fk, fp, cp, lag):
    dag = random_gossip(n, E, seed=seed, forkers=fk, fork_p=fp, cascade_p=cp, op_lag=lag)
    return dag, schedule(len(dag["creator"]), k)


def _oracle(case, dag, calls):
    """The oracle's state of a case, computed once (read only; the long streams in the
    oracle's scale mode); a coin case's statistics asserted."""
    from make_mc_digests import oracle_state
    if case not in _WANT:
        stats = {}
        _WANT[case] = oracle_state(dag, calls, scale=case[1] > 10000, stats=stats)
        if case in COIN_CASES:
            assert stats[COIN_CASES[case]] > 0, (case, stats)
    return _WANT[case]


@pytest.mark.parametrize("n", sorted({c[0] for c in CASES}))
def test_batch_matches_oracle(n):
    from babble_amd.engine import Batch
    from digest import first_difference
    cases = [c for c in CASES if c[0] == n]
    streams = [_stream(*c) for c in cases]
    b = Batch(n)
    try:
        for dag, calls in streams:
            b.add(dag, calls)
        tot = b.run()
        if any(c in COIN_CASES for c in cases):
            assert b.fallbacks() == 0
        want = [_oracle(c, dag, calls) for c, (dag, calls) in zip(cases, streams)]
        assert tot == sum(len(w["order"]) for w in want)
        for rep in range(2):  # a second replay of the staged batch gives the same state
            for g, (case, w) in enumerate(zip(cases, want)):
                got = b.state(g)
                diff = first_difference(got, w)
                assert diff is None, f"case {case}: first differing field {diff}"
            if rep == 0:
                b.run()
    finally:
        b.close()


def test_batch_many_graphs_one_launch_per_stage():
    """256 graphs of config 5's shape in one batch, each equal to the oracle."""
    from babble_amd.engine import Batch
    from digest import first_difference
    from make_mc_digests import oracle_state
    streams = [_stream(32, 1200, 32, 7000 + g, 10, 0.05, 0.5, 0) for g in range(256)]
    b = Batch(32)
    try:
        for dag, calls in streams:
            b.add(dag, calls)
        b.run()
        ms = b.kernel_ms()
        assert set(ms) == {"kb_coords", "kb_fd", "kb_fdrows", "kb_front", "kb_fame", "kb_fold", "kb_receive",
                           "kb_order"}
        assert b.fallbacks() == 0  # every graph in bulk
        # 256 graphs: one per compute unit of an MI355X (test_gpu_batch_variants.py goes past it)
        plan = b.launch_plan()
        assert (plan["coords"], plan["front_threads"], plan["ns"]) == (1, 1024, 3), plan
        for g in range(0, 256, 5):
            w = oracle_state(*streams[g])
            assert first_difference(b.state(g), w) is None, f"graph {g}"
    finally:
        b.close()


def test_batch_refuses_bad_arguments():
    from babble_amd.engine import Batch, HgeError
    with pytest.raises(HgeError):
        Batch(65)
    b = Batch(4)
    try:
        dag, _ = _stream(4, 100, 4, 1, 0, 0.0, 0.0, 0)
        with pytest.raises(HgeError):
            b.add(dag, np.array([5, 3], np.int64))  # not ascending
        with pytest.raises(HgeError):
            b.info(0)  # no graph yet
    finally:
        b.close()


@pytest.mark.parametrize("n", [4, 5, 8, 32, 64])
def test_batch_serial_path_matches_oracle(n, monkeypatch):
    """HGB_SERIAL=1: every graph through the call-by-call kb_consensus (the bulk
    path's fallback), against the oracle."""
    from babble_amd.engine import Batch
    from digest import first_difference
    monkeypatch.setenv("HGB_SERIAL", "1")
    cases = [c for c in CASES if c[0] == n]
    streams = [_stream(*c) for c in cases]
    b = Batch(n)
    try:
        for dag, calls in streams:
            b.add(dag, calls)
        b.run()
        assert b.fallbacks() == len(cases)
        for g, (case, (dag, calls)) in enumerate(zip(cases, streams)):
            diff = first_difference(b.state(g), _oracle(case, dag, calls))
            assert diff is None, f"case {case}: first differing field {diff}"
    finally:
        b.close()


def test_batch_fallback_mixed_with_bulk():
    """One batch holding a graph past the bulk fold (N = 1, ~700 rounds) and bulk
    graphs: only that graph is replayed by kb_consensus, all equal the oracle."""
    from babble_amd.engine import Batch
    from digest import first_difference
    from make_mc_digests import oracle_state
    cases = [c for c in CASES if c[0] == 1]
    streams = [_stream(*c) for c in cases]
    b = Batch(1)
    try:
        for dag, calls in streams:
            b.add(dag, calls)
        b.run()
        assert b.fallbacks() == 1
        for g, (case, (dag, calls)) in enumerate(zip(cases, streams)):
            assert first_difference(b.state(g), oracle_state(dag, calls)) is None, f"case {case}"
    finally:
        b.close()
