"""The direct rounds walk (k_rounds_direct, 32 < N, N % 4 == 0) selects each round's
frontier over 8-bit frontier-relative copies of its window rows and member slices
(babble_amd/csrc/hge_narrow.h), and takes the 16-bit select in a round whose values leave
the 7-bit range or lie below their base.  Every case checks the full state against the
oracle; Engine.walk_select_paths() says which path the chain-rounds took.
N = 64 is the kernel's smallest width (one narrow word per thread), N = 132 has columns
past N inside the 256-wide geometry, N = 256 is the headline width."""
import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule
from parity import compare_state, oracle_run, with_creators

pytestmark = pytest.mark.gpu

MIN_ORDERED = 1000


def fast_creator_stream(n, events, seed, weight=40):
    """Participant 0 creates events `weight` times as often as each other participant;
    every other-parent is the peer's latest event.  A slow chain's rows then jump by
    ~weight in column 0 from one row to the next: far outside the narrow range within
    a window, and the frontier of chain 0 advances by more than a window per round."""
    dag = random_gossip(n, events, seed=seed)  # timestamps, signatures, hashes
    rng = np.random.default_rng(seed + 1000)
    p = np.ones(n)
    p[0] = weight
    m = events - n
    a = rng.choice(n, m, p=p / p.sum())
    b = rng.integers(0, n - 1, m)
    b = b + (b >= a)
    creator = np.concatenate([np.arange(n), a]).astype(np.int32)
    sp = np.full(events, -1, np.int32)
    op = np.full(events, -1, np.int32)
    index = np.zeros(events, np.int32)
    last = list(range(n))
    count = [1] * n
    for i in range(m):
        e, c = n + i, int(a[i])
        sp[e], op[e], index[e] = last[c], last[int(b[i])], count[c]
        count[c] += 1
        last[c] = e
    dag.update(creator=creator, sp=sp, op=op, index=index)
    return dag


STREAMS = {
    # name: (N, E, K, stream)
    "plain64": (64, 6000, 100, lambda: random_gossip(64, 6000, seed=11)),
    "plain132": (132, 9240, 132, lambda: random_gossip(132, 9240, seed=7)),
    "plain256": (256, 20000, 500, lambda: random_gossip(256, 20000, seed=5)),
    "fast64": (64, 6000, 100, lambda: fast_creator_stream(64, 6000, seed=3)),
    "lag64": (64, 6000, 100, lambda: random_gossip(64, 6000, seed=13, op_lag=8)),
}
_refs = {}


def _reference(name):
    """(N, E, stream, calls, oracle, status, order, counts), computed once per stream."""
    if name not in _refs:
        n, e, k, make = STREAMS[name]
        dag = make()
        calls = schedule(e, k)
        o, ost, oorder, ocounts = oracle_run(dag, calls)
        _refs[name] = (n, e, dag, calls, o, ost, oorder, ocounts)
    return _refs[name]


def _replay_and_check(name, min_ordered=MIN_ORDERED):
    """Bulk replay of the stream, full state against the oracle; returns (narrow, exact)."""
    from babble_amd.engine import Engine
    n, e, dag, calls, o, ost, oorder, ocounts = _reference(name)
    eng = Engine(n, e)
    try:
        st, order, counts = eng.replay(dag, calls)
        with_creators(eng, dag, st)
        np.testing.assert_array_equal(st, ost, err_msg="admission status differs")
        assert len(order) == len(oorder) >= min_ordered, (len(order), len(oorder))
        np.testing.assert_array_equal(order, oorder, err_msg="consensus order differs")
        np.testing.assert_array_equal(counts, ocounts, err_msg="per-call batch sizes differ")
        compare_state(eng, o)
        paths = eng.walk_select_paths()
        print(f"{name}: rounds {eng.rounds()}, walk_select_paths (narrow, exact) = {paths}")
        return paths
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["plain64", "plain132", "plain256"])
def test_plain_streams_take_the_narrow_path(name):
    """Random gossip stays inside the 7-bit range (the frontier recurrence recomputed on
    the CPU: at most 75 above the base over the probed rows): the rounds select over the
    narrow rows, at most 1 % of the chain-rounds may be legitimate exact ones."""
    narrow, exact = _replay_and_check(name)
    assert narrow > 0, (narrow, exact)
    assert exact <= 0.01 * (narrow + exact), (narrow, exact)


def test_fast_creator_takes_the_exact_path():
    """One participant 40 times as fast as the others: window values far past the range
    (exact rounds), and a chain that advances by more than a window per round (the
    16-bit probe search behind the select)."""
    narrow, exact = _replay_and_check("fast64", min_ordered=200)
    assert exact > 0, (narrow, exact)


def test_exact_hook_same_state(monkeypatch):
    """HGE_TEST_DIR_EXACT=1: every round takes the 16-bit select, from the reloaded
    member slice.  Same state."""
    monkeypatch.setenv("HGE_TEST_DIR_EXACT", "1")
    narrow, exact = _replay_and_check("plain132")
    assert narrow == 0 and exact > 0, (narrow, exact)


def test_stale_other_parents():
    """op_lag = 8: other-parents up to 8 events behind their chain's head put many window
    values below the column's base (they encode as 0)."""
    narrow, exact = _replay_and_check("lag64", min_ordered=500)  # (stale parents: fewer rounds decided)
    assert narrow + exact > 0


def test_replay_then_online_calls():
    """60 calls replayed in bulk, then 10 online calls at N = 132: an online call's walk
    restarts a few rounds back and passes over frontier rows kept from earlier calls
    (no select: one 16-bit probe for their strongly-see bits) before it selects."""
    from babble_amd.engine import Engine, events_array
    n, e, dag, calls, o, ost, oorder, ocounts = _reference("plain132")
    e_replay = 7920
    ev = events_array(dag)
    nrep = int(np.searchsorted(calls, e_replay)) + 1
    assert calls[nrep - 1] == e_replay and len(calls) - nrep == 10
    eng = Engine(n, e)
    try:
        st, order, counts = eng.replay(ev[:e_replay], calls[:nrep])
        np.testing.assert_array_equal(st, ost[:e_replay])
        order, counts = list(order), list(counts)
        nxt = e_replay
        walked = 0
        for c in calls[nrep:]:
            eng.insert_events(ev[nxt:c].copy())
            got = eng.run_consensus()
            walked += sum(eng.walk_select_paths())
            order.extend(got)
            counts.append(len(got))
            nxt = int(c)
        assert walked > 0
        assert len(order) == len(oorder) >= MIN_ORDERED
        np.testing.assert_array_equal(np.asarray(order), oorder, err_msg="consensus order differs")
        np.testing.assert_array_equal(np.asarray(counts), ocounts, err_msg="per-call batch sizes differ")
        with_creators(eng, dag, ost)
        compare_state(eng, o)
    finally:
        eng.close()
