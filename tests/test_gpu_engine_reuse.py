"""One engine over two streams.  An engine is made dirty on stream A, then re-used for
stream B through Engine.reset() (hge_reset) or a replay (hge_replay_prepare), and every
field it reports is compared with a fresh engine on B and with the oracle on B.  B is
shorter than A and comes from other seeds, so state that survived the reset would lie
inside A's extent.  Everything on this path is an integer: every assertion is equality.

Widths: 8 (k_la_seq and the single-call kernels), 32 (sweeps), 34 (the N % 4 != 0 walk),
64 (direct walk, narrow rows), 132 (uint16 FD rows, k_median_rows, stale FD timestamp
rows).  About 40 N events in A, 25 N in B, RunConsensus every 16 events."""
import functools

import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule
from parity import compare_state, oracle_run, with_creators

pytestmark = pytest.mark.gpu

K = 16
WIDTHS = [8, 32, 34, 64, 132]


def _fields(eng):
    """Everything the engine reports in bulk, as comparable arrays."""
    rounds, wit = eng.event_rounds()
    rr, cts = eng.event_received()
    lcr = eng.last_consensus_round()
    return {
        "rounds()": np.int64(eng.rounds()),
        "last_consensus_round": np.int64(-1 if lcr is None else lcr),
        "last_committed_round_events": np.int64(eng.last_committed_round_events()),
        "consensus_transactions": np.int64(eng.consensus_transactions()),
        "event_count": np.int64(eng.event_count()),
        "known": np.asarray(eng.known()),
        "undetermined": np.asarray(eng.undetermined()),
        "consensus_events": np.asarray(eng.consensus_events()),
        "consensus_log": np.asarray(eng.consensus_log()),
        "event_rounds": np.asarray(rounds),
        "witness": np.asarray(wit),
        "event_received": np.asarray(rr),
        # (an event without a round received has no consensus timestamp: the table keeps
        # whatever an earlier stream left there, as the other suites' comparisons allow)
        "consensus_timestamps": np.where(np.asarray(rr) >= 0, np.asarray(cts), 0),
        "fame_table": np.asarray(eng.fame_table()),
    }


@functools.lru_cache(maxsize=None)
def _streams(n):
    """(A, B, B's calls, the oracle on B with its results, a fresh engine's fields on B),
    computed once per width and left unchanged."""
    from babble_amd.engine import Engine, events_array
    a = random_gossip(n, 40 * n, seed=7100 + n)
    b = random_gossip(n, 25 * n, seed=8000 + n)
    calls = schedule(25 * n, K)
    o, ost, oorder, ocounts = oracle_run(b, calls)
    fresh = Engine(n, 40 * n + 64)
    try:
        st, order, counts = fresh.replay(b, calls)
        np.testing.assert_array_equal(st, ost)
        np.testing.assert_array_equal(order, oorder)
        np.testing.assert_array_equal(counts, ocounts)
        want = _fields(fresh)
    finally:
        fresh.close()
    return events_array(a), events_array(b), b, calls, (o, ost, oorder, ocounts), want


def _assert_empty(eng, n):
    """Right after reset(), before anything else."""
    assert eng.rounds() == 0
    assert eng.last_consensus_round() is None
    assert len(eng.undetermined()) == 0
    assert len(eng.consensus_events()) == 0
    assert len(eng.consensus_log()) == 0
    np.testing.assert_array_equal(eng.known(), np.zeros(n, np.int64))
    assert eng.event_count() == 0


def _online(eng, ev, calls, first=0):
    """InsertEvent + RunConsensus at every call point from `first` on; (order, counts)."""
    order, counts = [], []
    nxt = first
    for c in calls:
        if c <= first:
            continue
        eng.insert_events(ev[nxt:c].copy())
        got = eng.run_consensus()
        order.extend(int(x) for x in got)
        counts.append(len(got))
        nxt = int(c)
    return np.asarray(order, np.int64), np.asarray(counts, np.int64)


def _assert_b(eng, n, order, counts):
    """The re-used engine on B: against the fresh engine field by field, and the oracle."""
    _, _, dag_b, _, (o, ost, oorder, ocounts), want = _streams(n)
    np.testing.assert_array_equal(order, oorder, err_msg="consensus order differs from the oracle")
    np.testing.assert_array_equal(counts, ocounts, err_msg="per-call batches differ from the oracle")
    got = _fields(eng)
    for name, w in want.items():
        np.testing.assert_array_equal(got[name], w, err_msg=f"{name} differs from a fresh engine")
    np.testing.assert_array_equal(got["consensus_log"], oorder, err_msg="consensus_log differs from the oracle")
    with_creators(eng, dag_b, ost)
    compare_state(eng, o, check_events=n <= 34)


@pytest.fixture
def engine():
    made = []

    def make(n):
        from babble_amd.engine import Engine
        made.append(Engine(n, 40 * n + 64))
        return made[-1]
    yield make
    for e in made:
        e.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_reset_after_a_replay_then_online(engine, n):
    """(a) replay A, reset(): the engine reports an empty store; then B online."""
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    eng = engine(n)
    eng.replay(ev_a, schedule(len(ev_a), K))
    assert eng.rounds() > 0 and eng.event_count() == len(ev_a)
    eng.reset()
    _assert_empty(eng, n)
    order, counts = _online(eng, ev_b, calls)
    _assert_b(eng, n, order, counts)


@pytest.mark.parametrize("n", WIDTHS)
def test_replay_after_a_replay(engine, n):
    """(b) replay A, then replay B on the same engine."""
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    eng = engine(n)
    eng.replay(ev_a, schedule(len(ev_a), K))
    _, order, counts = eng.replay(ev_b, calls)
    _assert_b(eng, n, order, counts)


@pytest.mark.parametrize("n", WIDTHS)
def test_reset_mid_stream_then_replay_and_online_tail(engine, n):
    """(c) A online part-way (undetermined events, a log), reset(), B's head as a replay
    and its tail online (at N = 132 the tail reads the FD timestamp rows the replay's end
    refreshed)."""
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    eng = engine(n)
    # (these streams commit their first events between 0.4 and 0.93 of A's length)
    part = [c for c in schedule(len(ev_a), K) if c <= (15 * len(ev_a)) // 16]
    _online(eng, ev_a, part)
    assert len(eng.undetermined()) > 0 and len(eng.consensus_log()) > 0
    eng.reset()
    _assert_empty(eng, n)
    head = [int(c) for c in calls if c <= (3 * len(ev_b)) // 5]
    _, order, counts = eng.replay(ev_b[:head[-1]].copy(), head)
    order2, counts2 = _online(eng, ev_b, calls, first=head[-1])
    _assert_b(eng, n, np.concatenate([order, order2]), np.concatenate([counts, counts2]))


def test_reset_with_a_coordinate_step_pending(engine):
    """(d) split_begin() on A leaves the coordinate step pending; reset(), then B online."""
    n = 64
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    eng = engine(n)
    eng.prepare(ev_a, schedule(len(ev_a), K))
    eng.split_begin()
    eng.reset()
    _assert_empty(eng, n)
    order, counts = _online(eng, ev_b, calls)
    _assert_b(eng, n, order, counts)


def test_replay_prepare_drops_the_split_plan(engine):
    """(e) a split-emulate record and a split plan on A, then B is staged: split_run
    refuses (a plan belongs to the stream it was made for), a plain replay of B is exact."""
    from babble_amd.dist import ROUND_EVENTS_PER_PARTICIPANT, split_plan
    from babble_amd.engine import HgeError
    n = 64
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    eng = engine(n)
    eng.prepare(ev_a, schedule(len(ev_a), K))
    eng.split_emulate(True)
    n_a = eng.run()
    eng.split_plan(0, 2, split_plan(eng.call_events(), eng.event_count(), 2, 8 * ROUND_EVENTS_PER_PARTICIPANT * n))
    eng.clear_exchange()
    assert eng.split_run() == n_a
    eng.prepare(ev_b, calls)
    with pytest.raises(HgeError) as ei:
        eng.split_run()
    assert ei.value.code == -8 and "no split plan" in str(ei.value)
    eng.run()
    _, order, counts = eng.fetch()
    _assert_b(eng, n, order, counts)


# A's longest chain crosses the limit, B's stays below it (asserted)
WIDE_N, WIDE_LIMIT = 40, 46


def test_reset_returns_to_packed_positions(engine, monkeypatch):
    """(f) HGE_CHAIN_LIMIT low: A crosses to int32 positions (its rounds come from
    k_round_step32: the direct walk's select counters stay untouched), reset(), B stays on
    the packed path (the direct walk counts its selects) and is exact."""
    n = WIDE_N
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    assert np.bincount(ev_a["creator"], minlength=n).max() > WIDE_LIMIT
    assert np.bincount(ev_b["creator"], minlength=n).max() < WIDE_LIMIT
    monkeypatch.setenv("HGE_CHAIN_LIMIT", str(WIDE_LIMIT))
    eng = engine(n)
    eng.replay(ev_a, schedule(len(ev_a), K))
    assert eng.rounds() > 0
    assert eng.walk_select_paths() == (0, 0)
    eng.reset()
    _assert_empty(eng, n)
    order, counts = _online(eng, ev_b, calls)
    assert sum(eng.walk_select_paths()) > 0
    _assert_b(eng, n, order, counts)


def test_reset_after_a_failed_widening(engine, monkeypatch):
    """(g) HGE_TEST_W32_FAIL: the switch to int32 positions fails part-way on A (the runs
    widened, the FD rows not); reset(): the engine accepts B and is exact."""
    from babble_amd.engine import HgeError
    n = 132
    ev_a, ev_b, _, calls, _, _ = _streams(n)
    monkeypatch.setenv("HGE_CHAIN_LIMIT", "20")
    monkeypatch.setenv("HGE_TEST_W32_FAIL", "2")
    eng = engine(n)
    with pytest.raises(HgeError) as ei:
        _online(eng, ev_a, schedule(len(ev_a), K))
    assert "to_wide32 stopped" in str(ei.value)
    eng.reset()
    _assert_empty(eng, n)
    order, counts = _online(eng, ev_b, calls)
    _assert_b(eng, n, order, counts)
