"""The chain tables regrown with their contents kept (hge_engine.hip ensure_ccap), one
case per table family: an engine that starts at the smallest capacity takes a stream
online and must grow every chain table at least twice, keeping what the earlier calls
wrote; it has to end in the state of an engine that replays the same stream at full
capacity without growing.

Starting capacity in positions (init(), cap = 1024): 1024 / N + 1024 / (8 N) + 64, rounded
up to a multiple of 64; a growth goes to max(needed, 1.5 x) rounded up likewise.

  N    tables regrown                                        events   start -> longest chain
  12   int32 LA, FD and FDT; no FDTD                          4,800   192 -> over 400
  24   FDTD and FDTW; FSS padded rows                         7,200   128 -> over 300
  64   LA16 beside int32 FD and FDT                          16,000   128 -> over 250
  132  uint16 FD rows and runs, N % 64 != 0                  26,400   128 -> over 200

Each case asserts that its longest chain exceeds twice the starting capacity (two growths
at the least: 1.5 x does not reach it), so it cannot pass without growing.  Under uniform
gossip the longest of 132 chains over 26,400 events is about 230 positions, below 2 x 128:
the streams here let every fourth creator submit 1.4 times as often, which takes the
longest chain past 2 x 128 at the same N and event count and keeps it below the starting capacity
of the engine that replays at full capacity (asserted: that one never grows)."""
import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule

pytestmark = pytest.mark.gpu


def _start_positions(n, cap=1024):
    c0 = max(cap, 1024)
    return (c0 // n + c0 // (8 * n) + 64 + 63) // 64 * 64


def _stream(n, E, seed):
    """random_gossip's records (timestamps, signatures, hashes) under a creator sequence in
    which every fourth creator is drawn 1.4 times as often; the other-parent is the latest
    event of a uniformly drawn other creator, as in random_gossip."""
    dag = random_gossip(n, E, seed=seed)
    rng = np.random.default_rng(seed)
    w = np.where(np.arange(n) % 4 == 0, 1.4, 1.0)
    a = rng.choice(n, E - n, p=w / w.sum())
    b = rng.integers(0, n - 1, E - n)
    b = b + (b >= a)
    creator = np.concatenate([np.arange(n), a]).astype(np.int32)
    index = np.zeros(E, np.int32)
    sp = np.full(E, -1, np.int32)
    op = np.full(E, -1, np.int32)
    last = [-1] * n
    cnt = [0] * n
    for x in range(E):
        c = int(creator[x])
        index[x] = cnt[c]
        sp[x] = last[c]
        if x >= n:
            op[x] = last[int(b[x - n])]
        cnt[c] += 1
        last[c] = x
    dag.update(creator=creator, index=index, sp=sp, op=op)
    return dag


@pytest.mark.parametrize("n,E,start,needed", [(12, 4800, 192, 400), (24, 7200, 128, 300), (64, 16000, 128, 250),
                                              (132, 26400, 128, 200)])
def test_chain_tables_regrown_online_match_full_capacity_replay(n, E, start, needed):
    from babble_amd.engine import Engine, events_array
    assert _start_positions(n) == start
    dag = _stream(n, E, seed=1300 + n)
    longest = int(np.bincount(dag["creator"], minlength=n).max())
    assert longest > needed and longest > 2 * start
    assert longest + 1 <= _start_positions(n, E + 64)  # the reference engine below never grows
    # the last event inserted while every chain still fits the starting capacity
    # (upload() asks for the longest chain + 1 positions)
    before = int(np.flatnonzero(np.maximum.accumulate(dag["index"]) + 2 <= start)[-1])
    assert n < before < E // 2
    calls = schedule(E, n)
    a = Engine(n, E + 64)
    b = Engine(n, 1024)
    try:
        _, order, counts = a.replay(dag, calls)
        ev = events_array(dag)
        nxt, got = 0, []
        for c in calls:
            b.insert_events(ev[nxt:c].copy())
            got.append(len(b.run_consensus()))
            nxt = int(c)
        np.testing.assert_array_equal(b.consensus_events(), order)
        assert len(order) > E // 2
        np.testing.assert_array_equal(np.asarray(got, np.int64), np.asarray(counts, np.int64))
        assert b.rounds() == a.rounds()
        assert b.last_consensus_round() == a.last_consensus_round()
        for x, y in zip(a.event_rounds(), b.event_rounds()):
            np.testing.assert_array_equal(y, x)
        for x, y in zip(a.event_received(), b.event_received()):
            np.testing.assert_array_equal(y, x)
        for x in (0, before, E // 2, E - 1):
            for p, q in zip(a.coordinates(x), b.coordinates(x)):
                np.testing.assert_array_equal(q, p)
    finally:
        a.close()
        b.close()
