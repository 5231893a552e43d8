"""The batch engine's device front (hge_batch_generate / hge_batch_clear /
hge_batch_submissions, hge_batch_gen.hip; Batch.generate / clear / submissions): graphs
generated, admitted and staged by kernels, against counter_gossip (the same stream on the
host), the oracle and a second Batch fed the same streams through add().

The sizes are the walk's boundaries: streams of one step past a 64-step chunk, one short of
two and many chunks (events 65, 127, 600; N itself: the initial events alone), N = 1 and 2
(no peer, no third creator), N = 33 and 64 (the lane boundary), every step forking, every
twin cascading, lagging other-parents, and call points that fall on refused submissions
(K = 1).  At N = 64 and 600 events a parent is looked up past the walk's LDS window of 256
submissions (asserted below), so the map's global side is read too.  Graphs past the bulk
fold (kb_consensus) are the N = 1 ones of ~320 and ~700 rounds."""
import itertools
import os
import sys

import numpy as np
import pytest

from babble_amd.gossip import counter_gossip, schedule

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

HGE_ERR_ARG = -8
NS = [1, 2, 3, 5, 32, 33, 64]
ONE_CALL = 1 << 40
FIELDS = ("creator", "index", "sp", "op", "ts", "S", "hash", "ntx", "honest")
_cache = {}


def _corners(n):
    """(forkers, fork_p, cascade_p, op_lag): none, config 5's shape, every step forking
    and every twin cascading, with and without lag."""
    some = max(1, n // 3)
    return [(0, 0.0, 0.0, 0), (some, 0.05, 0.5, 3), (n, 1.0, 1.0, 0), (n, 1.0, 0.5, 3), (some, 1.0, 0.0, 0)]


def _groups(n, events_list):
    """One generate() call each: (events, k, graphs, seed, forkers, fork_p, cascade_p, op_lag),
    the batch sizes 1, 3, 5 and K = 1, N, one call going round."""
    out = []
    for j, (events, corner) in enumerate(itertools.product(events_list, _corners(n))):
        out.append((events, (1, n, ONE_CALL)[j % 3], (1, 3, 5)[(j // 3) % 3], 1000 * n + 10 * j) + corner)
    return out


def _want(n, events, k, seed, fk, fp, cp, lag, state=False):
    """The host's statement of one generated graph, computed once and left unchanged:
    (stream, call points, oracle admission status or full state)."""
    key = (n, events, k, seed, fk, fp, cp, lag)
    if key not in _cache:
        dag = counter_gossip(n, events, seed, fk, fp, cp, lag)
        _cache[key] = [dag, schedule(len(dag["creator"]), min(k, len(dag["creator"]))), None, None]
    c = _cache[key]
    if state and c[3] is None:
        from make_mc_digests import oracle_state
        c[3] = oracle_state(c[0], c[1])
        c[2] = c[3]["status"]
    if c[2] is None:
        from oracle.oracle import replay
        c[2] = replay(c[0], c[1][-1:])[1]
    return c


def _generate(b, groups):
    """The groups appended; [(graph, its _want key)]"""
    graphs = []
    for events, k, count, seed, fk, fp, cp, lag in groups:
        g0 = b.generate(events, k, count, seed, fk, fp, cp, lag)
        graphs += [(g0 + i, (b.n, events, k, seed + i, fk, fp, cp, lag)) for i in range(count)]
    assert b.graphs() == len(graphs)
    return graphs


def _check_stream(b, g, key):
    dag, _, status, _ = _want(*key)
    got = b.submissions(g)
    assert len(got["creator"]) == len(dag["creator"]), key
    for f in FIELDS:
        assert np.array_equal(got[f], dag[f]), f"{key}: {f}"
        assert got[f].dtype == np.asarray(dag[f]).dtype, f"{key}: {f} dtype"
    assert np.array_equal(got["status"], status), f"{key}: status"


@pytest.mark.parametrize("n", NS)
def test_raw_stream_and_admission(n):
    from babble_amd.engine import Batch
    b = Batch(n)
    try:
        graphs = _generate(b, _groups(n, sorted({e for e in (n, 65, 127, 600) if e >= n})))
        b.stage()
        refused = 0
        for g, key in graphs:
            _check_stream(b, g, key)
            refused += int((_want(*key)[2] < 0).sum())
        assert refused > 0
    finally:
        b.close()


def test_a_parent_is_looked_up_past_the_lds_window():
    """What the module docstring promises of N = 64, 600 events: some parent is more than
    256 submissions behind its child."""
    far = 0
    for events, k, count, seed, fk, fp, cp, lag in _groups(64, [600]):
        d = _want(64, events, k, seed, fk, fp, cp, lag)[0]
        i = np.arange(len(d["creator"]))
        far += int(((i - d["sp"] > 256) & (d["sp"] >= 0)).sum() + ((i - d["op"] > 256) & (d["op"] >= 0)).sum())
    assert far > 0


STATE_GROUPS = {
    # n: generate() calls; the N = 1 batch holds a graph past the bulk fold's 256 rounds (~320; the
    # ~700-round one is test_full_state_past_the_bulk_fold's)
    1: [(320, 5, 1, 5, 0, 0.0, 0.0, 0), (50, 5, 3, 7, 1, 1.0, 1.0, 0), (65, 1, 1, 8, 1, 0.5, 0.0, 3)],
    2: [(300, 2, 3, 21, 1, 0.3, 1.0, 2), (127, 1, 1, 24, 2, 1.0, 1.0, 0)],
    3: [(600, 3, 1, 31, 3, 1.0, 1.0, 0), (65, ONE_CALL, 3, 32, 1, 0.05, 0.5, 3)],
    5: [(600, 1, 5, 51, 2, 0.3, 0.5, 3), (600, ONE_CALL, 1, 56, 0, 0.0, 0.0, 0)],
    32: [(1200, 32, 3, 321, 10, 0.05, 0.5, 0), (600, 1, 1, 324, 32, 1.0, 1.0, 3)],
    33: [(900, 50, 3, 331, 11, 0.1, 0.5, 3)],
    64: [(1500, 64, 1, 641, 20, 0.05, 0.5, 2), (600, 7, 3, 642, 64, 1.0, 1.0, 0)],
}


def _check_states(b, twin, graphs):
    from digest import first_difference
    for g, key in graphs:
        w = _want(*key, state=True)[3]
        got = b.state(g)
        assert first_difference(got, w) is None, f"{key}: first differing field {first_difference(got, w)}"
        if twin is not None:
            assert first_difference(got, twin.state(g)) is None, f"{key}: differs from the add-built batch"
            assert b.info(g) == twin.info(g), key


def _built_by_add(n, graphs):
    from babble_amd.engine import Batch
    twin = Batch(n)
    for _, key in graphs:
        dag, calls = _want(*key)[:2]
        twin.add(dag, calls)
    return twin


@pytest.mark.parametrize("n", sorted(STATE_GROUPS))
def test_full_state(n):
    from babble_amd.engine import Batch
    b, twin = Batch(n), None
    try:
        graphs = _generate(b, STATE_GROUPS[n])
        twin = _built_by_add(n, graphs)
        assert b.run() == twin.run()
        assert b.fallbacks() == twin.fallbacks() == (1 if n == 1 else 0)
        for g, key in graphs:
            _check_stream(b, g, key)
        _check_states(b, twin, graphs)
        b.run()  # a second replay of the staged batch
        _check_states(b, None, graphs)
    finally:
        b.close()
        if twin is not None:
            twin.close()


def test_full_state_past_the_bulk_fold():
    """N = 1, 700 events (~700 rounds): kb_consensus serves a generated graph.  One run,
    against the oracle: a run of this graph is ~9 s of kb_consensus, added or generated, so
    the add-built twin of a graph past the fold is test_full_state[1]'s ~320-round one."""
    from babble_amd.engine import Batch
    b = Batch(1)
    try:
        graphs = _generate(b, [(700, 5, 1, 5, 0, 0.0, 0.0, 0)])
        b.run()
        assert b.fallbacks() == 1
        _check_stream(b, *graphs[0])
        _check_states(b, None, graphs)
    finally:
        b.close()


@pytest.mark.parametrize("n", [5, 33])
def test_full_state_serial(n, monkeypatch):
    """HGB_SERIAL=1: every generated graph through kb_consensus."""
    from babble_amd.engine import Batch
    monkeypatch.setenv("HGB_SERIAL", "1")
    b = Batch(n)
    try:
        graphs = _generate(b, STATE_GROUPS[n])
        b.run()
        assert b.fallbacks() == len(graphs)
        _check_states(b, None, graphs)
    finally:
        b.close()


@pytest.mark.parametrize("n", [1, 5, 32])
def test_delivery(n):
    """With delivery on (bits 0 and 1) a generated batch's commit streams are the
    add-built batch's."""
    from babble_amd.engine import Batch
    b, twin = Batch(n), None
    try:
        graphs = _generate(b, STATE_GROUPS[n])
        twin = _built_by_add(n, graphs)
        for x in (b, twin):
            x.deliver(order=True, received=True)
            x.run()
        assert b.delivered() == twin.delivered() == 1
        for g, key in graphs:
            got, want = b.commits(g), twin.commits(g)
            w = _want(*key, state=True)[3]
            assert np.array_equal(got["ids"], w["order"]), key
            for f in ("ids", "rr", "cts", "counts"):
                assert np.array_equal(got[f], want[f]), f"{key}: {f}"
        _check_states(b, twin, graphs)
    finally:
        b.close()
        if twin is not None:
            twin.close()


def test_clear_and_reuse():
    from babble_amd.engine import Batch
    first = [(300, 5, 3, 70, 2, 0.3, 0.5, 0)]
    larger = [(900, 5, 5, 90, 2, 0.3, 0.5, 1)]  # other seeds, more graphs, longer streams: the pools regrow
    b = Batch(5)
    try:
        for groups in (first, larger, first):
            graphs = _generate(b, groups)
            b.run()
            for g, key in graphs:
                _check_stream(b, g, key)
            _check_states(b, None, graphs)
            b.clear()
            assert b.graphs() == 0
        # an added graph after clear() as well
        dag, calls = _want(5, 300, 5, 70, 2, 0.3, 0.5, 0)[:2]
        b.add(dag, calls)
        b.run()
        _check_states(b, None, [(0, (5, 300, 5, 70, 2, 0.3, 0.5, 0))])
    finally:
        b.close()


def test_mixing_and_bad_arguments_are_refused():
    from babble_amd.engine import Batch, HgeError
    b = Batch(4)
    try:
        bad = [dict(events=3), dict(graphs=0), dict(fork_p=1.5), dict(cascade_p=-0.5), dict(forkers=-1), dict(k=0),
               dict(op_lag=-1), dict(op_lag=1 << 20)]
        for change in bad:
            with pytest.raises(HgeError) as e:
                b.generate(**dict(dict(events=100, k=4, graphs=2, seed=1), **change))
            assert e.value.code == HGE_ERR_ARG, change
        assert b.graphs() == 0
        dag, calls = _want(4, 100, 4, 1, 0, 0.0, 0.0, 0)[:2]
        b.add(dag, calls)
        with pytest.raises(HgeError) as e:
            b.generate(100, 4, 1, 1)
        assert e.value.code == HGE_ERR_ARG
        with pytest.raises(HgeError) as e:
            b.submissions(0)  # an added graph has no device stream
        assert e.value.code == HGE_ERR_ARG
        b.clear()
        b.generate(100, 4, 1, 1)
        with pytest.raises(HgeError) as e:
            b.add(dag, calls)
        assert e.value.code == HGE_ERR_ARG
        assert b.graphs() == 1
        b.run()
        _check_states(b, None, [(0, (4, 100, 4, 1, 0, 0.0, 0.0, 0))])
    finally:
        b.close()
