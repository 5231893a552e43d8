"""A fresh bulk replay at uint16 positions (N > 128, N % 4 == 0) takes its median from
the FD rows (k_median_rows after k_fd_rows16) and never writes the FD timestamp table;
the replay ends with that table's rows for the still-undetermined events alone
(fdtd_tail), which a later online call's k_median_wave reads.  N = 132 is the smallest
width of the path: 33 four-column lanes, a partial 64-column tile, int32 threshold rows.
Everything against the oracle (MedianTimestamp, hashgraph.go:762-770)."""
import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule
from parity import compare_state, oracle_reach, oracle_run, with_creators
from ts_shapes import shape

pytestmark = pytest.mark.gpu

N, E, K, SEED = 132, 9240, 132, 7
E_REPLAY = 7920  # the first 60 calls
MIN_ORDERED = 2000

ROWS = "k_median_rows"
WAVE = "k_median_wave"
FD_ROWS = "k_fd_rows16"
TAIL = "fdtd_tail"
ENSURE = "fdtd_ensure"


def _stream(kind):
    dag = random_gossip(N, E, seed=SEED)
    ids = np.arange(E, dtype=np.int64)
    if kind == "wide":  # offsets outside int32: the exact 64-bit select
        dag["ts"] = dag["ts"] + (ids // 500) * 3_000_000_000
    elif kind == "spread":  # test_gpu_wide.py::test_median_select_extremes' two recipes
        rng = np.random.default_rng(N)
        dag["ts"] = 1_700_000_000_000_000_000 + rng.integers(-(1 << 30) + 1, 1 << 30, E, dtype=np.int64)
    elif kind == "ties":
        dag["ts"] = 1_700_000_000_000_000_000 + (ids // 97) * 1000
    elif kind in ("two31m", "two31"):  # every offset 0 or +-(2^31 - 1), the last of the int32 rows; or +-2^31
        dag = shape(dag, kind, SEED)
    else:
        assert kind == "plain"
    return dag


_refs = {}


def _reference(kind):
    """(stream, calls, oracle, status, order, counts), computed once per kind."""
    if kind not in _refs:
        dag = _stream(kind)
        calls = schedule(E, K)
        o, ost, oorder, ocounts = oracle_run(dag, calls)
        assert len(oorder) >= MIN_ORDERED, len(oorder)
        if kind in ("two31m", "two31"):  # the oracle's own run shows events on / past the int32 edge
            r = oracle_reach(dag, o, ost, oorder, ocounts)
            assert (r["edge_i32"] > 0 and r["out_i32"] == 0) if kind == "two31m" else r["out_i32"] > 0, r
        _refs[kind] = (dag, calls, o, ost, oorder, ocounts)
    return _refs[kind]


def _ran(stats, prefix):
    return sum(cnt for name, (_, cnt) in stats.items() if name.startswith(prefix))


def _check_replay(eng, kind):
    dag, calls, o, ost, oorder, ocounts = _reference(kind)
    st, order, counts = eng.replay(dag, calls)
    with_creators(eng, dag, st)
    np.testing.assert_array_equal(st, ost, err_msg="admission status differs")
    assert len(order) == len(oorder) >= MIN_ORDERED
    np.testing.assert_array_equal(order, oorder, err_msg="consensus order differs")
    np.testing.assert_array_equal(counts, ocounts, err_msg="per-call batch sizes differ")
    compare_state(eng, o)


@pytest.mark.parametrize("kind", ["plain", "wide", "spread", "ties", "two31m", "two31"])
def test_median_rows_parity(kind):
    """Full state against the oracle at N = 132: the plain stream; timestamps that grow by
    3 s per 500 events (offsets outside int32: the wide rows of the uint16 path);
    timestamps spread over +-2^30 ns; long runs of equal timestamps; two timestamps
    2^31 - 1 ns apart (offsets of +-INT32_MAX, the last that stay int32 rows, their image
    the select's filler) and 2^31 ns apart (the first that must not)."""
    from babble_amd.engine import Engine
    eng = Engine(N, E)
    try:
        eng.set_profiling(True)
        _check_replay(eng, kind)
        ks = eng.kernel_stats()
        assert _ran(ks, ROWS) == 1 and _ran(ks, FD_ROWS) == 1 and _ran(ks, WAVE) == 0, ks
    finally:
        eng.close()


def test_replay_then_online_calls():
    """60 calls replayed in bulk, then 10 online calls: the replay takes the new kernels
    and leaves valid timestamp rows for the undetermined events (its tail pass, never the
    full-table pass); the online calls take k_median_wave over them."""
    from babble_amd.engine import Engine, events_array
    dag, calls, o, ost, oorder, ocounts = _reference("plain")
    ev = events_array(dag)
    nrep = int(np.searchsorted(calls, E_REPLAY)) + 1
    assert calls[nrep - 1] == E_REPLAY and len(calls) - nrep == 10
    eng = Engine(N, E)
    try:
        eng.set_profiling(True)
        st, order, counts = eng.replay(ev[:E_REPLAY], calls[:nrep])
        np.testing.assert_array_equal(st, ost[:E_REPLAY])
        ks = eng.kernel_stats()
        assert _ran(ks, ROWS) == 1 and _ran(ks, FD_ROWS) == 1 and _ran(ks, TAIL) == 1, ks
        assert _ran(ks, WAVE) == 0 and _ran(ks, ENSURE) == 0, ks
        eng.set_profiling(True)  # (resets the statistics)
        order, counts = list(order), list(counts)
        nxt = E_REPLAY
        for c in calls[nrep:]:
            eng.insert_events(ev[nxt:c].copy())
            got = eng.run_consensus()
            order.extend(got)
            counts.append(len(got))
            nxt = int(c)
        ks = eng.kernel_stats()
        assert 1 <= _ran(ks, WAVE) <= 10 and _ran(ks, ROWS) == 0, ks
        assert _ran(ks, ENSURE) == 0 and _ran(ks, TAIL) == 0 and _ran(ks, FD_ROWS) == 0, ks
        assert len(order) == len(oorder) >= MIN_ORDERED
        np.testing.assert_array_equal(np.asarray(order), oorder, err_msg="consensus order differs")
        np.testing.assert_array_equal(np.asarray(counts), ocounts, err_msg="per-call batch sizes differ")
        with_creators(eng, dag, ost)
        compare_state(eng, o)
    finally:
        eng.close()


def test_fallback_hook_takes_the_full_timestamp_pass(monkeypatch):
    """HGE_TEST_MEDIAN_ROWS_FALLBACK=1: the coordinate step skips the timestamps, the
    median takes k_median_wave, so ensure_fdtd() writes the whole table first.  Same result."""
    from babble_amd.engine import Engine
    monkeypatch.setenv("HGE_TEST_MEDIAN_ROWS_FALLBACK", "1")
    eng = Engine(N, E)
    try:
        eng.set_profiling(True)
        _check_replay(eng, "plain")
        ks = eng.kernel_stats()
        assert _ran(ks, FD_ROWS) == 1 and _ran(ks, WAVE) == 1 and _ran(ks, ENSURE) == 1, ks
        assert _ran(ks, ROWS) == 0 and _ran(ks, TAIL) == 0, ks
    finally:
        eng.close()


def test_repeated_runs_of_a_staged_stream():
    """run() three times over the staged stream: the same state each time (the oracle's
    order), the new kernels in every replay."""
    from babble_amd.engine import Engine, events_array
    dag, calls, o, ost, oorder, ocounts = _reference("plain")
    eng = Engine(N, E)
    try:
        eng.prepare(events_array(dag), calls)
        first = None
        for _ in range(3):
            eng.set_profiling(True)
            eng.run()
            ks = eng.kernel_stats()
            assert _ran(ks, ROWS) == 1 and _ran(ks, FD_ROWS) == 1 and _ran(ks, TAIL) == 1, ks
            assert _ran(ks, WAVE) == 0 and _ran(ks, ENSURE) == 0, ks
            _, order, counts = eng.fetch()
            state = (order, counts, eng.event_rounds(), eng.event_received(), eng.undetermined())
            if first is None:
                first = state
                assert len(order) >= MIN_ORDERED
                np.testing.assert_array_equal(order, oorder)
                np.testing.assert_array_equal(counts, ocounts)
            for x, y in zip(first, state):
                np.testing.assert_array_equal(x, y)
    finally:
        eng.close()
