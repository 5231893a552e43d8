"""A run's consensus-latency statistics reduced on the device (hge_batch_stats,
hge_batch_stats.hip; Batch.stats, babble_amd.sweep): every field of the per-graph rows, the
summed histograms and the per-graph histograms, exactly, against tests/stats_expect.py on
the oracle's state.

The sizes are the pass's boundaries: batches of graphs of different sizes (the per-graph
offsets of the event, call and round pools), streams of N, 65, 127 and 600 events and one
of 3,000 (N = 5 under K = 1: ~3,100 call points, past the 2,048 the kernel stages in LDS)
or 5,000 (N >= 32, where the shorter streams order nothing: 600 events are three rounds),
K = 1 over refused submissions (repeated call points), one call, graphs that order
nothing, x ranges that are empty, inside one 64-event chunk, past the end and at it,
timestamp differences that are negative, outside int32 and binned from INT64_MIN, graphs
replayed call by call (HGB_SERIAL=1, and one of 297 rounds beside bulk graphs: the second
source of an event's commit call), delivery on, and a regrown batch.  N = 2 has no large
graph: 3,000 events there are ~750 rounds, past the bulk fold, which test_mixed_batch
covers with the 297-round one."""
import itertools

import numpy as np
import pytest

import stats_expect as se
import ts_shapes

pytestmark = pytest.mark.gpu

HGE_ERR_ARG = -8
ONE_CALL = se.ONE_CALL
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _spec(**kw):
    from babble_amd.engine import StatsSpec
    return StatsSpec(**kw)


def _clamping(cases):
    """every histogram clamps: two round bins, eight call bins, four lag bins of 100 events,
    three ts bins of 1 us from 1 us above the smallest dts of the batch"""
    dmin = min(int(d["dts"][d["ordered"]].min()) for d in (se.derive(*c) for c in cases) if d["ordered"].any())
    return _spec(round_bins=2, call_bins=8, lag_bins=4, lag_bin=100, ts_bins=3, ts_bin=1000, ts_lo=dmin + 1000)


def _wide():
    return _spec(round_bins=256, call_bins=256, lag_bins=256, lag_bin=64, ts_bins=256, ts_bin=5000, ts_lo=0)


def _corners(n):
    """(forkers, fork_p, cascade_p, op_lag): none, config 5's shape, every step forking
    and every twin cascading, with and without lag."""
    some = max(1, n // 3)
    return [(0, 0.0, 0.0, 0), (some, 0.05, 0.5, 3), (n, 1.0, 1.0, 0), (n, 1.0, 0.5, 3), (some, 1.0, 0.0, 0)]


def _groups(n, large=True):
    """One generate() call each: (events, k, graphs, seed, forkers, fork_p, cascade_p, op_lag);
    every events x K pair, the batch sizes 1, 3, 5 and the corners going round."""
    out, corners = [], _corners(n)
    sizes = sorted({e for e in (n, 65, 127, 600) if e >= n})
    for j, (events, k) in enumerate(itertools.product(sizes, (1, n, ONE_CALL))):
        out.append((events, k, (1, 3, 5)[(j + j // 3) % 3], 7000 * n + 10 * j) + corners[j % 5])
    if large and n > 2:
        out.append((3000, 1, 1, 7000 * n + 900) + corners[1] if n == 5 else (5000, n, 1, 7000 * n + 900) + corners[1])
    return out


def _generate(b, groups):
    """The groups appended; [(graph, its se.counter_case key)]"""
    graphs = []
    for events, k, count, seed, fk, fp, cp, lag in groups:
        g0 = b.generate(events, k, count, seed, fk, fp, cp, lag)
        graphs += [(g0 + i, (b.n, events, k, seed + i, fk, fp, cp, lag)) for i in range(count)]
    assert b.graphs() == len(graphs)
    return graphs


def _want(cases, spec, paths=None):
    """(rows [G][24], hist [hist_len], per-graph hists [G][hist_len]) of the graphs whose
    (stream, calls, state) are `cases`"""
    rows, hists = [], []
    for i, (dag, calls, st) in enumerate(cases):
        r, h = se.expect(dag, calls, st, spec, 0 if paths is None else paths[i])
        rows.append(r)
        hists.append(h)
    return np.array(rows), np.sum(hists, axis=0), np.array(hists)


def _rows(st):
    return st["graphs"].view(np.int64).reshape(-1, se.FIELDS)


def _per_graph(st):
    return np.concatenate([st["per_graph"][f] for f in ("round", "call", "lag", "ts")], axis=1)


def _check(b, cases, spec, paths=None, what=""):
    from babble_amd.engine import STATS_FIELDS
    rows, hist, hists = _want(cases, spec, paths)
    st = b.stats(spec, per_graph_hist=True)
    got = _rows(st)
    assert got.shape == rows.shape, what
    for g, f in zip(*np.nonzero(got != rows)):
        raise AssertionError(f"{what} graph {g} field {STATS_FIELDS[f]}: {got[g, f]}, want {rows[g, f]}")
    assert np.array_equal(_per_graph(st), hists), f"{what}: per-graph histograms"
    assert np.array_equal(st["hist"], hist), f"{what}: summed histograms"
    assert np.array_equal(np.concatenate([st[f] for f in ("round", "call", "lag", "ts")]), hist), what
    assert st["hist"].dtype == np.int64 and len(st["hist"]) == spec.hist_len()
    lean = b.stats(spec)  # without the per-graph histograms: the same rows and totals
    assert lean["per_graph"] is None and np.array_equal(_rows(lean), rows) and np.array_equal(lean["hist"], hist)
    return st


def _cases(graphs):
    return [se.counter_case(*key) for _, key in graphs]


@pytest.mark.parametrize("n", [2, 5, 32, 33, 64])
def test_generated_batches_of_mixed_sizes(n):
    from babble_amd.engine import Batch
    b = Batch(n)
    try:
        graphs = _generate(b, _groups(n))
        cases = _cases(graphs)
        b.run()
        assert b.fallbacks() == 0
        st = _check(b, cases, _clamping(cases), what="clamping")
        # the clamps are reached: the last bin of each histogram holds events
        assert st["round"][-1] > 0 and st["call"][-1] > 0 and st["lag"][-1] > 0 and st["ts"][0] > 0 and st["ts"][-1] > 0
        _check(b, cases, _wide(), what="wide")
        if n == 5:  # the large graph's call points pass the kernel's LDS table
            assert max(len(c[1]) for c in cases) > 2048
    finally:
        b.close()


def test_x_ranges():
    from babble_amd.engine import Batch
    b = Batch(5)
    try:
        graphs = _generate(b, _groups(5, large=False))
        cases = _cases(graphs)
        b.run()
        E = [se.derive(*c)["E"] for c in cases]
        assert 600 in E and min(E) == 5
        for lo, hi in [(10, 10), (0, 0), (70, 100), (64, 128), (63, 65), (500, 10 ** 9), (0, 600), (600, INT64_MAX),
                       (600, 600), (599, 600), (601, INT64_MAX), (INT64_MAX, INT64_MAX)]:
            spec = _spec(x_lo=lo, x_hi=hi, lag_bin=5)
            st = _check(b, cases, spec, what=f"x in [{lo}, {hi})")
            if lo >= 600 or lo == hi:
                assert not st["hist"].any() and not st["graphs"]["in_range"].any()
    finally:
        b.close()


@pytest.mark.parametrize("case,kind", se.TS_CASES, ids=lambda v: v if isinstance(v, str) else str(v[0]))
def test_added_graphs_on_timestamp_shapes(case, kind):
    """Negative dts (spread), dts = +-2^31 (two31), dts up to 3.0e9 (gaps); ts_lo at
    INT64_MIN, at +-B (the timestamps' own scale, 1.7e18) and where the values lie."""
    from babble_amd.engine import Batch
    dag, calls, state, _ = ts_shapes.oracle_case(case, kind)
    small = se.counter_case(case[0], 127, 3, 5)  # a second graph: the first one's offsets are not 0 everywhere
    b = Batch(case[0])
    try:
        b.add(small[0], small[1])
        b.add(dag, calls)
        b.run()
        assert b.fallbacks() == 0
        cases = [small, (dag, calls, state)]
        B = ts_shapes.B
        for kw in [dict(ts_lo=INT64_MIN, ts_bin=1 << 62, ts_bins=4), dict(ts_lo=INT64_MIN, ts_bin=1, ts_bins=256),
                   dict(ts_lo=INT64_MIN, ts_bin=INT64_MAX, ts_bins=1), dict(ts_lo=-B, ts_bin=B >> 7, ts_bins=256),
                   dict(ts_lo=B, ts_bin=1, ts_bins=3), dict(ts_lo=INT64_MAX, ts_bin=1, ts_bins=1),
                   dict(ts_lo=-(1 << 31), ts_bin=1 << 24, ts_bins=256), dict(ts_lo=-(1 << 31) + 1, ts_bin=1 << 31, ts_bins=2),
                   dict(ts_lo=0, ts_bin=30_000_000, ts_bins=100)]:
            st = _check(b, cases, _spec(**kw), what=f"{kind} {kw}")
            assert st["ts"].sum() == st["graphs"]["ordered"].sum() > 0
        row = _rows(b.stats())[1]
        if kind == "spread":
            assert row[17] < 0
        if kind == "two31":
            assert (row[17], row[18]) == (-(1 << 31), 1 << 31)
        if kind == "gaps":
            assert row[18] >= 3_000_000_000
    finally:
        b.close()


@pytest.mark.parametrize("n", [5, 33])
def test_serial_replay_has_the_bulk_runs_statistics(n, monkeypatch):
    """HGB_SERIAL=1: every graph through kb_consensus, whose per-event commit call the
    pass then reads.  Field 19 = 1 for all; everything else is the bulk run's result."""
    from babble_amd.engine import Batch
    groups = _groups(n, large=n > 5)  # (N = 5's large graph is ~3,100 calls of kb_consensus)
    bulk = Batch(n)
    try:
        graphs = _generate(bulk, groups)
        cases = _cases(graphs)
        specs = (("clamping", _clamping(cases)), ("wide", _wide()))
        bulk.run()
        assert bulk.fallbacks() == 0
        ref = {name: bulk.stats(spec, per_graph_hist=True) for name, spec in specs}
        assert ref["wide"]["graphs"]["ordered"].sum() > 1000
    finally:
        bulk.close()
    monkeypatch.setenv("HGB_SERIAL", "1")
    b = Batch(n)
    try:
        _generate(b, groups)
        b.run()
        assert b.fallbacks() == len(graphs)
        for name, spec in specs:
            st = _check(b, cases, spec, paths=[1] * len(graphs), what=f"serial {name}")
            got, want = _rows(st).copy(), _rows(ref[name]).copy()
            assert (got[:, 19] == 1).all() and (want[:, 19] == 0).all()
            got[:, 19] = 0
            assert np.array_equal(got, want)
            assert np.array_equal(_per_graph(st), _per_graph(ref[name])) and np.array_equal(st["hist"], ref[name]["hist"])
    finally:
        b.close()


# generate() groups: (events, k, graphs, seed, forkers, fork_p, cascade_p, op_lag)
MIXED = [(300, 2, 1, 21, 1, 0.3, 1.0, 2), se.PAST_FOLD[1:3] + (1,) + se.PAST_FOLD[3:], (127, 1, 1, 24, 2, 1.0, 1.0, 0)]


def test_mixed_batch():
    """N = 2: the 297-round graph (past the bulk fold's 256, 1,189 events ordered) between
    two graphs the bulk path orders: the pass takes each graph's commit calls from its own
    source."""
    from babble_amd.engine import Batch
    b = Batch(2)
    try:
        graphs = _generate(b, MIXED)
        cases = _cases(graphs)
        assert cases[1][2]["scalars"][0] == 297 and len(cases[1][2]["order"]) == 1189
        b.run()
        assert b.fallbacks() == 1
        for spec in (_clamping(cases), _wide(), _spec(x_lo=100, x_hi=1000)):
            st = _check(b, cases, spec, paths=[0, 1, 0], what="mixed")
        assert st["graphs"]["path"].tolist() == [0, 1, 0]
        undelivered = b.stats(_wide(), per_graph_hist=True)
        b.deliver(order=True, received=True)  # kb_consensus' delivering instance stores the table too
        b.run()
        assert b.fallbacks() == 1 and b.delivered() == 1
        st = _check(b, cases, _wide(), paths=[0, 1, 0], what="mixed, delivered")
        assert _rows(st).tobytes() == _rows(undelivered).tobytes()
    finally:
        b.close()


@pytest.mark.parametrize("n,no_pin", [(5, False), (32, False), (5, True)])
def test_delivery_leaves_the_statistics_unchanged(n, no_pin, monkeypatch):
    from babble_amd.engine import Batch
    if no_pin:
        monkeypatch.setenv("HGB_TEST_NO_PIN", "1")
    b = Batch(n)
    try:
        graphs = _generate(b, _groups(n))
        cases = _cases(graphs)
        b.run()
        plain = b.stats(_wide(), per_graph_hist=True)
        b.deliver(order=True, received=True)
        b.run()
        assert b.delivered() == (2 if no_pin else 1)
        for spec in (_clamping(cases), _wide()):
            st = _check(b, cases, spec, what="delivered")
        for f in ("graphs", "hist"):
            assert st[f].tobytes() == plain[f].tobytes()
        assert _per_graph(st).tobytes() == _per_graph(plain).tobytes()
    finally:
        b.close()


def test_lifecycle():
    from babble_amd.engine import Batch, HgeError

    def refused(b, spec=None):
        with pytest.raises(HgeError) as e:
            b.stats(spec)
        assert e.value.code == HGE_ERR_ARG

    first = [(300, 5, 3, 70, 2, 0.3, 0.5, 0)]
    larger = [(900, 1, 5, 90, 2, 0.3, 0.5, 1), (65, ONE_CALL, 2, 97, 0, 0.0, 0.0, 0)]  # the pools regrow
    b, fresh = Batch(5), None
    try:
        refused(b)  # nothing run
        assert b.run() == 0  # no graphs: zeros
        st = b.stats(per_graph_hist=True)
        assert len(st["graphs"]) == 0 and not st["hist"].any() and st["per_graph"]["round"].shape == (0, 16)
        graphs = _generate(b, first)
        refused(b)  # generated, not run
        b.stage()
        refused(b)
        b.run()
        refused(b, _spec(round_bins=0))  # a bad spec
        refused(b, _spec(x_lo=3, x_hi=2))
        cases = _cases(graphs)
        one = _check(b, cases, _clamping(cases), what="first")
        two = b.stats(_clamping(cases), per_graph_hist=True)  # twice: the same bytes
        for f in ("graphs", "hist"):
            assert one[f].tobytes() == two[f].tobytes()
        assert _per_graph(one).tobytes() == _per_graph(two).tobytes()
        _check(b, cases, _wide(), what="another hist_len on the same run")
        _check(b, cases, _clamping(cases), what="and back")
        b.stage()  # staged since the run
        refused(b)
        b.run()
        _check(b, cases, _clamping(cases), what="second run")
        b.clear()
        refused(b)
        graphs = _generate(b, larger)
        refused(b)
        b.run()
        cases = _cases(graphs)
        st = _check(b, cases, _wide(), what="regrown")
        fresh = Batch(5)
        _generate(fresh, larger)
        fresh.run()
        other = fresh.stats(_wide(), per_graph_hist=True)
        for f in ("graphs", "hist"):
            assert st[f].tobytes() == other[f].tobytes()
        assert _per_graph(st).tobytes() == _per_graph(other).tobytes()
        b.clear()
        dag, calls, _ = cases[0]
        b.add(dag, calls)  # an added graph after clear()
        refused(b)
        b.run()
        _check(b, cases[:1], _clamping(cases), what="added")
        b.add(dag, calls)
        refused(b)
    finally:
        b.close()
        if fresh is not None:
            fresh.close()


def test_sweep():
    from babble_amd.engine import STATS_ROW_DTYPE
    from babble_amd.sweep import quantile, sweep
    n, events, k, seed, corner = 5, 300, 5, 4100, (2, 0.3, 0.5, 1)
    spec = _spec(lag_bin=5, ts_bin=1000)
    out = sweep(n, events, k, 3, 2, seed, *corner, spec=spec)
    cases = [se.counter_case(n, events, k, seed + i, *corner) for i in range(6)]
    rows, hist, _ = _want(cases, spec)
    assert out["graphs"].dtype == STATS_ROW_DTYPE
    assert np.array_equal(out["graphs"].view(np.int64).reshape(-1, se.FIELDS), rows)
    assert np.array_equal(out["hist"], hist)
    assert np.array_equal(np.concatenate([out[f] for f in ("round", "call", "lag", "ts")]), hist)
    assert out["ordered"] == rows[:, 2].sum() > 0 and out["fallbacks"] == 0
    # the median dround's bin against the events themselves
    dround = np.concatenate([se.derive(*c)["dround"][se.derive(*c)["ordered"]] for c in cases])
    lo, hi = quantile(out["round"], 0.5, 0, 1)
    assert lo <= np.sort(dround)[(len(dround) - 1) // 2] < hi
    assert quantile(np.zeros(4, np.int64), 0.5, 0, 1) is None
