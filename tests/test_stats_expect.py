"""tests/stats_expect.py on the CPU oracle: the expectation is consistent with the oracle's
own scalars, and every stream the statistics tests use reaches the case it is there for
(asserted, so that a changed generator cannot silently empty a case)."""
import types

import numpy as np
import pytest

import stats_expect as se
import ts_shapes

SPEC = types.SimpleNamespace(round_bins=16, call_bins=64, lag_bins=64, ts_bins=64, lag_bin=16, ts_bin=10_000,
                             ts_lo=0, x_lo=0, x_hi=(1 << 63) - 1)


def _consistent(dag, calls, st):
    row, hist = se.expect(dag, calls, st, SPEC)
    a, b, c = 16, 80, 144
    for h in (hist[:a], hist[a:b], hist[b:c], hist[c:]):
        assert int(h.sum()) == row[2]
    assert row[0] == int((np.asarray(st["status"]) >= 0).sum())
    assert row[2] == len(st["order"])
    assert row[4] == st["scalars"][0] and row[5] == st["scalars"][1]
    assert row[1] == row[0] and row[3] == row[1] - row[2]
    assert row[6] == row[7] + row[8] + row[9]
    return row, hist


def test_one_call_reaches_five_rounds():
    dag, calls, st = se.counter_case(*se.LONG_ROUNDS)
    _consistent(dag, calls, st)
    d = se.derive(dag, calls, st)
    assert len(calls) == 1 and d["dround"][d["ordered"]].max() == 5
    assert not d["dcall"][d["ordered"]].any()


def test_k1_over_refused_submissions():
    dag, calls, st = se.counter_case(*se.K1_REFUSED)
    _consistent(dag, calls, st)
    d = se.derive(dag, calls, st)
    o = d["ordered"]
    assert se.repeated_calls(dag, calls, st) == 21
    assert set(d["dround"][o].tolist()) == {1, 2}
    assert (d["dcall"][o].min(), d["dcall"][o].max()) == (67, 151)


def test_k2_over_refused_submissions():
    dag, calls, st = se.counter_case(*se.K2_REFUSED)
    _consistent(dag, calls, st)
    assert se.repeated_calls(dag, calls, st) == 49


@pytest.mark.parametrize("case", se.NOTHING, ids=str)
def test_nothing_ordered(case):
    dag, calls, st = se.counter_case(*case)
    row, hist = _consistent(dag, calls, st)
    assert row[2] == 0 and row[3] == row[1] == row[0] > 0
    assert not row[10:19].any() and not hist.any()


@pytest.mark.parametrize("case,kind", se.TS_CASES, ids=lambda v: v if isinstance(v, str) else str(v[0]))
def test_timestamp_shapes(case, kind):
    dag, calls, st, _ = ts_shapes.oracle_case(case, kind)
    row, _ = _consistent(dag, calls, st)
    d = se.derive(dag, calls, st)
    dts = d["dts"][d["ordered"]]
    if kind == "spread":
        assert int((dts < 0).sum()) == 314
    if kind == "two31":
        assert (dts.min(), dts.max()) == (-(1 << 31), 1 << 31)
    if kind == "gaps":
        assert 3_000_000_000 <= dts.max() < 3_100_000_000
    assert (row[17], row[18]) == (dts.min(), dts.max())


def test_the_graph_past_the_bulk_fold_orders_events():
    dag, calls, st = se.counter_case(*se.PAST_FOLD)
    row, _ = _consistent(dag, calls, st)
    assert row[4] == 297 and row[2] == 1189


def test_x_range_and_clamps():
    dag, calls, st = se.counter_case(*se.K1_REFUSED)
    full, _ = se.expect(dag, calls, st, SPEC)
    d = se.derive(dag, calls, st)
    dts = np.sort(d["dts"][100:164][d["ordered"][100:164]])
    assert dts[0] < dts[-1]
    lo = int(dts[len(dts) // 2]) if dts[len(dts) // 2] > dts[0] else int(dts[-1])  # above the smallest dts
    cut = types.SimpleNamespace(**dict(vars(SPEC), x_lo=100, x_hi=164, round_bins=2, call_bins=8, lag_bins=4,
                                       lag_bin=100, ts_bins=3, ts_bin=1, ts_lo=lo))
    row, hist = se.expect(dag, calls, st, cut)
    assert row[0] == full[0] and row[1] == 64 and 0 < row[2] <= 64
    assert len(hist) == 2 + 8 + 4 + 5 and hist[9] == row[2]  # every dcall >= 67: the last call bin
    assert hist[14] > 0 and hist[15] > 0  # dts below ts_lo, and at it
