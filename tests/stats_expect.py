"""What Batch.stats() (hge_batch_stats) must return for one graph, computed in numpy from
an oracle state straight from the definitions (babble_amd/csrc/hge_stats.h), and the
cache of the streams the CPU and GPU tests of the statistics share (a test helper).

For an accepted event x that the replay ordered:
  dround = rr[x] - round[x]
  icall  = the first call c whose accepted count calls[c] is above x
  ccall  = the call whose batch committed x
  dcall  = ccall - icall,  lag = calls[ccall] - 1 - x,  dts = cts[x] - ts[x]
binned as round: min(dround, bins - 1); call: min(dcall, bins - 1); lag: min(lag // lag_bin,
bins - 1); ts: 0 below ts_lo, else 1 + min((dts - ts_lo) // ts_bin, ts_bins), in exact
(Python) integers.  Only events with x_lo <= x < x_hi count."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

FIELDS = 24
ONE_CALL = 1 << 40


def derive(dag, calls, state):
    """Per accepted event of the stream: dict(E, callE, ordered (mask), dround, icall, ccall,
    dcall, lag, dts); the per-event arrays are defined where `ordered` holds."""
    status = np.asarray(state["status"])
    acc = status >= 0
    E = int(acc.sum())
    ts = np.zeros(E, np.int64)
    ts[status[acc]] = np.asarray(dag["ts"], np.int64)[acc]
    calls = np.asarray(calls, np.int64)
    callE = np.cumsum(acc)[calls - 1].astype(np.int64) if len(calls) else np.zeros(0, np.int64)
    order = np.asarray(state["order"], np.int64)
    counts = np.asarray(state["counts"], np.int64)
    assert len(counts) == len(calls) and int(counts.sum()) == len(order)
    ccall = np.full(E, -1, np.int64)
    ccall[order] = np.repeat(np.arange(len(calls)), counts)
    rr = np.asarray(state["rr"], np.int64)[:E]
    rounds = np.asarray(state["rounds"], np.int64)[:E]
    cts = np.asarray(state["cts"], np.int64)[:E]
    x = np.arange(E, dtype=np.int64)
    ordered = rr >= 0
    assert np.array_equal(ordered, ccall >= 0)
    icall = np.searchsorted(callE, x, side="right")
    lag = np.where(ordered, callE[np.maximum(ccall, 0)] - 1 - x, 0) if len(calls) else np.zeros(E, np.int64)
    return dict(E=E, callE=callE, ordered=ordered, dround=rr - rounds, icall=icall, ccall=ccall,
                dcall=ccall - icall, lag=lag, dts=cts - ts)


def expect(dag, calls, state, spec, path=0):
    """(row int64[24], hist int64[hist_len]) of one graph under `spec` (a StatsSpec or
    anything with its attributes); `path` is field 19 (how the engine replayed it)."""
    d = derive(dag, calls, state)
    E = d["E"]
    x = np.arange(E, dtype=np.int64)
    inr = (x >= spec.x_lo) & (x < spec.x_hi)
    sel = inr & d["ordered"]
    dround, dcall, lag, dts = (d[f][sel] for f in ("dround", "dcall", "lag", "dts"))
    fame = np.asarray(state["fame"])
    R, lcr = int(state["scalars"][0]), int(state["scalars"][1])
    row = np.zeros(FIELDS, np.int64)
    row[0], row[1], row[2] = E, int(inr.sum()), int(sel.sum())
    row[3] = row[1] - row[2]
    row[4], row[5] = R, lcr
    row[6:10] = [(fame[:R] >= 0).sum(), (fame[:R] == 1).sum(), (fame[:R] == 2).sum(), (fame[:R] == 0).sum()]
    if row[2]:
        assert dround.min() >= 1 and dcall.min() >= 0 and lag.min() >= 0
        row[10:16] = [dround.sum(), dround.max(), dcall.sum(), dcall.max(), lag.sum(), lag.max()]
        total = sum(dts.tolist()) & ((1 << 64) - 1)  # wrapping mod 2^64, as a signed value
        row[16] = total - (1 << 64) if total >= 1 << 63 else total
        row[17], row[18] = dts.min(), dts.max()
    row[19] = path
    rb, cb, lb, tb = spec.round_bins, spec.call_bins, spec.lag_bins, spec.ts_bins
    lo, w = int(spec.ts_lo), int(spec.ts_bin)
    tsb = np.array([0 if v < lo else 1 + min((v - lo) // w, tb) for v in dts.tolist()], np.int64)
    hist = np.concatenate([np.bincount(np.minimum(dround, rb - 1), minlength=rb),
                           np.bincount(np.minimum(dcall, cb - 1), minlength=cb),
                           np.bincount(np.minimum(lag // int(spec.lag_bin), lb - 1), minlength=lb),
                           np.bincount(tsb, minlength=tb + 2)]).astype(np.int64)
    assert len(hist) == rb + cb + lb + tb + 2
    return row, hist


_cache = {}


def counter_case(n, events, k, seed, fk=0, fp=0.0, cp=0.0, lag=0):
    """(stream, calls, oracle state) of a counter_gossip stream under schedule(., k): what
    Batch.generate(events, k, 1, seed, fk, fp, cp, lag) holds.  Computed once, shared by
    every test that needs it, and left unchanged."""
    from babble_amd.gossip import counter_gossip, schedule
    from make_mc_digests import oracle_state
    key = (n, events, k, seed, fk, fp, cp, lag)
    if key not in _cache:
        dag = counter_gossip(n, events, seed, fk, fp, cp, lag)
        calls = schedule(len(dag["creator"]), min(k, len(dag["creator"])))
        _cache[key] = (dag, calls, oracle_state(dag, calls))
    return _cache[key]


def repeated_calls(dag, calls, state):
    """Call points whose accepted count equals the previous call's (refused submissions)."""
    callE = derive(dag, calls, state)["callE"]
    return int((callE[1:] == callE[:-1]).sum())


# the streams the issue names: each reaches the case it is there for (tests/test_stats_expect.py)
LONG_ROUNDS = (64, 5000, ONE_CALL, 13)                  # one call: dround up to 5, every dcall 0
K1_REFUSED = (5, 600, 1, 7, 2, 0.05, 0.5, 3)            # K = 1 over refused submissions
K2_REFUSED = (2, 127, 2, 6, 1, 1.0, 1.0, 0)
NOTHING = [(5, 5, 1, 3), (32, 600, 32, 4), (1, 65, 5, 5)]  # nothing ordered
PAST_FOLD = (2, 1200, 7, 22, 1, 0.05, 0.5, 0)           # 297 rounds: past the bulk fold's 256
TS_CASES = [((4, 1200, 1, 31, 0, 0.0, 0.0, 0), "spread"), ((5, 1500, 40, 32, 0, 0.0, 0.0, 3), "two31"),
            ((32, 3000, 32, 33, 10, 0.05, 0.5, 0), "gaps")]
