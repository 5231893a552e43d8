"""FindOrder's commit records of a seeded stream, from a live oracle (a test helper).

FindOrder hands its caller events with their roundReceived and consensusTimestamp
(hashgraph.go:723-760); the timestamp is the source event's own Body.Timestamp
(MedianTimestamp, hashgraph.go:762-770).  expected() computes, for log position q:

  ids[q]  order[q]
  rr[q], cts[q]   the oracle's event_received() at that id
  src[q]  among o.oldest_self_ancestor_to_see(w, x), w over o.round_witnesses(rr) with
          o.round_fame(rr, w) == 1 and o.see(w, x), the one of lowest creator whose own
          timestamp equals cts (the engine's documented choice where several share the
          instant: the reference leaves it to a sort over a map-ordered list)

and two flags per record that say what a stream proves about a kernel:

  multi[q]  more than one candidate at the median instant
  wrong[q]  the middle of the candidates sorted by (timestamp, creator) is another event
            than src[q]: a kernel with that tie rule fails on the record

Ids are engine ids: a forked stream's submissions map to them through the status array.
Everything is computed once per case, shared by the tests and left unchanged."""
import numpy as np

from babble_amd.gossip import random_gossip, schedule
from oracle.oracle import replay as oracle_replay

from ts_shapes import shape

# name -> n, events, K, seed, forkers, fork_p, cascade_p, op_lag, timestamp shape, oracle scale mode
CASES = {
    "A": (4, 1200, 1, 31, 0, 0.0, 0.0, 0, "ties", False),
    "B": (5, 1500, 40, 32, 0, 0.0, 0.0, 3, "two31", False),
    "C": (16, 3000, 16, 61, 0, 0.0, 0.0, 0, "ties", False),
    "D": (32, 3000, 32, 33, 10, 0.05, 0.5, 0, "ties", False),
    "E": (33, 2500, 50, 36, 0, 0.0, 0.0, 3, "ties", False),
    "F": (64, 5000, 64, 37, 0, 0.0, 0.0, 0, "ties", False),
    "F31": (64, 5000, 64, 37, 0, 0.0, 0.0, 0, "two31", False),
    "G": (132, 9000, 132, 41, 0, 0.0, 0.0, 0, "ties", True),
    "H": (256, 14000, 256, 43, 0, 0.0, 0.0, 0, "two31", True),
    # case E's gossip among 64 participants, a second, shorter stream for an engine that ran F.
    # E's own 2,500 events order nothing among 64 (nor do 3,000), which would show nothing: 4,500
    # order 1,759 over two rounds received
    "E64": (64, 4500, 50, 36, 0, 0.0, 0.0, 3, "ties", False),
    # int32 chain positions under HGE_CHAIN_LIMIT=40 (the longest chain is 69)
    "I": (36, 2000, 36, 41, 0, 0.0, 0.0, 0, "spread", False),
}

_streams, _expected = {}, {}


def stream(name):
    """(dag, calls) of a case."""
    if name not in _streams:
        cn, E, k, seed, fk, fp, cp, lag, kind, _ = CASES[name]
        dag = shape(random_gossip(cn, E, seed=seed, forkers=fk, fork_p=fp, cascade_p=cp, op_lag=lag), kind, seed)
        _streams[name] = (dag, schedule(len(dag["creator"]), k))
    return _streams[name]


def records_of(dag, calls, scale=False):
    """The expected records of a stream: dict(status, counts, ids, rr, cts, src, multi, wrong)."""
    o, status, order, counts = oracle_replay(dag, calls, scale=scale)
    try:
        acc = status >= 0
        E = int(acc.sum())
        ts = np.zeros(E, np.int64)
        ts[status[acc]] = np.asarray(dag["ts"], np.int64)[acc]
        creator = np.zeros(E, np.int64)
        creator[status[acc]] = np.asarray(dag["creator"], np.int64)[acc]
        orr, octs = o.event_received()
        ids = np.asarray(order, np.int32)
        rr = orr[ids].astype(np.int32)
        cts = octs[ids].astype(np.int64)
        m = len(ids)
        src = np.full(m, -1, np.int32)
        multi = np.zeros(m, bool)
        wrong = np.zeros(m, bool)
        famous = {}
        for q in range(m):
            x, r = int(ids[q]), int(rr[q])
            if r not in famous:
                famous[r] = [w for w in o.round_witnesses(r) if o.round_fame(r, w) == 1]
            cands = [o.oldest_self_ancestor_to_see(w, x) for w in famous[r] if o.see(w, x)]
            assert cands and None not in cands, (q, x, r)
            at = sorted((int(creator[c]), c) for c in cands if ts[c] == cts[q])
            assert at, (q, x, r)  # the median is one of the candidates' timestamps
            src[q] = at[0][1]
            multi[q] = len(at) > 1
            mid = sorted((int(ts[c]), int(creator[c]), c) for c in cands)[len(cands) // 2]
            assert mid[0] == cts[q], (q, x, r)  # MedianTimestamp: events[len / 2]
            wrong[q] = mid[2] != src[q]
        return dict(status=status, counts=np.asarray(counts, np.int64), ids=ids, rr=rr, cts=cts, src=src,
                    multi=multi, wrong=wrong)
    finally:
        o.close()


def expected(name):
    if name not in _expected:
        dag, calls = stream(name)
        _expected[name] = records_of(dag, calls, scale=CASES[name][9])
    return _expected[name]


def assert_records(got, exp, lo=0, hi=None, sources=True):
    """got (Engine.commit_records' dict) equals the slice [lo, hi) of the expected records."""
    hi = len(exp["ids"]) if hi is None else hi
    for k in ("ids", "rr", "cts"):
        np.testing.assert_array_equal(got[k], exp[k][lo:hi], err_msg=k)
    if sources:
        np.testing.assert_array_equal(got["src"], exp["src"][lo:hi], err_msg="src")
    else:
        assert got["src"] is None
