"""Timestamp (and signature) shapes of real clocks for the seeded streams, and what an
oracle run over such a stream reaches in the median and sort kernels (a test helper).

random_gossip's timestamps are TS_BASE + 1000 * submission and its S is uniform:
strictly increasing clocks 1 us apart and signatures that differ in their first 64
bits.  Real events carry each node's own clock: skewed, out of order, tied, seconds
apart.  shape() rewrites a stream's ts (and S for `ties`) by submission position, over
the whole stream (fork twins and cascade records included):

  gaps     3 s more every 500 submissions: median offsets ts(w) - ts(x) outside int32
  spread   uniform over +-2^30 ns: out of order, offsets up to +-(2^31 - 2), call
           buckets whose consensus timestamps span 2^28 ns or more
  ties     97 submissions per timestamp; S's first limb equal everywhere, limbs 1 and 2
           equal on every second submission: keys equal in (rr, cts, limb 0), half of
           them down to limb 3 (S stays distinct: its last limb is random)
  two28m, two28, two31m, two31
           two timestamps D apart, D = 2^28 - 1, 2^28, 2^31 - 1, 2^31: every median
           offset and every bucket's timestamp span is 0 or exactly D, the last value
           that packs / fits int32 and the first that does not

reach() counts, from an oracle state, the events and call buckets that must have taken
those branches.  oracle_case() is the cache of (stream, calls, oracle state, reach) that
the CPU test of the shapes and the GPU tests share."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

B = 1_700_000_000_000_000_000
INT32_MAX = (1 << 31) - 1
SPAN_PACKED = 1 << 28  # kb_sort packs a bucket's timestamps while their span is below this
TWO = {"two28m": (1 << 28) - 1, "two28": 1 << 28, "two31m": (1 << 31) - 1, "two31": 1 << 31}
KINDS = ("gaps", "spread", "ties") + tuple(TWO)

# kb_sort's size classes: one wave or workgroup in LDS, a workgroup in LDS, in HBM
CLASSES = (("to1024", 2, 1024), ("to4096", 1025, 4096), ("past4096", 4097, 1 << 62))

# n, events, k, seed, forkers, fork_p, cascade_p, op_lag -> the size classes its buckets fill
CASES = {
    (4, 1200, 1, 31, 0, 0.0, 0.0, 0): ("to1024",),         # many small buckets, three over two rounds
    (5, 1500, 40, 32, 0, 0.0, 0.0, 3): ("to1024",),        # odd N
    (32, 3000, 32, 33, 10, 0.05, 0.5, 0): ("to1024",),     # rejected submissions
    (32, 3000, 700, 7, 0, 0.0, 0.0, 0): ("to1024", "to4096"),
    (32, 7000, 7000, 35, 0, 0.0, 0.0, 0): ("past4096",),   # one call
    (33, 2500, 50, 36, 0, 0.0, 0.0, 3): ("to1024",),       # a partial row of the 64-wide template
    (64, 5000, 64, 37, 0, 0.0, 0.0, 0): ("to1024", "to4096"),   # the widest
    (64, 5000, 1500, 38, 0, 0.0, 0.0, 0): ("to1024", "to4096"),
}
WIDTHS = sorted({c[0] for c in CASES})


def shape(dag, kind, seed):
    """A copy of the stream with the timestamps (and S for `ties`) of `kind`."""
    m = len(dag["creator"])
    i = np.arange(m, dtype=np.int64)
    rng = np.random.default_rng(1000 + seed)
    out = dict(dag)
    if kind == "gaps":
        out["ts"] = dag["ts"] + (i // 500) * 3_000_000_000
    elif kind == "spread":
        out["ts"] = B + rng.integers(-(1 << 30) + 1, 1 << 30, m, dtype=np.int64)
    elif kind == "ties":
        out["ts"] = B + (i // 97) * 1000
        S = dag["S"].copy()
        S[:, :8] = 0x5A
        S[::2, 8:24] = 0x11
        assert len(np.unique(S, axis=0)) == m  # an order among equal S is not defined
        out["S"] = S
    else:
        out["ts"] = B + rng.integers(0, 2, m, dtype=np.int64) * TWO[kind]
    return out


def reach(dag, state):
    """What the oracle's `state` (status, order, counts, rr, cts) of the stream `dag` shows
    the kernels must have gone through:
      out_i32 / edge_i32  ordered events with |cts - ts| above / equal to INT32_MAX (the
                          median is one of the gathered timestamps, so such an event had
                          that offset among its values)
      rr_span             call buckets received over more than one round
      rr_span_max         the widest such span
      <class>             per kb_sort size class: `buckets`, `unpacked` (timestamp span
                          >= 2^28), and adjacent ordered pairs equal in (rr, cts, S[:8])
                          (`tie0`) and in (rr, cts, S[:24]) (`tie2`)."""
    status = np.asarray(state["status"])
    acc = status >= 0
    order = np.asarray(state["order"], np.int64)
    E = int(acc.sum())
    ts = np.empty(E, np.int64)
    ts[status[acc]] = np.asarray(dag["ts"], np.int64)[acc]
    S = np.empty((E, 32), np.uint8)
    S[status[acc]] = dag["S"][acc]
    rr = np.asarray(state["rr"], np.int64)[order]
    cts = np.asarray(state["cts"], np.int64)[order]
    off = np.abs(cts - ts[order])
    out = {"out_i32": int((off > INT32_MAX).sum()), "edge_i32": int((off == INT32_MAX).sum()),
           "rr_span": 0, "rr_span_max": 0}
    for name, _, _ in CLASSES:
        out[name] = {"buckets": 0, "unpacked": 0, "tie0": 0, "tie2": 0}
    So = S[order]
    same = (rr[1:] == rr[:-1]) & (cts[1:] == cts[:-1])
    tie0 = same & (So[1:, :8] == So[:-1, :8]).all(axis=1)
    tie2 = same & (So[1:, :24] == So[:-1, :24]).all(axis=1)
    lo = 0
    for cnt in np.asarray(state["counts"], np.int64).tolist():
        hi = lo + cnt
        if cnt >= 2:
            c = out[next(nm for nm, a, b in CLASSES if a <= cnt <= b)]
            c["buckets"] += 1
            c["unpacked"] += int(cts[lo:hi].max() - cts[lo:hi].min() >= SPAN_PACKED)
            c["tie0"] += int(tie0[lo:hi - 1].sum())  # pairs inside the bucket
            c["tie2"] += int(tie2[lo:hi - 1].sum())
            span = int(rr[lo:hi].max() - rr[lo:hi].min())
            out["rr_span"] += span >= 1
            out["rr_span_max"] = max(out["rr_span_max"], span)
        lo = hi
    assert lo == len(order)
    return out


_cache = {}


def oracle_case(case, kind):
    """(stream, calls, oracle state, reach) of a case in a kind: computed once, shared
    by every test that needs it, and left unchanged."""
    from babble_amd.gossip import random_gossip, schedule
    from make_mc_digests import oracle_state
    key = (tuple(case), kind)
    if key not in _cache:
        n, E, k, seed, fk, fp, cp, lag = case
        dag = shape(random_gossip(n, E, seed=seed, forkers=fk, fork_p=fp, cascade_p=cp, op_lag=lag), kind, seed)
        calls = schedule(len(dag["creator"]), k)
        st = oracle_state(dag, calls)
        _cache[key] = (dag, calls, st, reach(dag, st))
    return _cache[key]


def check_reach(case, kind, r):
    """The branches that `kind` exists for, asserted on a reach() of `case`."""
    classes = CASES[tuple(case)]
    if kind in ("gaps", "two31"):
        assert r["out_i32"] > 0, (case, kind, r)
    if kind == "two31m":
        assert r["edge_i32"] > 0 and r["out_i32"] == 0, (case, kind, r)
    if kind == "two28m":
        assert all(r[nm]["unpacked"] == 0 for nm, _, _ in CLASSES), (case, kind, r)
    if kind in ("two28", "two31m", "two31", "spread"):
        for nm in classes:
            assert r[nm]["unpacked"] > 0, (case, kind, nm, r)
    if kind == "ties":
        for nm in classes:
            assert r[nm]["tie0"] > 0 and r[nm]["tie2"] > 0, (case, kind, nm, r)
    if case[0] == 4:
        assert r["rr_span"] > 0, (case, kind, r)
