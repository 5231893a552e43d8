"""Batches past the batch engine's size thresholds, at the widths where its kernels
change path (a test helper; tests/test_batch_variants.py, tests/test_gpu_batch_variants.py).

A run launches a template instance of almost every batch kernel chosen (hge_batch_plan.h)
from the batch's size against the device's compute-unit count (DESIGN.md §4.8;
Batch.launch_plan() names the choice), and inside kb_front the thread count selects one
(member, chain) pair per thread while N * N fits the workgroup, a strided loop above:
N = 32 / 33 at 1,024 threads, 22 / 23 at 512, 16 / 17 at 256.  WIDTHS holds both sides
of every flip, an odd small width and the widest of both templates.

Each width has base streams, taken in all seven timestamp kinds of ts_shapes.py (so the
sort instances chosen by the batch's size meet unpackable spans and full-key ties), and
at N = 5 and 32 additions: plain-timestamp streams (kind None) and one (case, kind).
distinct(n) lists them; batch(n, G) adds graph g = distinct[g % len(distinct)], so
neighbouring graphs differ in events, calls and rounds and the per-graph offsets are
irregular.  oracle(entry) is the cache of (stream, calls, oracle state, reach or
DecideFame statistics), shared by every test and left unchanged."""
import numpy as np

import ts_shapes
from ts_shapes import KINDS

WIDTHS = (5, 16, 17, 22, 23, 32, 33, 64)

# n, events, k, seed, forkers, fork_p, cascade_p, op_lag; the 32, 33 and 64 wide share
# ts_shapes.CASES' streams (and its cache)
BASE = {
    5: [(5, 1500, 40, 32, 0, 0.0, 0.0, 3)],
    16: [(16, 2000, 16, 61, 5, 0.05, 0.5, 0), (16, 2500, 600, 62, 0, 0.0, 0.0, 3)],
    17: [(17, 2000, 17, 63, 0, 0.0, 0.0, 0), (17, 2500, 600, 64, 6, 0.1, 0.5, 3)],
    22: [(22, 2500, 22, 65, 7, 0.05, 0.5, 0), (22, 3000, 700, 66, 0, 0.0, 0.0, 2)],
    23: [(23, 2500, 23, 67, 0, 0.0, 0.0, 3), (23, 3000, 700, 68, 0, 0.0, 0.0, 0)],
    32: [(32, 3000, 32, 33, 10, 0.05, 0.5, 0), (32, 3000, 700, 7, 0, 0.0, 0.0, 0)],
    33: [(33, 2500, 50, 36, 0, 0.0, 0.0, 3), (33, 3000, 800, 69, 11, 0.1, 0.5, 0)],
    64: [(64, 5000, 64, 37, 0, 0.0, 0.0, 0), (64, 5000, 1500, 38, 0, 0.0, 0.0, 0)],
}
# base streams whose large-K calls also fill kb_sort's second size class
FILLS_4096 = [(22, 3000, 700, 66, 0, 0.0, 0.0, 2), (33, 3000, 800, 69, 11, 0.1, 0.5, 0),
              (32, 3000, 700, 7, 0, 0.0, 0.0, 0)] + BASE[64]

K3 = (5, 2000, 3, 13, 0, 0.0, 0.0, 0)             # test_gpu_batch.CASES': a call every three submissions
COIN_VOTE = (5, 1500, 1500, 12, 0, 0.0, 0.0, 3)   # one call: coin-bit votes taken (hashgraph.go:647)
PAST_FOLD = (5, 6500, 600, 41, 0, 0.0, 0.0, 0)    # 273 rounds: past the bulk fold, replayed by kb_consensus
ONE_CALL_32 = (32, 7000, 7000, 35, 0, 0.0, 0.0, 0)  # ts_shapes': a bucket past 4,096 keys
# (case, kind) added to a width's base streams x KINDS; kind None: random_gossip's own timestamps
EXTRA = {5: [(K3, None), (COIN_VOTE, None), (PAST_FOLD, None)], 32: [(ONE_CALL_32, "spread")]}


def distinct(n):
    """The (case, kind) entries of width n, in the order batch() cycles through."""
    return [(c, k) for c in BASE[n] for k in KINDS] + EXTRA.get(n, [])


_plain = {}
_events = {}


def oracle(entry):
    """(stream, calls, oracle state, info) of a (case, kind): info is ts_shapes.reach() for
    a kind, the oracle's DecideFame statistics for kind None.  Computed once."""
    case, kind = entry
    if kind is not None:
        return ts_shapes.oracle_case(case, kind)
    if case not in _plain:
        from babble_amd.gossip import random_gossip, schedule
        from make_mc_digests import oracle_state
        n, E, k, seed, fk, fp, cp, lag = case
        dag = random_gossip(n, E, seed=seed, forkers=fk, fork_p=fp, cascade_p=cp, op_lag=lag)
        calls = schedule(len(dag["creator"]), k)
        stats = {}
        st = oracle_state(dag, calls, stats=stats)
        _plain[case] = (dag, calls, st, stats)
    return _plain[case]


def sizes(n=5):
    """(G_mid, G_big): the batch sizes just past one and two graphs per compute unit of
    this device, where kb_front drops to 512 and to 256 threads and every rule on
    G > 2 * cus flips."""
    from babble_amd.engine import Batch
    b = Batch(n)
    try:
        cus = b.launch_plan()["cus"]
    finally:
        b.close()
    assert cus > 0
    return cus + 8, 2 * cus + 8


def batch(n, G, deliver=False):
    """A Batch of G graphs of width n, graph g = distinct(n)[g % len(distinct(n))], not yet
    run; returns (batch, the entry of every graph).  HGB_SERIAL is read when the Batch is
    constructed: set it before."""
    from babble_amd.engine import Batch, events_array
    ds = distinct(n)
    for e in ds:
        if e not in _events:
            dag, calls = oracle(e)[:2]
            _events[e] = (events_array(dag), np.ascontiguousarray(calls, np.int64))
    entries = [ds[g % len(ds)] for g in range(G)]
    b = Batch(n)
    try:
        for e in entries:
            b.add(*_events[e])
        if deliver:
            b.deliver(order=True, received=True)
    except BaseException:
        b.close()
        raise
    return b, entries


def check_states(b, entries):
    """Every graph's full state equal to the oracle's, field by field."""
    from digest import first_difference
    for g, e in enumerate(entries):
        diff = first_difference(b.state(g), oracle(e)[2])
        assert diff is None, f"graph {g}, case {e[0]} {e[1]}: first differing field {diff}"


def check_commits(b, wants, labels):
    """The delivered commit records of every graph (ids, counts, rr, cts, as
    test_gpu_batch_commit.py checks them) against the oracle states `wants`."""
    for g, (w, label) in enumerate(zip(wants, labels)):
        cm = b.commits(g)
        ids, counts = cm["ids"], cm["counts"]
        assert len(ids) == len(w["order"]) == b.info(g)["ordered"], label
        assert np.array_equal(ids, w["order"]), f"{label}: ids"
        assert np.array_equal(counts, w["counts"]), f"{label}: counts"
        assert ids.dtype == np.int32 and counts.dtype == np.int64
        assert cm["rr"].dtype == np.int32 and cm["cts"].dtype == np.int64
        assert np.array_equal(cm["rr"], np.asarray(w["rr"])[ids]), f"{label}: rr"
        assert np.array_equal(cm["cts"], np.asarray(w["cts"])[ids]), f"{label}: cts"
