"""The batch engine's commit stream delivered to host memory inside the run
(hge_batch_set_delivery / hge_batch_commits_view, Batch.deliver / Batch.commits)
against the live oracle.

With delivery on, the sort kernels (kb_sort's LDS and in-HBM sites) and kb_consensus
(its LDS and global-scratch sites) store each graph's consensus order, the per-call
batch sizes and, when asked, every ordered event's round received and consensus
timestamp into mapped pinned host memory.  Every stream here is the smallest that
reaches one writer or sort class; b.fallbacks() is asserted in every case, so that a
stream cannot silently take another path."""
import os
import sys

import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

# n, events, k, seed, forkers, fork_p, cascade_p, op_lag
SMALL_K1 = (4, 1000, 1, 2, 0, 0.0, 0.0, 0)         # many small buckets
SMALL_K4 = (4, 1000, 4, 1, 0, 0.0, 0.0, 0)
REJECTS = (32, 3000, 32, 4, 10, 0.05, 0.5, 0)      # rejected submissions: ids are graph-local
MID = (32, 5000, 700, 25, 0, 0.0, 0.0, 0)          # 513-1,024-key buckets
ONE_CALL = (4, 1500, 1500, 12, 0, 0.0, 0.0, 0)     # one 1.4k-key bucket (1,024 < n <= 4,096); coin rounds
BIG16 = (16, 14000, 6000, 31, 0, 0.0, 0.0, 0)      # buckets past 4,096 keys, an empty call in between
BIG32 = (32, 14000, 6000, 33, 0, 0.0, 0.0, 0)
WIDE64 = (64, 6000, 64, 18, 0, 0.0, 0.0, 0)        # the 64-wide template
WIDE33 = (33, 3000, 50, 17, 0, 0.0, 0.0, 3)
LONG1 = (1, 700, 5, 5, 0, 0.0, 0.0, 0)             # ~700 rounds: past the bulk fold, kb_consensus
LONG4 = (4, 4000, 40, 7, 0, 0.0, 0.0, 0)           # the same with four participants: it orders events
SHORT1 = (1, 50, 5, 3, 0, 0.0, 0.0, 0)
NOTHING = (4, 8, 4, 1, 0, 0.0, 0.0, 0)             # orders nothing

_cache = {}


def _case(case):
    """(dag, calls, oracle state) of a stream, computed once and shared (read-only)."""
    if case not in _cache:
        n, E, k, seed, fk, fp, cp, lag = case
        dag = random_gossip(n, E, seed=seed, forkers=fk, fork_p=fp, cascade_p=cp, op_lag=lag)
        calls = schedule(len(dag["creator"]), k)
        from make_mc_digests import oracle_state
        _cache[case] = (dag, calls, oracle_state(dag, calls))
    return _cache[case]


def _check_commits(b, g, w, received=True, label=""):
    c = b.commits(g)
    ids, counts = c["ids"], c["counts"]
    assert len(ids) == len(w["order"]) == b.info(g)["ordered"], label
    assert np.array_equal(ids, w["order"]), f"{label}: ids"
    assert np.array_equal(counts, w["counts"]), f"{label}: counts"
    assert ids.dtype == np.int32 and counts.dtype == np.int64
    if received:
        assert c["rr"].dtype == np.int32 and c["cts"].dtype == np.int64
        assert np.array_equal(c["rr"], np.asarray(w["rr"])[ids]), f"{label}: rr"
        assert np.array_equal(c["cts"], np.asarray(w["cts"])[ids]), f"{label}: cts"
    else:
        assert c["rr"] is None and c["cts"] is None
    return c


def _check_batch(b, cases, received=True):
    from digest import first_difference
    for g, case in enumerate(cases):
        w = _case(case)[2]
        _check_commits(b, g, w, received, f"case {case}")
        diff = first_difference(b.state(g), w)  # results() with delivery on
        assert diff is None, f"case {case}: first differing field {diff}"


def _run(cases, received=True, n=None):
    from babble_amd.engine import Batch
    b = Batch(n or cases[0][0])
    for case in cases:
        dag, calls, _ = _case(case)
        b.add(dag, calls)
    b.deliver(order=True, received=received)
    tot = b.run()
    assert tot == sum(len(_case(c)[2]["order"]) for c in cases)
    return b


BULK = {
    "small_buckets": [SMALL_K1, SMALL_K4, NOTHING],
    "wave_per_bucket": [SMALL_K1] * 5,   # more than 4,096 calls in the batch: one wave per bucket
    "rejected_and_mid": [REJECTS, MID],
    "one_call": [ONE_CALL],
    "wide64": [WIDE64],
    "wide33": [WIDE33],
}


@pytest.mark.parametrize("name", sorted(BULK))
def test_commits_bulk_paths(name):
    cases = BULK[name]
    b = _run(cases)
    try:
        assert b.delivered() == 1
        assert b.fallbacks() == 0
        _check_batch(b, cases)
    finally:
        b.close()


def test_rejected_submissions_give_graph_local_ids():
    dag, calls, w = _case(REJECTS)
    assert (w["status"] < 0).any()  # the stream has rejected submissions
    b = _run([REJECTS])
    try:
        assert b.fallbacks() == 0
        ids = b.commits(0)["ids"]
        assert ids.max() < b.info(0)["events"] < len(dag["creator"])
    finally:
        b.close()


@pytest.mark.parametrize("case,sizes,rounds", [(BIG16, [5661, 0, 8018], 115), (BIG32, [5076, 0, 8168], 47)],
                         ids=["n16", "n32"])
def test_commits_buckets_past_4096_keys(case, sizes, rounds):
    """The in-HBM sort's final loop, with an empty call in between."""
    w = _case(case)[2]
    assert list(w["counts"]) == sizes and max(sizes) > 4096
    assert int(w["scalars"][0]) == rounds <= 256  # inside the bulk fold's limit
    b = _run([case])
    try:
        assert b.delivered() == 1
        assert b.fallbacks() == 0
        _check_batch(b, [case])
    finally:
        b.close()


def test_commits_nothing_ordered():
    w = _case(NOTHING)[2]
    assert len(w["order"]) == 0
    b = _run([NOTHING])
    try:
        assert b.fallbacks() == 0
        c = _check_commits(b, 0, w, True, "nothing")
        assert len(c["ids"]) == 0 and len(c["rr"]) == 0 and len(c["cts"]) == 0
        assert len(c["counts"]) == len(_case(NOTHING)[1]) and not c["counts"].any()
    finally:
        b.close()


@pytest.mark.parametrize("cases", [[LONG1, SHORT1], [SMALL_K4, LONG4, ONE_CALL]], ids=["n1", "n4"])
def test_commits_fallback_mixed_with_bulk(cases):
    """A graph past the bulk fold's 256 rounds, replayed by kb_consensus after the bulk
    pass (its LDS sort site), beside bulk graphs: both deliver into the one set of buffers.
    The single-participant stream orders nothing, so its part is the counts; the
    four-participant one orders most of its events."""
    long = [c for c in cases if int(_case(c)[2]["scalars"][0]) > 256]
    assert len(long) == 1
    if cases[0][0] == 4:
        assert len(_case(long[0])[2]["order"]) > 3000
    b = _run(cases)
    try:
        assert b.delivered() == 1
        assert b.fallbacks() == 1
        _check_batch(b, cases)
    finally:
        b.close()


@pytest.mark.parametrize("case", [BIG16, SMALL_K4], ids=["global_scratch", "lds"])
def test_commits_serial_path(case, monkeypatch):
    """HGB_SERIAL=1: every graph through kb_consensus (BIG16: its global-scratch sort site)."""
    monkeypatch.setenv("HGB_SERIAL", "1")
    b = _run([case])
    try:
        assert b.delivered() == 1
        assert b.fallbacks() == 1
        _check_batch(b, [case])
    finally:
        b.close()


def test_stale_data_must_show():
    """A third graph shifts the pooled offsets: every slot has to be written again."""
    cases = [SMALL_K4, ONE_CALL, SMALL_K1]
    b = _run(cases[:2])
    try:
        assert b.fallbacks() == 0
        _check_batch(b, cases[:2])
        dag, calls, _ = _case(cases[2])
        b.add(dag, calls)
        from babble_amd.engine import HgeError
        with pytest.raises(HgeError):
            b.commits(0)  # the added graph invalidated the last run
        for _ in range(2):  # the second run without changes
            b.run()
            assert b.delivered() == 1 and b.fallbacks() == 0
            _check_batch(b, cases)
    finally:
        b.close()


def test_modes():
    cases = [SMALL_K4, ONE_CALL]
    b1 = _run(cases, received=False)
    b3 = _run(cases, received=True)
    try:
        assert b1.delivered() == 1 and b3.delivered() == 1
        assert b1.fallbacks() == 0 and b3.fallbacks() == 0
        _check_batch(b1, cases, received=False)
        _check_batch(b3, cases, received=True)
        for g in range(len(cases)):
            c1, c3 = b1.commits(g), b3.commits(g)
            assert c1["rr"] is None and c1["cts"] is None
            assert np.array_equal(c1["ids"], c3["ids"]) and np.array_equal(c1["counts"], c3["counts"])
        # the same batch switched from one mode to the other
        b1.deliver(order=True, received=True)
        b1.run()
        _check_batch(b1, cases, received=True)
        b1.deliver(order=True, received=False)
        b1.run()
        _check_batch(b1, cases, received=False)
    finally:
        b1.close()
        b3.close()


def test_views_do_not_copy_and_keep_the_batch():
    b = _run([SMALL_K4])
    try:
        c, c2 = b.commits(0), b.commits(0)
        for k in ("ids", "rr", "cts", "counts"):
            assert not c[k].flags.owndata and not c[k].flags.writeable
            assert c[k].ctypes.data == c2[k].ctypes.data  # the batch's own buffer both times
            assert c[k].base.owner is b
    finally:
        b.close()


@pytest.mark.parametrize("cases", [[SMALL_K4, ONE_CALL], [BIG16]], ids=["lds", "past_4096"])
def test_copy_fallback(cases, monkeypatch):
    """HGB_TEST_NO_PIN=1: no pinned memory, the same buffers filled by copies after the run."""
    monkeypatch.setenv("HGB_TEST_NO_PIN", "1")
    b = _run(cases)
    try:
        assert b.delivered() == 2
        assert b.fallbacks() == 0
        _check_batch(b, cases)
        b.deliver(order=True, received=False)  # the copies of ids and counts alone
        b.run()
        assert b.delivered() == 2
        _check_batch(b, cases, received=False)
    finally:
        b.close()


def test_refusals():
    from babble_amd.engine import Batch, HgeError
    dag, calls, w = _case(SMALL_K4)
    b = Batch(4)
    try:
        b.add(dag, calls)
        with pytest.raises(HgeError):
            b.commits(0)  # before any run
        b.run()
        assert b.delivered() == 0
        with pytest.raises(HgeError):
            b.commits(0)  # a run with delivery off
        with pytest.raises(HgeError):
            b.deliver(order=False, received=True)
        b.run()
        with pytest.raises(HgeError):
            b.commits(0)  # the refused mode changed nothing
        b.deliver()
        b.run()
        assert b.delivered() == 1
        assert np.array_equal(b.commits(0)["ids"], w["order"])
        for g in (-1, 1):
            with pytest.raises(HgeError):
                b.commits(g)
        b.deliver(order=False)
        b.run()
        assert b.delivered() == 0
        with pytest.raises(HgeError):
            b.commits(0)
    finally:
        b.close()


def test_default_path_unchanged():
    """Delivery never enabled: delivered() is 0 and the state equals the oracle."""
    from babble_amd.engine import Batch
    from digest import first_difference
    cases = [SMALL_K4, ONE_CALL]
    b = Batch(4)
    try:
        for case in cases:
            b.add(*_case(case)[:2])
        b.run()
        if hasattr(b, "delivered"):
            assert b.delivered() == 0
        assert b.fallbacks() == 0
        for g, case in enumerate(cases):
            assert first_difference(b.state(g), _case(case)[2]) is None, f"case {case}"
    finally:
        b.close()
