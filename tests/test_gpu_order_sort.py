"""The order stage sorts a call bucket of 513 .. 16,384 keys on packed 64-bit keys in
registers (packed_bitonic, babble_amd/csrc/hge_kernels.hip and hge_sortkey.h) and keeps
the LDS index sort for a bucket whose roundReceived and timestamp ranges do not pack.
Every case replays one N = 64 stream of 40,000 events against the live oracle: the order
and the per-call counts must be equal, and Engine.sort_paths() must show the intended
path for every such bucket.

The call schedule is irregular: a call after a gap of G submissions receives about G
events, so gaps of 900, 1,700, 3,200, 6,400 and 12,500 put buckets into every size class
the sort distinguishes (1,024, 2,048, 4,096 and 8,192 slots, and the two-halves merge
path past 8,192 keys).  The wide gaps also put several roundReceived values into one
bucket.  Two schedules: 49 calls (the bulk replay's k_bucket_sort_big) and 8 calls
(k_bucket_sort_all, the launch an online call takes).  The oracle's own batch sizes say
which classes a schedule hit, and the tests assert on them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from babble_amd.gossip import random_gossip
from parity import oracle_run

pytestmark = pytest.mark.gpu

N, E, SEED = 64, 40000, 21
GAPS = [900, 1700, 3200, 6400, 12500]
CLASSES = [(513, 1024), (1025, 2048), (2049, 4096), (4097, 8192), (8193, 16384)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sched_many():
    """Four calls 250 apart, then one after each gap; 400 apart to the end: 49 calls."""
    calls, p = [], 0
    for g in [2000] + GAPS:
        for q in range(p + 250, p + 1001, 250):
            calls.append(q)
        p = calls[-1] + g
        calls.append(p)
    while p + 400 < E:
        p += 400
        calls.append(p)
    calls.append(E)
    return np.array(sorted(set(calls)), np.int64)


def sched_few():
    """Eight calls.  Events are received a round (~700 events) at a time, so the call points
    are chosen from the oracle's received count per 100 submissions: the batches are
    1,906, 1,320, 2,841, 4,237, 749, 7,068, 10,370 and 9,608 events (asserted by class)."""
    return np.array([3500, 4900, 7700, 12100, 13100, 20000, 30000, E], np.int64)


def stream(kind):
    dag = random_gossip(N, E, seed=SEED)
    if kind == "ties":
        # the top 32 bits of every S equal: keys with equal medians reach the full-key compare
        S = dag["S"].copy()
        S[:, :4] = np.array([0x5A, 0x01, 0xFE, 0x33], np.uint8)
        dag["S"] = S
    elif kind == "jump":
        # one jump of 2^33 ns mid-stream (still strictly increasing): the bucket whose
        # medians straddle it spans more than 32 bits of timestamp
        ts = dag["ts"].copy()
        ts[JUMP_AT:] += 1 << 33
        dag["ts"] = ts
    return dag


# inside the 3,200 gap of sched_many (submissions 8,600 .. 11,800): a 2-4k bucket, sorted whole
JUMP_AT = 10000

_refs = {}


def _reference(kind, sched):
    """(stream, calls, oracle, status, order, counts), computed once per (stream, schedule)."""
    key = (kind, sched)
    if key not in _refs:
        dag = stream(kind)
        calls = sched_many() if sched == "many" else sched_few()
        o, ost, oorder, ocounts = oracle_run(dag, calls)
        _refs[key] = (dag, calls, o, ost, oorder, ocounts)
    return _refs[key]


def _big(counts):
    return [int(c) for c in counts if 512 < c <= 16384]


def _classes_hit(counts):
    return [sum(lo <= c <= hi for c in counts) for lo, hi in CLASSES]


def _expected_paths(o, oorder, ocounts):
    """(packed, index) by the packing rule over the oracle's batches: a batch packs when
    bits(rr span) + bits(cts span) <= 32.  A batch past 8,192 keys is sorted as two halves
    of the engine's choosing: it packs for certain only when the whole batch does, so the
    streams here keep every such batch packable (asserted)."""
    rr, cts = o.event_received()
    packed = index = 0
    pos = 0
    for c in ocounts:
        ids = oorder[pos:pos + c]
        pos += c
        if not 512 < c <= 16384:
            continue
        r, t = rr[ids].astype(np.int64), cts[ids].astype(np.int64)
        bits = int(r.max() - r.min()).bit_length() + int(t.max() - t.min()).bit_length()
        if bits <= 32:
            packed += 1
        else:
            assert c <= 8192, "an unpackable batch past 8,192 keys: the halves' paths are the engine's choice"
            index += 1
    return packed, index


def _replay(kind, sched):
    from babble_amd.engine import Engine
    dag, calls, o, ost, oorder, ocounts = _reference(kind, sched)
    eng = Engine(N, E)
    try:
        st, order, counts = eng.replay(dag, calls)
        np.testing.assert_array_equal(st, ost, err_msg="admission status differs")
        assert len(order) == len(oorder) > 30000, (len(order), len(oorder))
        np.testing.assert_array_equal(order, oorder, err_msg="consensus order differs")
        np.testing.assert_array_equal(counts, ocounts, err_msg="per-call batch sizes differ")
        paths = eng.sort_paths()
        print(f"{kind}/{sched}: {len(calls)} calls, batches past 512 keys {_big(ocounts)}, "
              f"sort_paths (packed, index) = {paths}")
        return paths, (o, oorder, ocounts)
    finally:
        eng.close()


def test_schedules_hit_every_size_class():
    """The oracle's batch sizes: both schedules put a bucket into each of the five classes;
    the schedules differ in the launch they take (more than 8 calls, at most 8)."""
    for sched, ncalls_ok in (("many", lambda n: n > 8), ("few", lambda n: n <= 8)):
        _, calls, _, _, _, ocounts = _reference("plain", sched)
        assert ncalls_ok(len(calls)), len(calls)
        hit = _classes_hit(ocounts)
        print(f"{sched}: {len(calls)} calls, batches past 512 keys {_big(ocounts)}, per class {hit}")
        assert all(h > 0 for h in hit), (sched, hit, _big(ocounts))


@pytest.mark.parametrize("sched", ["many", "few"])
def test_every_bucket_packed(sched):
    """Plain stream: every bucket of 513 .. 16,384 keys is packable and sorts packed."""
    (packed, index), (o, oorder, ocounts) = _replay("plain", sched)
    assert all(h > 0 for h in _classes_hit(ocounts))
    assert (packed, index) == _expected_paths(o, oorder, ocounts) == (len(_big(ocounts)), 0)


def test_ties_reach_the_full_key():
    """The top 32 bits of S constant: events with equal medians have equal sort words and
    are ordered by the full key from HBM."""
    (packed, index), (o, oorder, ocounts) = _replay("ties", "many")
    rr, cts = o.event_received()
    # equal (rr, cts) pairs do occur inside the big batches: the tie branch is exercised
    pos = ties = 0
    for c in ocounts:
        ids = oorder[pos:pos + c]
        pos += c
        if 512 < c <= 16384:
            k = np.stack([rr[ids].astype(np.int64), cts[ids].astype(np.int64)], 1)
            ties += int((np.diff(k, axis=0) == 0).all(axis=1).sum())
    print(f"adjacent equal (rr, cts) pairs inside the big batches: {ties}")
    assert ties > 0
    assert all(h > 0 for h in _classes_hit(ocounts))
    assert (packed, index) == (len(_big(ocounts)), 0)


def test_unpackable_bucket_takes_the_index_sort():
    """One timestamp jump of 2^33 ns: the bucket that straddles it reports `index`, the
    others `packed`."""
    (packed, index), (o, oorder, ocounts) = _replay("jump", "many")
    exp = _expected_paths(o, oorder, ocounts)
    assert exp[1] >= 1, exp
    assert (packed, index) == exp
    assert packed + index == len(_big(ocounts))


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
from babble_amd.engine import Engine
from babble_amd.gossip import random_gossip
ref = np.load({ref!r})
eng = Engine({n}, {e})
st, order, counts = eng.replay(random_gossip({n}, {e}, seed={seed}), ref["calls"])
np.testing.assert_array_equal(order, ref["order"], err_msg="consensus order differs")
np.testing.assert_array_equal(counts, ref["counts"], err_msg="per-call batch sizes differ")
print("forced index paths", *eng.sort_paths())
eng.close()
"""


def test_forced_index_sort_same_order(tmp_path):
    """HGE_TEST_SORT_INDEX=1 in a fresh process: every bucket takes the index sort, the
    order is the oracle's all the same."""
    dag, calls, o, ost, oorder, ocounts = _reference("plain", "many")
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, calls=calls, order=oorder, counts=ocounts)
    env = dict(os.environ, HGE_TEST_SORT_INDEX="1")
    code = _CHILD.format(root=ROOT, ref=ref, n=N, e=E, seed=SEED)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"forced index paths 0 {len(_big(ocounts))}" in out.stdout, out.stdout
