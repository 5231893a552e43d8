"""The timestamp shapes of tests/ts_shapes.py reach the branches they exist for: the
oracle's state of every (case, kind) of the batch engine's timestamp tests shows events
whose median offsets leave int32 (or sit on its edge), call buckets that kb_sort cannot
pack, and keys that tie past S's first limb, in every size class the case fills.  Oracle
only; tests/test_gpu_batch_timestamps.py runs the same streams on the device."""
import numpy as np
import pytest

import ts_shapes
from ts_shapes import CASES, CLASSES, KINDS, check_reach, oracle_case, reach, shape


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("kind", KINDS)
def test_shape_reaches_its_branch(case, kind):
    dag, calls, st, r = oracle_case(case, kind)
    assert len(st["order"]) > 500  # (wide graphs with lagging other-parents order a third of their events)
    for nm in CASES[case]:
        assert r[nm]["buckets"] > 0, (case, kind, nm, r)
    check_reach(case, kind, r)
    # no stream here has a bucket over 16 rounds or more: that half of kb_sort's packing
    # condition is not reached by these tests
    assert r["rr_span_max"] < 16


def test_shapes_cover_every_submission():
    """The recipes index by submission position: fork twins and cascade records get a
    shaped timestamp too, `ties` leaves S distinct with its last limb untouched, and the
    two-valued kinds hold exactly their two values."""
    from babble_amd.gossip import random_gossip
    dag = random_gossip(32, 3000, seed=33, forkers=10, fork_p=0.05, cascade_p=0.5)
    m = len(dag["creator"])
    assert m > 3000
    for kind in KINDS:
        s = shape(dag, kind, 33)
        assert s["ts"].shape == (m,) and s["ts"].dtype == np.int64
        assert s["ts"] is not dag["ts"] and s["creator"] is dag["creator"]
        if kind in ts_shapes.TWO:
            assert sorted(set((s["ts"] - ts_shapes.B).tolist())) == [0, ts_shapes.TWO[kind]]
        if kind == "ties":
            assert len(np.unique(s["S"], axis=0)) == m
            assert np.array_equal(s["S"][:, 24:], dag["S"][:, 24:])
            assert (s["S"][:, :8] == 0x5A).all() and (s["S"][::2, 8:24] == 0x11).all()
            assert np.array_equal(s["S"][1::2, 8:24], dag["S"][1::2, 8:24])
        else:
            assert s["S"] is dag["S"]
    sp = shape(dag, "spread", 33)["ts"] - ts_shapes.B
    assert sp.min() > -(1 << 30) and sp.max() < (1 << 30) and (np.diff(sp) < 0).any()


def test_reach_counts_a_hand_made_state():
    """reach() on a state small enough to count by hand: two call buckets of three keys."""
    S = np.zeros((6, 32), np.uint8)
    S[:, 31] = np.arange(6)
    S[2, 0] = 1      # event 2 differs from the rest in limb 0
    S[4, 20] = 1     # event 4 in limb 2
    dag = {"ts": np.array([0, 10, 20, 30, 40, 50], np.int64), "S": S}
    state = {"status": np.arange(6), "order": np.array([0, 1, 2, 3, 4, 5]), "counts": np.array([3, 0, 3]),
             "rr": np.array([1, 1, 1, 2, 2, 3]),
             "cts": np.array([5, 5, 5, 30 + ts_shapes.INT32_MAX, 30 + ts_shapes.INT32_MAX, 51 + ts_shapes.INT32_MAX])}
    r = reach(dag, state)
    assert r["out_i32"] == 1 and r["edge_i32"] == 1  # events 5 and 3 (event 4's offset is INT32_MAX - 10)
    assert r["rr_span"] == 1 and r["rr_span_max"] == 1
    small = r[CLASSES[0][0]]
    # bucket 0: pairs (0,1) tie through limb 2, (1,2) differ in limb 0; bucket 1: (3,4) tie in limb 0 only
    assert small == {"buckets": 2, "unpacked": 0, "tie0": 2, "tie2": 1}
    assert all(r[nm]["buckets"] == 0 for nm, _, _ in CLASSES[1:])
    state["cts"] = np.array([5, 5, 5 + (1 << 28), 30, 30 + (1 << 28) - 1, 31])
    assert reach(dag, state)[CLASSES[0][0]]["unpacked"] == 1
