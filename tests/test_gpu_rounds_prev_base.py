"""The direct rounds walk with member rows handed off in 8-bit form: the workgroup of a
chain stages its next frontier row encoded against the frontier it holds (the next
round's base is the previous frontier, babble_amd/csrc/hge_narrow.h), consumers load the
narrow slice and encode nothing, and the row's condition-(ii) flag travels in the granule.
Every case checks the full state against the oracle (parity.compare_state);
Engine.walk_select_paths() says which path the chain-rounds took.  The plain streams are
those of tests/test_rounds_prev_base_model.py, which shows on the CPU that they stay
inside the narrow range against the previous frontier: hence the 1 % cap here (the model
says 0)."""
import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule
from parity import compare_state, oracle_run, with_creators
from test_gpu_rounds_narrow import fast_creator_stream

pytestmark = pytest.mark.gpu

MIN_ORDERED = 1000

STREAMS = {
    # name: (N, E, K, stream)
    "plain64": (64, 6000, 100, lambda: random_gossip(64, 6000, seed=11)),
    "plain132": (132, 9240, 132, lambda: random_gossip(132, 9240, seed=7)),
    "plain256": (256, 20000, 500, lambda: random_gossip(256, 20000, seed=5)),
    "fast64": (64, 6000, 100, lambda: fast_creator_stream(64, 6000, seed=3)),
    "lag64": (64, 6000, 100, lambda: random_gossip(64, 6000, seed=13, op_lag=8)),
}
_refs = {}


def _reference(name):
    """(N, E, stream, calls, oracle, status, order, counts), computed once per stream."""
    if name not in _refs:
        n, e, k, make = STREAMS[name]
        dag = make()
        calls = schedule(e, k)
        o, ost, oorder, ocounts = oracle_run(dag, calls)
        _refs[name] = (n, e, dag, calls, o, ost, oorder, ocounts)
    return _refs[name]


def _replay_and_check(name, min_ordered=MIN_ORDERED):
    """Bulk replay of the stream, full state against the oracle; returns (narrow, exact)."""
    from babble_amd.engine import Engine
    n, e, dag, calls, o, ost, oorder, ocounts = _reference(name)
    eng = Engine(n, e)
    try:
        st, order, counts = eng.replay(dag, calls)
        with_creators(eng, dag, st)
        np.testing.assert_array_equal(st, ost, err_msg="admission status differs")
        assert len(order) == len(oorder) >= min_ordered, (len(order), len(oorder))
        np.testing.assert_array_equal(order, oorder, err_msg="consensus order differs")
        np.testing.assert_array_equal(counts, ocounts, err_msg="per-call batch sizes differ")
        compare_state(eng, o)
        paths = eng.walk_select_paths()
        print(f"{name}: rounds {eng.rounds()}, walk_select_paths (narrow, exact) = {paths}")
        return paths
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["plain64", "plain132", "plain256"])
def test_plain_streams_stay_narrow_against_the_previous_frontier(name):
    narrow, exact = _replay_and_check(name)
    assert narrow > 0, (narrow, exact)
    assert exact <= 0.01 * (narrow + exact), (narrow, exact)


def test_fast_creator_takes_the_exact_path():
    """Window values far past the range, and frontier advances of more than a window:
    flagged rounds reload the 16-bit rows, which are still staged beside the narrow ones."""
    narrow, exact = _replay_and_check("fast64", min_ordered=200)
    assert exact > 0, (narrow, exact)


def test_stale_other_parents():
    """op_lag = 8 at N = 64: many window values below their (older) base encode as 0."""
    narrow, exact = _replay_and_check("lag64", min_ordered=500)
    assert narrow + exact > 0


def test_exact_hook_same_state(monkeypatch):
    """HGE_TEST_DIR_EXACT=1 at N = 132: every round selects over the 16-bit slice
    reloaded from the 16-bit staging block."""
    monkeypatch.setenv("HGE_TEST_DIR_EXACT", "1")
    narrow, exact = _replay_and_check("plain132")
    assert narrow == 0 and exact > 0, (narrow, exact)


@pytest.mark.parametrize("name", ["plain64", "plain132"])
def test_member_flag_hook_sends_one_round_to_the_exact_select(name, monkeypatch):
    """HGE_TEST_DIR_MEMBER_FLAG=2: chain 1 flags the (fine) row it stages at hand-off epoch
    2, the frontier of round 2.  Every chain with a frontier position in that round then
    takes the 16-bit select for it -- the flag reached every workgroup through the
    granule -- and the state is unchanged."""
    n, e, dag, calls, o, ost, oorder, ocounts = _reference(name)
    narrow0, exact0 = _replay_and_check(name)
    monkeypatch.setenv("HGE_TEST_DIR_MEMBER_FLAG", "2")
    narrow1, exact1 = _replay_and_check(name)
    # chains with a round-2 frontier position: those with an event of round >= 2
    rounds, _ = o.event_rounds()
    creators = np.asarray(dag["creator"])[:len(rounds)]
    chains = len(np.unique(creators[rounds >= 2]))
    assert chains > n // 2, chains
    assert exact1 - exact0 >= chains, (narrow0, exact0, narrow1, exact1, chains)
    assert narrow1 + exact1 == narrow0 + exact0


@pytest.mark.parametrize("name,e_replay", [("plain64", 5000), ("plain256", 15000)])
def test_replay_then_online_calls(name, e_replay):
    """A bulk replay, then 10 online calls: an online call's walk restarts a few rounds
    back and passes over frontier rows kept from earlier calls.  A kept row inside the
    narrow rows of an unflagged round takes its strongly-see bits from one narrow count;
    any other reloads the 16-bit slice before the publish."""
    from babble_amd.engine import Engine, events_array
    n, e, dag, calls, o, ost, oorder, ocounts = _reference(name)
    ev = events_array(dag)
    nrep = int(np.searchsorted(calls, e_replay)) + 1
    assert calls[nrep - 1] == e_replay and len(calls) - nrep == 10
    eng = Engine(n, e)
    try:
        st, order, counts = eng.replay(ev[:e_replay], calls[:nrep])
        np.testing.assert_array_equal(st, ost[:e_replay])
        order, counts = list(order), list(counts)
        nxt = e_replay
        walked = 0
        for c in calls[nrep:]:
            eng.insert_events(ev[nxt:c].copy())
            got = eng.run_consensus()
            walked += sum(eng.walk_select_paths())
            order.extend(got)
            counts.append(len(got))
            nxt = int(c)
        assert walked > 0
        assert len(order) == len(oorder) >= MIN_ORDERED
        np.testing.assert_array_equal(np.asarray(order), oorder, err_msg="consensus order differs")
        np.testing.assert_array_equal(np.asarray(counts), ocounts, err_msg="per-call batch sizes differ")
        with_creators(eng, dag, ost)
        compare_state(eng, o)
    finally:
        eng.close()
