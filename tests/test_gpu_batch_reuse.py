"""One Batch through every transition of its host state, the batch engine's counterpart of
test_gpu_engine_reuse.py: add and run, add more and run again (every pool and table
regrows), what a batch answers between an add and the run that follows it, clear and
generate, clear and add fewer and smaller graphs (every table larger than its contents: a
stale tail must not show), delivery switched on and off over one staged batch, stage()
after a run, and a run of no graphs.  After every run each graph's full state is compared
with the oracle's (batch_variants.check_states), for generated graphs with counter_gossip's
stream as well (as test_gpu_batch_generate.py does).  Everything is an integer: every
assertion is equality.

Widths 5 and 33 (both NM) on batch_variants.BASE's streams, which the other batch tests
have cached.  At N = 5 the second run holds PAST_FOLD (273 rounds, past the bulk fold), so
a run with a fallback graph stands between two bulk-only runs: consensus_occ and
fallbacks() go 0 -> 1 -> 0."""
import functools

import numpy as np
import pytest

from batch_variants import BASE, PAST_FOLD, check_commits, check_states, oracle
from test_gpu_batch_generate import _check_states as check_generated
from test_gpu_batch_generate import _check_stream, _generate
from ts_shapes import KINDS

pytestmark = pytest.mark.gpu

HGE_ERR_ARG = -8
# generate() calls of step 4: (events, k, graphs, seed, forkers, fork_p, cascade_p, op_lag),
# test_gpu_batch_generate.STATE_GROUPS' shapes (its cache serves their first graphs)
GENERATED = {5: [(600, 1, 4, 51, 2, 0.3, 0.5, 3)], 33: [(900, 50, 4, 331, 11, 0.1, 0.5, 3)]}


@functools.lru_cache(maxsize=None)
def _events(entry):
    from babble_amd.engine import events_array
    dag, calls = oracle(entry)[:2]
    return events_array(dag), np.ascontiguousarray(calls, np.int64)


def _add(b, entries):
    for e in entries:
        b.add(*_events(e))


def _ordered(entries):
    return sum(len(oracle(e)[2]["order"]) for e in entries)


def _refused(call, text):
    from babble_amd.engine import HgeError
    with pytest.raises(HgeError) as e:
        call()
    assert e.value.code == HGE_ERR_ARG and text in str(e.value), str(e.value)


def _nothing_to_read(b):
    """Graphs added, generated or cleared since the last run: results, commits and
    statistics are refused; delivery reads 0."""
    if b.graphs():
        _refused(lambda: b.info(0), "no replay yet")
        _refused(lambda: b.state(0), "no replay yet")
        _refused(lambda: b.commits(0), "did not deliver")
    _refused(b.stats, "no run since the batch last changed")
    assert b.delivered() == 0


def _run(b, entries, fallbacks=0, dlv=0):
    assert b.run() == _ordered(entries)
    plan = b.launch_plan()
    assert plan["nm"] == (32 if b.n <= 32 else 64) and plan["cus"] > 0
    # a few graphs: the first row of every rule of DESIGN.md §4.8
    assert (plan["coords"], plan["front_threads"], plan["ns"], plan["sort_threads"]) == (0, 1024, 3, 256), plan
    assert plan["consensus_occ"] == (1 if fallbacks else 0) and plan["dlv"] == dlv, plan
    assert b.fallbacks() == fallbacks
    check_states(b, entries)
    st = b.stats()
    assert len(st["graphs"]) == len(entries) and int(st["graphs"]["ordered"].sum()) == _ordered(entries)


@pytest.mark.parametrize("n", [5, 33])
def test_one_batch_through_every_transition(n):
    from babble_amd.engine import Batch
    small, large = BASE[n][0], BASE[n][-1]
    first = [(small, k) for k in KINDS[:3]]
    more = [(large, k) for k in KINDS[3:7]] + [(PAST_FOLD, None) if n == 5 else (large, KINDS[0])]
    past = 1 if n == 5 else 0
    b = Batch(n)
    try:
        plan0 = b.launch_plan()
        assert plan0["cus"] > 0 and all(v == 0 for k, v in plan0.items() if k != "cus"), plan0
        zero = dict(plan0)

        # 1. add 3 graphs and run
        _add(b, first)
        _nothing_to_read(b)
        _run(b, first)

        # 2. add 5 more (N = 33: longer streams; N = 5 has one base stream, there PAST_FOLD's
        # 6,500 events are the longer one): the pools are laid out again and every part regrows
        _add(b, more)
        _nothing_to_read(b)
        _run(b, first + more, fallbacks=past)

        # 3. between an add and the run that follows it: the last run's plan, fallbacks and
        # stage times still, nothing of its results
        plan, ms = b.launch_plan(), b.kernel_ms()
        assert any(v > 0 for v in ms.values())
        _add(b, first[:1])
        _nothing_to_read(b)
        assert b.launch_plan() == plan and b.fallbacks() == past and b.kernel_ms() == ms
        _run(b, first + more + first[:1], fallbacks=past)

        # 4. clear: plan, fallbacks and delivery zero, the stage times kept; then generated graphs
        ms = b.kernel_ms()
        b.clear()
        assert b.graphs() == 0 and b.launch_plan() == zero and b.fallbacks() == 0 and b.kernel_ms() == ms
        _nothing_to_read(b)
        graphs = _generate(b, GENERATED[n])
        assert len(graphs) == 4
        _nothing_to_read(b)
        assert b.launch_plan() == zero
        b.run()
        assert b.fallbacks() == 0 and b.launch_plan()["consensus_occ"] == 0
        for g, key in graphs:
            _check_stream(b, g, key)
        check_generated(b, None, graphs)

        # 5. clear, then fewer and smaller added graphs than the tables were sized for
        b.clear()
        last = [(small, KINDS[5]), (small, KINDS[1])]
        _add(b, last)
        _run(b, last)

        # 6. delivery off, on (order, rr, cts), off over the same staged batch; it takes
        # effect at the run, and the views describe the run, not the current request
        wants = [oracle(e)[2] for e in last]
        labels = [f"graph {g}, case {e[0]} {e[1]}" for g, e in enumerate(last)]
        b.deliver(False)
        _run(b, last)
        assert b.delivered() == 0
        _refused(lambda: b.commits(0), "did not deliver")
        b.deliver(order=True, received=True)
        assert b.delivered() == 0
        _refused(lambda: b.commits(0), "did not deliver")
        _run(b, last, dlv=1)
        assert b.delivered() == 1
        check_commits(b, wants, labels)
        b.deliver(False)
        assert b.delivered() == 1
        check_commits(b, wants, labels)
        _run(b, last)
        assert b.delivered() == 0
        _refused(lambda: b.commits(0), "did not deliver")

        # 7. stage() after a run: the statistics are refused, the results stay
        b.stage()
        _refused(b.stats, "no run since the batch last changed")
        check_states(b, last)
        assert b.launch_plan()["front_threads"] == 1024

        # 8. no graphs: a run of nothing, a histogram of zeros
        b.clear()
        assert b.run() == 0
        assert b.launch_plan() == zero and b.fallbacks() == 0 and b.delivered() == 0
        st = b.stats()
        assert len(st["graphs"]) == 0 and not st["hist"].any()
    finally:
        b.close()
