"""The batch kernels chosen by the batch's size, at every width where a path flips,
against the oracle: exactly, field by field, for every graph of the batch.

A run launches the instance of kb_coords, kb_front, kb_pairs / kb_fold, kb_sort's first
class and kb_consensus that hge_batch_plan.h picks from the number of graphs G, of calls and
of fallback graphs against the device's compute-unit count.  The rest of
the suite runs at G <= about 50 and so under the first row of every rule, but for two
batches of config 5's shape (N = 32).  Here G_mid = cus + 8 and G_big = 2 * cus + 8
graphs (tests/batch_variants.py: both sides of every `one` flip of kb_front plus both
width templates; streams in all seven timestamp kinds of ts_shapes.py, a graph past the
bulk fold, coin-bit votes, one-call schedules; neighbouring graphs all different), and
each test asserts Batch.launch_plan() field by field, so it names the instances it ran
and a changed threshold fails here instead of silently removing the coverage.
tests/test_batch_variants.py asserts on the CPU that the streams reach the branches."""
import pytest

from batch_variants import PAST_FOLD, WIDTHS, batch, check_commits, check_states, oracle, sizes

pytestmark = pytest.mark.gpu


def _plan(b, **want):
    plan = b.launch_plan()
    got = {k: plan[k] for k in want}
    assert got == want, f"launch plan {plan}"
    assert plan["nm"] == (32 if b.n <= 32 else 64)


def _ordered(entries):
    return sum(len(oracle(e)[2]["order"]) for e in entries)


@pytest.mark.parametrize("n", WIDTHS)
def test_mid_batch(n):
    """cus < G <= 2 cus: kb_coords<NM, 1024, true>, kb_front<NM, 512>, three pair slots;
    the graph past the bulk fold (N = 5) through kb_consensus<NM, 1>; and a second run."""
    G, _ = sizes()
    b, entries = batch(n, G)
    try:
        past = sum(e[0] == PAST_FOLD for e in entries)
        assert past == (0 if n != 5 else len(range(9, G, 10)))
        for rep in range(2):
            assert b.run() == _ordered(entries)
            _plan(b, coords=1, front_threads=512, ns=3, consensus_occ=1 if past else 0, dlv=0)
            assert b.fallbacks() == past
            check_states(b, entries)
    finally:
        b.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_big_batch(n):
    """G > 2 cus: the self-levelling kb_coords<NM, 512, false>, kb_front<NM, 256>, two pair
    slots (s = 2 decided inline by kb_fold<NM, 2>), one wave per bucket in kb_sort."""
    _, G = sizes()
    b, entries = batch(n, G)
    try:
        past = sum(e[0] == PAST_FOLD for e in entries)
        assert b.run() == _ordered(entries)
        _plan(b, coords=2, front_threads=256, ns=2, sort_threads=64, consensus_occ=1 if past else 0, dlv=0)
        assert b.fallbacks() == past
        check_states(b, entries)
    finally:
        b.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_big_batch_serial(n, monkeypatch):
    """HGB_SERIAL=1 at G > 2 cus: every graph through the occupancy-4 build of kb_consensus."""
    monkeypatch.setenv("HGB_SERIAL", "1")
    _, G = sizes()
    b, entries = batch(n, G)
    try:
        assert b.run() == _ordered(entries)
        assert b.fallbacks() == G
        _plan(b, coords=2, front_threads=256, ns=0, sort_threads=0, consensus_occ=4, dlv=0)
        check_states(b, entries)
    finally:
        b.close()


@pytest.mark.parametrize("n", [16, 33, 64])
def test_big_batch_delivered(n, monkeypatch):
    """The commit records delivered inside the run at G > 2 cus: the DLV instances of
    kb_sort<64, 0, 1024> (bulk) and of kb_consensus<NM, 4> (HGB_SERIAL=1)."""
    _, G = sizes()
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("HGB_SERIAL", "1")
        b, entries = batch(n, G, deliver=True)
        try:
            assert b.run() == _ordered(entries)
            assert b.delivered() == 1
            assert b.fallbacks() == (G if serial else 0)
            if serial:
                _plan(b, coords=2, front_threads=256, consensus_occ=4, dlv=1)
            else:
                _plan(b, coords=2, front_threads=256, ns=2, sort_threads=64, consensus_occ=0, dlv=1)
            check_commits(b, [oracle(e)[2] for e in entries], [f"graph {g}, case {e[0]} {e[1]}" for g, e in enumerate(entries)])
            check_states(b, entries)
        finally:
            b.close()


@pytest.mark.parametrize("n", [32, 64])
def test_small_batch_plan(n):
    """The plan the rest of the suite runs under (G of a few tens): a changed threshold
    shows here."""
    from babble_amd.engine import Batch
    b0 = Batch(n)
    try:
        plan = b0.launch_plan()
        assert plan["cus"] > 0 and all(v == 0 for k, v in plan.items() if k != "cus"), plan
        assert list(plan) == list(Batch.PLAN)
    finally:
        b0.close()
    b, entries = batch(n, 15)
    try:
        assert b.run() == _ordered(entries)
        _plan(b, coords=0, front_threads=1024, ns=3, sort_threads=256, consensus_occ=0, dlv=0)
        assert b.fallbacks() == 0
        check_states(b, entries)
    finally:
        b.close()
