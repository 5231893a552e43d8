"""The batch engine's median and sort on timestamps as real clocks give them
(tests/ts_shapes.py: gaps, spread, ties and the two-valued boundary kinds), against the
oracle, exactly and field by field (MedianTimestamp, hashgraph.go:762-770: the upper
median; consensus_sorter.go:36-59: round received, timestamp, S as a big integer).

Every other batch test runs on random_gossip's own fields, timestamps 1 us apart in
submission order and uniform S, which never leave kb_median's int32 register sort,
kb_sort's packed 64-bit prefix or key_less's first limb.  These streams do:

  gaps, two31      median offsets outside int32: kb_median's exact 64-bit rank search
                   (bulk) and kb_consensus's twin of it (HGB_SERIAL=1)
  two31m           offsets of exactly +-INT32_MAX: the int32 sort, where the value equals
                   the sort's filler
  spread, two28, two31m, two31
                   call buckets whose timestamps span 2^28 ns or more: kb_sort's prefix is
                   0 and every comparison is the full key from HBM
  two28m           a span of 2^28 - 1: the packed timestamp field's top bit beside the
                   round field (in use at N = 4, whose buckets span two rounds)
  ties             keys equal in (rr, cts, S's first limb), half of them down to the last
                   limb: key_less's loop over limbs 1..3, in kb_sort's three size classes
                   and in kb_consensus's sort_keys_lds / sort_keys_g

tests/test_ts_shapes.py asserts, from the oracle alone, that each stream reaches its
branch in every size class; the states here come from the same cache.  Every test asserts
fallbacks(), so no graph silently takes the other path.  Not reached: a bucket over 16
rounds or more (the other half of kb_sort's packing condition); the widest here is 1."""
import pytest

from batch_variants import check_commits
from ts_shapes import CASES, KINDS, WIDTHS, check_reach, oracle_case

pytestmark = pytest.mark.gpu


def _graphs(n):
    """(case, kind) of every graph of width n, in the batch's order."""
    return [(c, k) for c in CASES if c[0] == n for k in KINDS]


def _batch(n, deliver=False):
    from babble_amd.engine import Batch
    graphs = _graphs(n)
    assert 0 < len(graphs) <= 21
    for c, k in graphs:
        check_reach(c, k, oracle_case(c, k)[3])
    b = Batch(n)
    try:
        for c, k in graphs:
            dag, calls, _, _ = oracle_case(c, k)
            b.add(dag, calls)
        if deliver:
            b.deliver(order=True, received=True)
        tot = b.run()
    except BaseException:
        b.close()
        raise
    return b, graphs, tot


def _check_states(b, graphs):
    from digest import first_difference
    for g, (c, k) in enumerate(graphs):
        diff = first_difference(b.state(g), oracle_case(c, k)[2])
        assert diff is None, f"case {c} {k}: first differing field {diff}"


def _check_commits(b, graphs):
    """As test_gpu_batch_commit.py's _check_commits: the delivered records against the oracle."""
    check_commits(b, [oracle_case(c, k)[2] for c, k in graphs], [f"case {c} {k}" for c, k in graphs])


@pytest.mark.parametrize("n", WIDTHS)
def test_batch_shapes_match_oracle(n):
    """Every case of width n in every kind, one batch, in bulk; and a second run of it."""
    b, graphs, tot = _batch(n)
    try:
        assert b.fallbacks() == 0
        assert tot == sum(len(oracle_case(c, k)[2]["order"]) for c, k in graphs)
        _check_states(b, graphs)
        assert b.run() == tot
        assert b.fallbacks() == 0
        _check_states(b, graphs)
    finally:
        b.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_batch_shapes_serial_path(n, monkeypatch):
    """HGB_SERIAL=1: the same batches call by call through kb_consensus, its pass-2 median
    and both of its sorts (the 6,115-key bucket at N = 32 goes through sort_keys_g)."""
    monkeypatch.setenv("HGB_SERIAL", "1")
    b, graphs, tot = _batch(n)
    try:
        assert b.fallbacks() == len(graphs)
        assert tot == sum(len(oracle_case(c, k)[2]["order"]) for c, k in graphs)
        _check_states(b, graphs)
    finally:
        b.close()


@pytest.mark.parametrize("n", [4, 32])
def test_batch_shapes_delivered(n, monkeypatch):
    """The commit records (ids, counts, rr, cts) delivered inside the run, from the DLV
    instances of kb_sort (bulk) and of kb_consensus (HGB_SERIAL=1)."""
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("HGB_SERIAL", "1")
        b, graphs, _ = _batch(n, deliver=True)
        try:
            assert b.delivered() == 1
            assert b.fallbacks() == (len(graphs) if serial else 0)
            _check_commits(b, graphs)
            _check_states(b, graphs)
        finally:
            b.close()
