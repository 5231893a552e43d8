"""The streams of tests/batch_variants.py reach what tests/test_gpu_batch_variants.py
relies on, from the oracle and the bulk model alone (CPU): call buckets of the first
sort class (and of the second where a stream's K fills it) that kb_sort cannot pack,
keys that tie past S's first limb, DecideFame pairs at s = 2 (decided inline by
kb_fold<NM, 2>, from kb_pairs' window by kb_fold<NM, 3>) and past every window, a graph
past the bulk fold's 256 rounds, coin-bit votes.  A pass of the GPU tests on these
streams then means that the instances the batch's size selects went through those
branches.

Pairs past NS = 3's window (s >= 3) exist at the widths 16, 17, 22, 23, 32 and 33; no
stream of width 5 or 64 here has one (their calls follow the rounds too closely), so that
condition is stated for those six widths.  s = 2 pairs exist at every width."""
import numpy as np
import pytest

from batch_variants import BASE, COIN_VOTE, EXTRA, FILLS_4096, K3, KINDS, ONE_CALL_32, PAST_FOLD, WIDTHS, distinct, oracle

CASE_ID = lambda c: "-".join(str(v) for v in c)
ALL_BASE = [c for n in WIDTHS for c in BASE[n]]
WIDE_WINDOW = (16, 17, 22, 23, 32, 33)  # widths with a DecideFame pair past NS = 3's window


def test_widths_sit_on_every_flip_of_kb_front():
    """kb_front<NM, NT> gives each thread one (member, chain) pair while N * N <= NT."""
    for nt in (1024, 512, 256):
        lo = max(n for n in range(1, 65) if n * n <= nt)
        assert lo in WIDTHS and lo + 1 in WIDTHS, nt
    assert min(WIDTHS) < 16 and max(WIDTHS) == 64
    for n in WIDTHS:
        ds = distinct(n)
        assert len(set(ds)) == len(ds) == 7 * len(BASE[n]) + len(EXTRA.get(n, []))
        assert all(c[0] == n for c, _ in ds)
    assert set(FILLS_4096) <= set(ALL_BASE)


@pytest.mark.parametrize("case", ALL_BASE, ids=CASE_ID)
@pytest.mark.parametrize("kind", KINDS)
def test_base_stream_reaches_the_sort_branches(case, kind):
    dag, calls, st, r = oracle((case, kind))
    # (the bound of test_ts_shapes.py: wide graphs with lagging other-parents order a third of their events)
    assert len(st["order"]) > 500 and st["scalars"][1] >= 1, (case, kind, len(st["order"]), st["scalars"])
    if case[2] >= 600:  # buckets of the first class past one wave's 64 lanes (kb_sort's strides above 64)
        assert any(64 < c <= 1024 for c in st["counts"].tolist()), (case, kind, st["counts"])
    if kind in ("two28", "two31m", "two31", "spread"):
        assert r["to1024"]["unpacked"] > 0, (case, kind, r)
        if case in FILLS_4096:
            assert r["to4096"]["unpacked"] > 0, (case, kind, r)
    if kind == "ties":
        assert r["to1024"]["tie0"] > 0 and r["to1024"]["tie2"] > 0, (case, kind, r)
    assert r["rr_span_max"] < 16  # (kb_sort's other packing condition is not reached)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_has_inline_pairs(n):
    """DecideFame pairs outside kb_pairs' window, per width: more with two slots than with
    three (pairs at s = 2 exist), and at WIDE_WINDOW's widths some past three as well."""
    from bulk_model import bulk_replay
    miss = {2: 0, 3: 0}
    for case in BASE[n]:
        dag, calls, st, _ = oracle((case, "gaps"))  # (fame does not read timestamps)
        for ns in miss:
            got = bulk_replay(dag, calls, st["status"], st["rounds"], st["witness"], NS=ns)
            np.testing.assert_array_equal(got["order"], st["order"])
            miss[ns] += got["stats"]["misses"]
    print(f"N = {n}: misses NS=2 {miss[2]}, NS=3 {miss[3]}")
    assert miss[2] > miss[3], (n, miss)
    if n in WIDE_WINDOW:
        assert miss[3] > 0, (n, miss)


def test_additions_reach_their_branches():
    dag, calls, st, stats = oracle((PAST_FOLD, None))
    assert st["scalars"][0] > 256, st["scalars"]  # Rounds(): past the bulk fold
    assert st["scalars"][:2].tolist() == [273, 270]
    assert len(calls) > 1
    assert oracle((COIN_VOTE, None))[3]["coin_votes"] > 0
    assert len(oracle((COIN_VOTE, None))[1]) == 1
    assert len(oracle((K3, None))[2]["order"]) > 1500
    r = oracle((ONE_CALL_32, "spread"))[3]
    assert r["past4096"]["buckets"] > 0 and r["past4096"]["unpacked"] > 0, r
