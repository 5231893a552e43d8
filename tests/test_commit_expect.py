"""The streams of tests/commit_expect.py prove what tests/test_gpu_commit_records.py uses
them for, asserted from the oracle alone: every case orders something, has records with
more than one candidate at the median instant, and has records where "the middle of the
candidates sorted by (timestamp, creator)" is another event than "the lowest creator at
that instant" -- so a kernel with the wrong tie rule fails on them.

The figures are the oracle's, measured on the CPU over the whole log (at N = 64 the first
~600 entries are received in round 1 with a single famous witness: a prefix shows nothing).
Case I exists for the int32 chain positions, not for ties: its `spread` timestamps are
distinct, and only its order and chain length are asserted."""
import numpy as np
import pytest

from commit_expect import CASES, expected, stream

# case -> ordered, records with > 1 candidate at the instant, records where the wrong tie rule
# differs, least number of distinct rounds received
FIGURES = {
    "A": (1176, 1121, 1094, 3),
    "B": (1385, 1165, 757, 3),
    "C": (2684, 2565, 2478, 2),
    "D": (2320, 1990, 1899, 2),
    "E": (863, 863, 804, 2),
    "F": (3226, 2548, 2459, 4),
    "G": (4453, 4453, 4263, 3),
    "H": (5891, 5891, 5535, 2),
}


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_case_proves_the_tie_rule(name):
    ordered, multi, wrong, rounds = FIGURES[name]
    e = expected(name)
    got = (len(e["ids"]), int(e["multi"].sum()), int(e["wrong"].sum()), len(set(e["rr"].tolist())))
    print(name, "ordered, multi, wrong, rounds received:", got, "non-empty calls:", int((e["counts"] > 0).sum()))
    assert got[0] == ordered
    assert got[0] == int(e["counts"].sum())
    assert got[1] > 0 and got[2] > 0
    assert got[1] == multi and got[2] == wrong
    assert got[3] >= rounds
    # a record's source carries the consensus timestamp and every record has one
    assert (e["src"] >= 0).all() and (e["rr"] >= 0).all()


def test_prefix_figures():
    """The first 600 records of the small cases (the figures the cases were chosen by)."""
    for name, multi, wrong in (("A", 576, 563), ("B", 421, 267), ("D", 600, 576), ("E", 600, 555)):
        e = expected(name)
        got = (int(e["multi"][:600].sum()), int(e["wrong"][:600].sum()))
        print(name, "first 600: multi, wrong:", got)
        assert got == (multi, wrong), name
    assert int((expected("A")["counts"] > 0).sum()) == 82
    assert int((expected("C")["counts"] > 0).sum()) == 18
    assert sorted(set(expected("F")["rr"].tolist())) == [1, 3, 4, 5]
    assert sorted(set(expected("G")["rr"].tolist())) == [1, 2, 3]
    assert sorted(set(expected("H")["rr"].tolist())) == [1, 2]


def test_forked_case_maps_submissions_to_ids():
    """Case D refuses submissions: ids are engine ids, below the accepted count."""
    e = expected("D")
    acc = int((e["status"] >= 0).sum())
    assert acc < len(e["status"])
    assert e["ids"].max() < acc and e["src"].max() < acc


def test_case_i_crosses_the_chain_limit():
    dag, _ = stream("I")
    assert np.bincount(np.asarray(dag["creator"]), minlength=CASES["I"][0]).max() == 69
    e = expected("I")
    assert len(e["ids"]) == 607


def test_second_shape_and_second_stream_at_64():
    for name in ("F31", "E64"):
        e = expected(name)
        print(name, len(e["ids"]), int(e["multi"].sum()), int(e["wrong"].sum()))
        assert len(e["ids"]) > 0 and e["multi"].sum() > 0 and e["wrong"].sum() > 0
    e = expected("E64")
    assert (len(e["ids"]), sorted(set(e["rr"].tolist()))) == (1759, [1, 2])
    assert len(e["ids"]) < len(expected("F")["ids"]) and len(e["status"]) < len(expected("F")["status"])
