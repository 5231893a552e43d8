"""counter_gossip (babble_amd/gossip.py): the counter-based stream family the batch
engine's device front restates (hge_batch_gen.hip).  Its properties, against the live
oracle's admission statuses: a creator never picks itself, the forker set has exactly
min(forkers, N) creators, every honest submission is admitted, every twin is refused with
"Self-parent not last known event", records 1 and 3 of a cascade with "Other-parent not
known" and record 2 with "Self-parent not known", no honest event references a refused one,
the same arguments give the same bytes, and a shorter stream is a prefix of a longer one
(a decision depends on the seed and the step alone).  Then hge_batch_generate's argument
check, which runs before the device is touched.  No GPU needed."""
import itertools

import numpy as np
import pytest

from babble_amd import engine
from babble_amd.gossip import TS_BASE, counter_forkers, counter_gossip, random_gossip, schedule

HGE_ERR_ARG = -8
SP_UNKNOWN, OP_UNKNOWN, SP_NOT_LAST = -2, -4, -5
NS = [1, 2, 3, 5, 32, 64]


def _events(n):
    return sorted({e for e in (n, n + 1, 63, 64, 65, 600) if e >= n})


def _corners(n):
    some = max(1, n // 3)
    return itertools.product(sorted({0, some, n}), (0.05, 1.0), (0.0, 0.5, 1.0), (0, 3))


def _kinds(d):
    """twin, record 1 or 3, record 2 masks, from the stream's own fields."""
    honest = d["honest"]
    off = (d["ts"] - TS_BASE) % 1000
    twin = ~honest & (off == 1)
    rec = ~honest & ~twin
    rec2 = rec & ~honest[np.maximum(d["sp"], 0)]  # its self-parent is record 1
    return twin, rec & ~rec2, rec2


@pytest.mark.parametrize("n", NS)
def test_properties_against_the_oracle(n):
    from oracle.oracle import replay
    seen = dict(twin=0, rec13=0, rec2=0, lagged=0)
    for seed, (events, (fk, fp, cp, lag)) in enumerate(itertools.product(_events(n), _corners(n))):
        d = counter_gossip(n, events, 100 + seed, fk, fp, cp, lag)
        case = (n, events, 100 + seed, fk, fp, cp, lag)
        assert set(d) == set(random_gossip(n, n, 1)), case
        honest, cr, sp, op = d["honest"], d["creator"], d["sp"], d["op"]
        assert honest.sum() == events, case
        h = np.nonzero(honest)[0]
        later = h[n:]
        assert (sp[h[:n]] == -1).all() and (op[h[:n]] == -1).all() and (d["index"][h[:n]] == 0).all(), case
        if n > 1:
            assert (cr[op[later]] != cr[later]).all(), case
        # honest events reference honest events only, and their self-parent is their creator's
        assert honest[sp[later]].all() and honest[op[later]].all(), case
        assert (cr[sp[later]] == cr[later]).all(), case
        twin, rec13, rec2 = _kinds(d)
        fset = counter_forkers(n, 100 + seed, fk)
        assert len(fset) == min(fk, n), case
        assert set(cr[twin].tolist()) <= fset, case
        if fp == 1.0:  # every later step of a forker forks, nobody else's does
            assert twin.sum() == np.isin(cr[later], sorted(fset)).sum(), case
            if cp == 1.0 and n > 1:
                assert rec13.sum() >= twin.sum(), case
        if cp == 0.0:
            assert not rec13.any() and not rec2.any(), case
        _, status, _, _ = replay(d, schedule(len(cr), max(1, len(cr))))
        assert (status[honest] >= 0).all(), case
        assert (status[honest] == np.arange(events)).all(), case
        assert (status[twin] == SP_NOT_LAST).all(), case
        assert (status[rec13] == OP_UNKNOWN).all(), case
        assert (status[rec2] == SP_UNKNOWN).all(), case
        # the twin repeats its honest event; a lagged other-parent is not its chain's head
        tw = np.nonzero(twin)[0]
        for key in ("creator", "index", "sp", "op"):
            assert (d[key][tw] == d[key][tw - 1]).all(), case
        assert (d["ts"][tw] == d["ts"][tw - 1] + 1).all() and honest[tw - 1].all(), case
        seen["twin"] += int(twin.sum())
        seen["rec13"] += int(rec13.sum())
        seen["rec2"] += int(rec2.sum())
        if lag:
            heads = {}
            for i in h:
                if op[i] >= 0 and heads.get(cr[op[i]]) != op[i]:
                    seen["lagged"] += 1
                heads[cr[i]] = i
    assert seen["twin"] > 0
    if n > 1:
        assert seen["rec13"] > 0 and seen["rec2"] > 0 and seen["lagged"] > 0, seen


@pytest.mark.parametrize("n", NS)
def test_same_arguments_same_bytes_and_prefixes(n):
    some = max(1, n // 3)
    a = counter_gossip(n, 600, 9, some, 0.3, 0.5, 3)
    b = counter_gossip(n, 600, 9, some, 0.3, 0.5, 3)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    other = counter_gossip(n, 600, 10, some, 0.3, 0.5, 3)
    assert other["S"].tobytes() != a["S"].tobytes()
    short = counter_gossip(n, 65, 9, some, 0.3, 0.5, 3)
    # the longer stream's submissions up to honest event 65's step are the shorter stream
    cut = len(short["creator"])
    assert np.nonzero(a["honest"])[0][64] < cut <= np.nonzero(a["honest"])[0][65]
    for k in short:
        assert np.array_equal(np.asarray(a[k])[:cut] if k != "n" else a[k], short[k]), k


def test_generate_argument_check():
    ok = dict(n_participants=4, graphs=2, events=100, k=4, forkers=1, fork_p=0.5, cascade_p=1.0, op_lag=3)
    assert engine.gossip_params_check(**ok) == 0
    assert engine.gossip_params_check(**dict(ok, events=4, fork_p=0.0, cascade_p=0.0, op_lag=16)) == 0
    bad = [dict(events=3), dict(graphs=0), dict(graphs=-1), dict(fork_p=-0.1), dict(fork_p=1.5),
           dict(cascade_p=1.0001), dict(cascade_p=float("nan")), dict(forkers=-1), dict(k=0), dict(op_lag=-1),
           dict(op_lag=1 << 20), dict(n_participants=0), dict(n_participants=65), dict(events=1 << 40)]
    for change in bad:
        assert engine.gossip_params_check(**dict(ok, **change)) == HGE_ERR_ARG, change
    assert engine.lib().hge_gossip_params_check(4, None, 1) == HGE_ERR_ARG
    # a null handle is refused before anything else
    assert engine.lib().hge_batch_generate(None, None, 1, 0) == HGE_ERR_ARG
    assert engine.lib().hge_batch_clear(None) == HGE_ERR_ARG
    assert engine.lib().hge_batch_submissions(None, 0, None, None, 0) == HGE_ERR_ARG
