"""hge_commit_records, hge_find_order_records, hge_run_consensus_records: FindOrder's commit
records (id, round received, consensus timestamp, MedianTimestamp's source;
hashgraph.go:723-770) read from persisted state, against the records a live oracle gives
(tests/commit_expect.py; tests/test_commit_expect.py asserts what its streams prove).

The cases cover every table form the one kernel reads through la_at / fd_at: int32 LA/FD
(A to D, N <= 32), LA16 with int32 FD (E, F, N = 33 and 64), LA16 with FD16 (G, H, fresh bulk
replays at N > 128 whose median came from the FD rows: the timestamp offset table is stale
there, so a kernel that reads it fails) and the int32 positions past the chain limit (I)."""
import numpy as np
import pytest

from commit_expect import CASES, assert_records, expected, stream

pytestmark = pytest.mark.gpu

HGE_ERR_ARG = -8


def engine_for(name, n=None):
    from babble_amd.engine import Engine
    dag, _ = stream(name)
    return Engine(n or CASES[name][0], len(dag["creator"]) + 64)


def replayed(eng, name):
    dag, calls = stream(name)
    exp = expected(name)
    st, order, counts = eng.replay(dag, calls)
    np.testing.assert_array_equal(st, exp["status"])
    np.testing.assert_array_equal(order, exp["ids"])
    np.testing.assert_array_equal(counts, exp["counts"])
    return exp


def online(eng, ev, calls, first=0, records=True):
    """InsertEvent + RunConsensus at every call point past `first`; the calls' records (or
    their plain orders) and the host waits each consensus call took."""
    out, waits, nxt = [], [], first
    for c in calls:
        if c <= first:
            continue
        eng.insert_events(ev[nxt:c].copy())
        w0 = eng.host_syncs()
        out.append(eng.run_consensus_records() if records else eng.run_consensus())
        waits.append(eng.host_syncs() - w0)
        nxt = int(c)
    return out, waits


def joined(recs):
    cat = lambda k: np.concatenate([r[k] for r in recs]) if recs else np.zeros(0)
    return dict(ids=cat("ids"), rr=cat("rr"), cts=cat("cts"), src=cat("src"))


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F", "F31", "G", "H"])
def test_replay_every_table_form(name):
    eng = engine_for(name)
    try:
        exp = replayed(eng, name)
        assert_records(eng.commit_records(), exp)
        assert_records(eng.commit_records(sources=False), exp, sources=False)
        # the read changes nothing: again, after the log moved into its vector
        np.testing.assert_array_equal(eng.consensus_log(), exp["ids"])
        assert_records(eng.commit_records(), exp)
    finally:
        eng.close()


def test_int32_positions(monkeypatch):
    from babble_amd.engine import Engine
    monkeypatch.setenv("HGE_CHAIN_LIMIT", "40")  # read at create
    dag, _ = stream("I")
    eng = Engine(CASES["I"][0], len(dag["creator"]) + 64)
    try:
        exp = replayed(eng, "I")
        assert_records(eng.commit_records(), exp)
        assert_records(eng.commit_records(sources=False), exp, sources=False)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["A", "C", "F"])
def test_online_calls(name):
    from babble_amd.engine import events_array
    dag, calls = stream(name)
    exp = expected(name)
    assert (exp["status"] == np.arange(len(exp["status"]))).all()  # no forks: id = submission
    eng = engine_for(name)
    try:
        recs, _ = online(eng, events_array(dag), calls)
        np.testing.assert_array_equal([len(r["ids"]) for r in recs], exp["counts"])
        lo = 0
        for r in recs:
            assert_records(r, exp, lo, lo + len(r["ids"]))
            lo += len(r["ids"])
        assert lo == len(exp["ids"])
        assert_records(joined(recs), exp)
        assert_records(eng.commit_records(), exp)
    finally:
        eng.close()


def test_find_order_records_after_the_stages():
    from babble_amd.engine import events_array
    dag, calls = stream("A")
    exp = expected("A")
    ev = events_array(dag)
    eng = engine_for("A")
    try:
        recs, nxt = [], 0
        for c in calls:
            eng.insert_events(ev[nxt:c].copy())
            eng.divide_rounds()
            eng.decide_fame()
            recs.append(eng.find_order_records())
            nxt = int(c)
        np.testing.assert_array_equal([len(r["ids"]) for r in recs], exp["counts"])
        assert_records(joined(recs), exp)
        assert_records(eng.commit_records(), exp)
    finally:
        eng.close()


def test_replay_then_online():
    from babble_amd.engine import events_array
    dag, calls = stream("F")
    exp = expected("F")
    ev = events_array(dag)
    first = 3000
    nrep = int((calls <= first).sum())
    join = int(exp["counts"][:nrep].sum())
    assert 0 < join < len(exp["ids"])
    eng = engine_for("F")
    try:
        _, order, _ = eng.replay(ev[:first], calls[:nrep])
        np.testing.assert_array_equal(order, exp["ids"][:join])
        # the log's tail still where the replay delivered it
        assert_records(eng.commit_records(), exp, 0, join)
        assert_records(eng.commit_records(join - 5, join), exp, join - 5, join)
        recs, _ = online(eng, ev, calls, first=first)
        assert_records(joined(recs), exp, join)
        assert_records(eng.commit_records(), exp)
        assert_records(eng.commit_records(join - 40, join + 40), exp, join - 40, join + 40)
        assert_records(eng.commit_records(join, join + 1), exp, join, join + 1)
    finally:
        eng.close()


def test_ranges_and_arguments():
    from babble_amd.engine import Engine, HgeError
    eng = engine_for("D")
    try:
        empty = eng.commit_records()  # no consensus yet
        assert all(len(empty[k]) == 0 for k in ("ids", "rr", "cts", "src"))
        assert eng.L.hge_commit_records(eng.h, 0, 10, None, None, None, None) == 0
        exp = replayed(eng, "D")
        m = len(exp["ids"])
        rng = np.random.default_rng(5)
        for lo, hi in [(0, 1), (m - 1, m), (1, 64), (63, 65), (m - 7, m + 100)] + \
                [tuple(sorted(rng.integers(0, m, 2).tolist())) for _ in range(8)]:
            assert_records(eng.commit_records(lo, hi), exp, lo, min(hi, m))
            assert_records(eng.commit_records(lo, hi, sources=False), exp, lo, min(hi, m), sources=False)
        for start in (m, m + 1, 10 * m):  # at or past the end: 0, nothing written
            got = eng.commit_records(start)
            assert all(len(got[k]) == 0 for k in ("ids", "rr", "cts", "src"))
            assert eng.L.hge_commit_records(eng.h, start, 4, None, None, None, None) == 0
        # cap 0: the entries left, nothing written
        canary = np.full(4, -77, np.int32)
        p = canary.ctypes.data_as(eng.L.hge_commit_records.argtypes[3])
        assert eng.L.hge_commit_records(eng.h, 3, 0, p, p, None, p) == m - 3
        assert (canary == -77).all()
        got = eng.commit_records(3, 3)
        assert all(len(got[k]) == 0 for k in ("ids", "rr", "cts", "src"))
        # any output may be missing
        one = np.zeros(5, np.int32)
        assert eng.L.hge_commit_records(eng.h, 10, 5, None, one.ctypes.data_as(eng.L.hge_commit_records.argtypes[4]),
                                        None, None) == m - 10
        np.testing.assert_array_equal(one, exp["rr"][10:15])
        assert eng.L.hge_commit_records(eng.h, 10, 5, None, None, None,
                                        one.ctypes.data_as(eng.L.hge_commit_records.argtypes[6])) == m - 10
        np.testing.assert_array_equal(one, exp["src"][10:15])
        with pytest.raises(HgeError) as e:
            eng.commit_records(-1)
        assert e.value.code == HGE_ERR_ARG
        assert eng.L.hge_commit_records(eng.h, 0, -1, None, None, None, None) == HGE_ERR_ARG
        assert eng.L.hge_commit_records(None, 0, 1, None, None, None, None) == HGE_ERR_ARG
        assert_records(eng.commit_records(), exp)  # (a refused call leaves the engine usable)
    finally:
        eng.close()


@pytest.mark.parametrize("chunk", [100, 1])
def test_chunks(monkeypatch, chunk):
    eng = engine_for("F")
    try:
        exp = replayed(eng, "F")
        whole = eng.commit_records()
        w0 = eng.host_syncs()
        monkeypatch.setenv("HGE_TEST_RECORDS_CHUNK", str(chunk))  # read per use
        got = eng.commit_records()
        nchunks = -(-len(exp["ids"]) // chunk)
        assert eng.host_syncs() - w0 >= nchunks  # the chunked path ran
        for k in ("ids", "rr", "cts", "src"):
            np.testing.assert_array_equal(got[k], whole[k], err_msg=k)
        assert_records(got, exp)
        assert_records(eng.commit_records(sources=False), exp, sources=False)
        assert_records(eng.commit_records(150, 450), exp, 150, 450)
    finally:
        eng.close()


def test_reuse_shows_no_stale_state():
    eng = engine_for("F")
    try:
        first = replayed(eng, "F")
        assert_records(eng.commit_records(), first)
        eng.reset()
        assert len(eng.commit_records()["ids"]) == 0
        from babble_amd.engine import events_array
        dag, calls = stream("E64")
        exp = expected("E64")
        recs, _ = online(eng, events_array(dag), calls)
        assert_records(joined(recs), exp)
        assert_records(eng.commit_records(), exp)
        # and a replay of it over the same engine
        again = replayed(eng, "E64")
        assert_records(eng.commit_records(), again)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["C", "F"])
def test_host_waits(name):
    """A records call costs at most one host wait more than its plain twin: two engines fed
    the same stream, the first call a warm-up, every window of 10 calls after it."""
    from babble_amd.engine import events_array
    dag, calls = stream(name)
    ev = events_array(dag)
    a, b = engine_for(name), engine_for(name)
    try:
        plain, wp = online(a, ev, calls, records=False)
        recs, wr = online(b, ev, calls)
        np.testing.assert_array_equal(np.concatenate(plain), joined(recs)["ids"])
        wp, wr = np.asarray(wp[1:]), np.asarray(wr[1:])
        busy = np.asarray([len(r["ids"]) > 0 for r in recs[1:]])
        print(name, "host waits per call: plain", wp.sum(), "records", wr.sum(), "calls", len(wp),
              "max per-call difference", int((wr - wp).max()), "on calls that ordered", int((wr - wp)[busy].max()))
        assert busy.sum() > 0
        for lo in range(0, len(wp) - 9):
            assert wr[lo:lo + 10].sum() <= wp[lo:lo + 10].sum() + 10, lo
    finally:
        a.close()
        b.close()


def test_order_view():
    from babble_amd.engine import events_array
    dag, calls = stream("F")
    exp = expected("F")
    ev = events_array(dag)
    first = 3000
    nrep = int((calls <= first).sum())
    eng = engine_for("F")
    _, order, _ = eng.replay(ev[:first], calls[:nrep])
    v = eng.order_view()
    np.testing.assert_array_equal(v, order)
    np.testing.assert_array_equal(v, eng.commit_records()["ids"])
    assert not v.flags.writeable
    recs, _ = online(eng, ev, calls[:nrep + 12], first=first, records=False)
    assert sum(len(r) for r in recs) > 0
    v = eng.order_view()
    np.testing.assert_array_equal(v, exp["ids"][:len(v)])
    assert len(v) == len(order) + sum(len(r) for r in recs)
    np.testing.assert_array_equal(v, eng.commit_records()["ids"])
    # the view keeps the engine alive: dropping the last other reference frees nothing
    import gc
    import weakref
    alive = weakref.ref(eng)
    del eng
    gc.collect()
    assert alive() is not None
    np.testing.assert_array_equal(v, exp["ids"][:len(v)])
    del v
    gc.collect()
    assert alive() is None
