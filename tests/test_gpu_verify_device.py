"""Event.Verify on the device (hge_verify.hip: k_sha256_bodies, k_p256_key_tables,
k_ecdsa_p256_verify over the arithmetic of hge_p256.h) against hashlib, the host pipeline
(hge_verify_events, OpenSSL) and the pure-Python restatement of ecdsa.Verify
(oracle/p256.py); and hge_ingest_device against the oracle's replay and hge_ingest.
Every comparison is exact."""
import hashlib

import numpy as np
import pytest

from babble_amd import engine, signing
from babble_amd.engine import Engine, events_array
from babble_amd.gossip import random_gossip
from oracle import p256
from oracle.oracle import replay as oracle_replay

pytestmark = pytest.mark.gpu


# ---- SHA-256 ------------------------------------------------------------------------------
def test_sha256_matches_hashlib():
    rng = np.random.default_rng(17)
    lens = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 161, 300] + [int(x) for x in rng.integers(0, 400, 500)]
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    out = engine.sha256_batch_device(data)
    assert out.shape == (len(data), 32)
    for d, h in zip(data, out):
        assert bytes(h) == hashlib.sha256(d).digest(), len(d)


# ---- every way Event.Verify fails ------------------------------------------------------------
def _oracle_signed(n, seed):
    """n events signed by oracle/p256.py with 4 keys (tests/test_ingest.py's stream)."""
    rng = np.random.default_rng(seed)
    ds = [int.from_bytes(rng.bytes(32), "big") % (p256.N - 1) + 1 for _ in range(4)]
    pubs = [p256.public_key(d) for d in ds]
    bodies, P, S = [], [], []
    for i in range(n):
        body = rng.bytes(int(rng.integers(40, 300)))
        c = i % 4
        k = int.from_bytes(rng.bytes(32), "big") % (p256.N - 1) + 1
        r, s = p256.sign(ds[c], hashlib.sha256(body).digest(), k)
        bodies.append(body)
        P.append(np.frombuffer(pubs[c], np.uint8))
        S.append(np.frombuffer(r.to_bytes(32, "big") + s.to_bytes(32, "big"), np.uint8))
    return bodies, np.array(P), np.array(S)


def test_every_failure_of_event_verify():
    """tests/test_ingest.py::test_every_failure_of_event_verify's events and failures, with
    s = 0, r = n, X = p and the all-zero key added."""
    bodies, pubs, sigs = _oracle_signed(12, seed=3)
    bodies = list(bodies)
    pubs, sigs = pubs.copy(), sigs.copy()
    nb = np.frombuffer(p256.N.to_bytes(32, "big"), np.uint8)
    bad = {}
    bodies[1] = bodies[1][:-1] + bytes([bodies[1][-1] ^ 1]); bad[1] = "body"
    sigs[2, 31] ^= 1; bad[2] = "r"
    sigs[3, 63] ^= 1; bad[3] = "s"
    sigs[4, :32] = 0; bad[4] = "r = 0"
    sigs[5, 32:] = nb; bad[5] = "s = n"
    pubs[6, 64] ^= 1; bad[6] = "key off the curve"
    pubs[7, 0] = 2; bad[7] = "compressed key prefix"
    pubs[8] = pubs[9]; bad[8] = "another creator's key"
    sigs[0, 32:] = 0; bad[0] = "s = 0"
    sigs[10, :32] = nb; bad[10] = "r = n"
    pubs[11, 1:33] = np.frombuffer(p256.P.to_bytes(32, "big"), np.uint8); bad[11] = "X = p"
    pubs[9, 1:] = 0; bad[9] = "the all-zero key"
    # one key per event: the key table is the events' keys
    ok, hashes, ms = engine.verify_events_device(bodies, pubs, np.arange(12, dtype=np.int32), sigs)
    hok, hhashes = engine.verify_events(bodies, pubs, sigs, threads=3)
    assert np.array_equal(hashes, hhashes)
    for i in range(12):
        assert bytes(hashes[i]) == hashlib.sha256(bodies[i]).digest()
        assert bool(ok[i]) == bool(hok[i]), (i, bad.get(i))
        assert bool(ok[i]) == p256.verify_event(bodies[i], pubs[i], sigs[i]), (i, bad.get(i))
    assert not ok.any()  # every one of the twelve now carries a failure
    assert ms > 0
    # and the untouched events all verify
    bodies, pubs, sigs = _oracle_signed(12, seed=3)
    ok, _, _ = engine.verify_events_device(bodies, pubs, np.arange(12, dtype=np.int32), sigs)
    assert ok.all()


# ---- digest-level cases: where the point arithmetic can go wrong ------------------------------
def _b32(x):
    return np.frombuffer(int(x).to_bytes(32, "big"), np.uint8)


def test_digest_level_cases():
    rng = np.random.default_rng(23)

    def scalar():
        return int.from_bytes(rng.bytes(32), "big") % (p256.N - 1) + 1

    d = scalar()
    key_d = p256.public_key(d)
    key_g = p256.public_key(1)
    key_ng = b"\x04" + p256.GX.to_bytes(32, "big") + ((-p256.GY) % p256.P).to_bytes(32, "big")
    keys = np.array([np.frombuffer(k, np.uint8) for k in (key_d, key_g, key_ng)])
    digests, idx, sigs, want, what = [], [], [], [], []

    def case(digest, ki, r, s, expect, name):
        digests.append(np.frombuffer(bytes(digest), np.uint8))
        idx.append(ki)
        sigs.append(np.concatenate([_b32(r), _b32(s)]))
        want.append(expect)
        what.append(name)

    zero = bytes(32)
    for _ in range(3):
        r, s = p256.sign(d, zero, scalar())
        case(zero, 0, r, s, True, "digest 0 (u1 = 0)")
        case(zero, 0, r, (s + 1) % p256.N or 1, False, "digest 0, s changed")
        dg = rng.bytes(32)
        r, s = p256.sign(d, dg, scalar())
        case(dg, 0, r, s, True, "plain")
        case(dg, 1, r, s, False, "plain under G")
        # e = r under Q = G: s = 2 r / k gives u1 = u2, the ladder adds a multiple of G to itself
        k = scalar()
        r = p256._affine(p256._mul(k, p256.GX, p256.GY))[0] % p256.N
        s = 2 * r * pow(k, p256.N - 2, p256.N) % p256.N
        case(r.to_bytes(32, "big"), 1, r, s, True, "Q = G, e = r")
        # the same under Q = -G: u1 G + u2 Q is infinity
        case(r.to_bytes(32, "big"), 2, r, s, False, "Q = -G, e = r")
        case(r.to_bytes(32, "big"), 2, r, scalar(), False, "Q = -G, e = r, any s")
    digest_ones = b"\xff" * 32  # e >= n: reduced, not refused
    r, s = p256.sign(d, digest_ones, scalar())
    case(digest_ones, 0, r, s, True, "digest above n")
    ok = engine.verify_digests_device(np.array(digests), keys, np.array(idx, np.int32), np.array(sigs))
    for i in range(len(want)):
        ref = p256.verify(keys[idx[i]].tobytes(), digests[i].tobytes(), int.from_bytes(sigs[i][:32].tobytes(), "big"),
                          int.from_bytes(sigs[i][32:].tobytes(), "big"))
        assert ref == want[i], (i, what[i])
        assert bool(ok[i]) == ref, (i, what[i])


# ---- shapes: partial waves, more than one workgroup, the key-table indexing -------------------
@pytest.fixture(scope="module")
def stream4():
    dag = random_gossip(4, 257, seed=5)
    pubs, (flat, off), sigs = signing.signed_stream(dag, seed=9, threads=4)
    return dag["creator"].astype(np.int32), pubs, flat, off, sigs


def _check_shape(cre, pubs, flat, off, sigs, n, flip):
    bodies = (flat[:off[n]] if off[n] else np.zeros(1, np.uint8), off[:n + 1])
    sigs = sigs[:n].copy()
    sigs[flip, 37] ^= 0x04
    ok, hashes, _ = engine.verify_events_device(bodies, pubs, cre[:n], sigs)
    hok, hhashes = engine.verify_events(bodies, pubs[cre[:n]], sigs, threads=4)
    assert np.array_equal(hashes, hhashes)
    assert np.array_equal(ok, hok)
    want = np.ones(n, bool)
    want[flip] = False
    assert np.array_equal(ok, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_shapes_four_keys(stream4, n):
    cre, pubs, flat, off, sigs = stream4
    _check_shape(cre, pubs, flat, off, sigs, n, flip=n // 2)


def test_thousand_events_256_keys():
    dag = random_gossip(256, 1000, seed=8)
    pubs, (flat, off), sigs = signing.signed_stream(dag, seed=6, threads=4)
    cre = dag["creator"].astype(np.int32)
    assert len(np.unique(cre)) > 200
    _check_shape(cre, pubs, flat, off, sigs, 1000, flip=999)
    # the digests path over the same keys: the hashes from the host, the verdicts the same
    sg = sigs.copy()
    sg[501, 3] ^= 0x80
    hashes = engine.sha256_batch((flat, off), threads=4)
    ok = engine.verify_digests_device(hashes, pubs, cre, sg)
    want = np.ones(1000, bool)
    want[501] = False
    assert np.array_equal(ok, want)


# ---- hge_ingest_device ------------------------------------------------------------------------------
def _calls(n, k):
    pts = list(range(k, n + 1, k))
    if not pts or pts[-1] != n:
        pts.append(n)
    return np.array(pts, np.int64)


@pytest.mark.parametrize("n,E,k", [(16, 3000, 16), (64, 6000, 64)])
def test_ingest_device_matches_oracle_and_host_ingest(n, E, k):
    dag = random_gossip(n, E, seed=4)
    pubs, bodies, sigs = signing.signed_stream(dag, seed=2, threads=8)
    ev = events_array(dag)
    eng = Engine(n, E)
    rc, status, acc, tm = eng.ingest_device(ev, bodies, pubs, sigs, k, verify_block=1024)  # several blocks
    assert rc == 0 and acc == E
    assert np.array_equal(status, np.arange(E))
    order = eng.consensus_log()
    eng.close()
    _, _, oorder, _ = oracle_replay(dag, _calls(E, k))
    assert np.array_equal(order, oorder)
    assert tm["verify_ms"] > 0 and tm["wall_ms"] >= tm["verify_ms"]
    host = Engine(n, E)
    hrc, hstatus, hacc, _ = host.ingest(ev, bodies, pubs, sigs, k, threads=4)
    assert (hrc, hacc) == (rc, acc)
    assert np.array_equal(hstatus, status)
    assert np.array_equal(host.consensus_log(), order)
    host.close()


def test_ingest_device_stops_at_bad_signature():
    n, E, k, bad = 16, 2400, 16, 1203  # mid-batch, mid-block
    dag = random_gossip(n, E, seed=6)
    pubs, bodies, sigs = signing.signed_stream(dag, seed=3, threads=8)
    sigs = sigs.copy()
    sigs[bad, 40] ^= 0x10
    eng = Engine(n, E)
    rc, status, acc, _ = eng.ingest_device(events_array(dag), bodies, pubs, sigs, k, verify_block=1024)
    assert rc == -13 and acc == bad and status[bad] == -13
    assert eng.event_count() == bad
    pre = {key: (v[:bad] if isinstance(v, np.ndarray) else v) for key, v in dag.items()}
    _, _, oorder, _ = oracle_replay(pre, _calls(bad, k))
    assert np.array_equal(eng.consensus_log(), oorder)
    eng.close()


def test_ingest_device_refuses_body_signed_by_another_creator():
    n, E, k, bad = 16, 1600, 16, 777
    dag = random_gossip(n, E, seed=7)
    pubs, bodies, sigs = signing.signed_stream(dag, seed=4, threads=8)
    c = int(dag["creator"][bad])
    other = int(np.nonzero(dag["creator"] != c)[0][-1])
    flat, off = bodies
    flat = flat.copy()
    flat[off[bad]:off[bad + 1]] = flat[off[other]:off[other + 1]]
    sigs = sigs.copy()
    sigs[bad] = sigs[other]
    eng = Engine(n, E)
    rc, status, acc, _ = eng.ingest_device(events_array(dag), (flat, off), pubs, sigs, k)
    assert rc == -13 and acc == bad and status[bad] == -13
    eng.close()
