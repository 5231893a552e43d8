"""Witness tables for tests/abi/hge_fame_kernel_test.hip's --tables mode, built from a
live oracle run (plain mode: See and StronglySee are asked pair by pair), and that
program's output parsed.  Shared by test_fame_kernel_host.py and test_gpu_fame_kernel.py."""
import os
import subprocess

import numpy as np

from babble_amd.gossip import random_gossip
from oracle.oracle import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "hge_fame_kernel_test")

# the one-shot streams whose DecideFame takes coin-bit votes (hashgraph.go:647):
# n, events, seed, op_lag
COIN_VOTE_STREAMS = [(8, 2400, 5, 3), (5, 1500, 12, 3), (5, 10500, 4, 40)]

# the synthetic cases of the program (its kBlkN / kItemN), its pairs per case and the
# launch forms that compare every slot of the decision table: full + two parts, and the
# pair list for the block kernel
BLK_N = (64, 128, 192, 256)
ITEM_N = (5, 16, 33, 63, 65, 96, 130, 200, 255)
PAIRS = 4 + 2 + 7 + 6


def compared_slots_floor():
    return PAIRS * (4 * sum(BLK_N) + 3 * sum(ITEM_N))


def oracle_tables(n, events, seed, op_lag):
    """One call over the whole stream: (oracle, the table file's bytes)."""
    dag = random_gossip(n, events, seed=seed, op_lag=op_lag)
    E = len(dag["creator"])
    o, status, _, _ = replay(dag, [E])
    acc = status >= 0
    creator = np.asarray(dag["creator"])[acc]
    R, nw = o.rounds(), (n + 63) // 64
    W = np.full((R, n), -1, np.int32)
    seeb = np.zeros((R, n, nw), np.uint64)
    ssb = np.zeros((R, n, nw), np.uint64)
    prev = []
    for r in range(R):
        wits = o.round_witnesses(r)
        for y in wits:
            d = int(creator[y])
            W[r, d] = y
            for x in prev:
                s = int(creator[x])
                if o.see(y, x):
                    seeb[r, d, s >> 6] |= np.uint64(1 << (s & 63))
                if o.strongly_see(y, x):
                    ssb[r, d, s >> 6] |= np.uint64(1 << (s & 63))
        prev = wits
    coin = (np.asarray(dag["hash"])[acc][:, 16] != 0).astype(np.uint8)  # middleBit, hashgraph.go:781-790
    ids = int(acc.sum())
    blob = b"".join([np.array([n, R, ids, 1], np.int32).tobytes(), W.tobytes(), seeb.tobytes(), ssb.tobytes(),
                     coin.tobytes(), np.array([ids], np.int64).tobytes(), np.array([R], np.int32).tobytes()])
    return o, blob


def run_tables(path, host):
    """The program on one table file: {tag: decisions [pairs, N]} for tags ref / gpu,
    plus 'coin_votes' and (device runs) 'kernel'."""
    out = subprocess.run([EXE, "--tables", path] + (["--host"] if host else []), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] in ("ref", "gpu"):
            res[f[0]] = np.frombuffer(f[3].encode(), np.uint8).reshape(int(f[1]), int(f[2])) - ord("0")
        elif f[0] == "coin_votes":
            res["coin_votes"] = int(f[1])
        elif f[0] == "kernel":
            res["kernel"] = f[1]
    return res


def check_against_oracle(o, dec, what):
    """dec[i] (one call: pair i = round i) against the oracle's fame of every witness slot."""
    fame = o.fame_table()
    assert dec.shape == (fame.shape[0] - 1, fame.shape[1]), (dec.shape, fame.shape)
    has = fame[:-1] > -1
    assert has.any()
    np.testing.assert_array_equal(dec[has], fame[:-1][has], err_msg=what)
    assert (fame[-1] <= 0).all()  # the last round has no voters: nothing decided
