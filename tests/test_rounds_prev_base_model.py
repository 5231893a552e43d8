"""The value ranges of the direct rounds walk's 8-bit rows when both sides of round r are
encoded against the PREVIOUS frontier C_{r-1} (babble_amd/csrc/hge_narrow.h), modelled on
the CPU for the plain streams of tests/test_gpu_rounds_prev_base.py: the frontiers
C_r[c] = first position of chain c with round >= r come from the oracle's rounds, LA and
the members' FD rows are recomputed in numpy.  Over the first 32 window rows of every
chain-round no window value LA - C_{r-1} + 2 may reach 126 (condition (i)), and no finite
member value FD[m_d][i] may lie below its base (condition (ii)): that is the condition
under which the GPU test may demand the narrow path of these streams."""
import numpy as np
import pytest

from babble_amd.gossip import random_gossip, schedule
from parity import oracle_run

H = 32  # window rows the per-member bisection covers
INF = np.iinfo(np.int32).max

STREAMS = {
    "plain64": (64, 6000, 100, 11),
    "plain132": (132, 9240, 132, 7),
    "plain256": (256, 20000, 500, 5),
}


def frontier_model(dag, rounds):
    """(largest window value against C_{r-1}, largest against C_r, largest member value,
    finite member values below their base, chain-rounds, largest advance)."""
    n = int(dag["n"])
    creator, index, sp, op = (np.asarray(dag[k]) for k in ("creator", "index", "sp", "op"))
    E = len(creator)
    la = np.full((E, n), -1, np.int32)
    for x in range(E):  # submission order is topological
        if sp[x] >= 0:
            la[x] = la[sp[x]]
        if op[x] >= 0:
            np.maximum(la[x], la[op[x]], out=la[x])
        la[x, creator[x]] = index[x]
    chains = [np.flatnonzero(creator == c) for c in range(n)]
    for c in range(n):
        assert np.array_equal(index[chains[c]], np.arange(len(chains[c])))
    lac = [la[chains[c]] for c in range(n)]  # rows of chain c by position
    R = int(rounds.max()) + 1
    C = np.full((R, n), INF, np.int64)
    for c in range(n):
        rc = rounds[chains[c]]
        assert np.all(np.diff(rc) >= 0)
        for r in range(R):
            p = int(np.searchsorted(rc, r))
            if p < len(rc):
                C[r, c] = p
    win_prev = win_cur = mem = below = chain_rounds = adv = 0
    for r in range(R):
        base = C[max(r - 1, 0)]  # the walk's first round: its own frontier
        have = base != INF
        if r > 0:
            both = C[r] != INF
            adv = max(adv, int((C[r][both] - base[both]).max()))
        # member rows: FD[(d, C_r[d])][i] = first position of chain i that has the member
        # as an ancestor
        # (column d of chain i's rows only grows along the chain), for every d at once
        member = C[r] != INF
        for i in range(n):
            seen = lac[i][:, member] >= C[r][member]  # [position, member]
            p = seen.argmax(axis=0)[seen.any(axis=0)]  # finite FD values only
            if len(p) == 0:
                continue
            if base[i] == INF:
                below += len(p)
                continue
            below += int((p < base[i]).sum())
            mem = max(mem, int(p.max() - base[i] + 2))
        for c in range(n):
            if C[r, c] == INF:
                continue
            chain_rounds += 1
            rows = lac[c][C[r, c]:C[r, c] + H].astype(np.int64)
            win_prev = max(win_prev, int((rows[:, have] - base[have] + 2).max()))
            cur = C[r] != INF
            win_cur = max(win_cur, int((rows[:, cur] - C[r][cur] + 2).max()))
    return win_prev, win_cur, mem, below, chain_rounds, adv


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_previous_base_keeps_plain_streams_narrow(name):
    n, e, k, seed = STREAMS[name]
    dag = random_gossip(n, e, seed=seed)
    # (the rounds do not depend on the call schedule: one RunConsensus at the end)
    o, st, order, counts = oracle_run(dag, schedule(e, e))
    assert np.array_equal(st, np.arange(e)), "every submission is admitted under its own index"
    rounds, _ = o.event_rounds()
    win_prev, win_cur, mem, below, chain_rounds, adv = frontier_model(dag, rounds)
    print(f"{name}: LA - C_r + 2 <= {win_cur}, LA - C_(r-1) + 2 <= {win_prev}, member values <= {mem}, "
          f"below their base {below}, chain-rounds {chain_rounds}, largest advance {adv}")
    assert chain_rounds > n
    assert win_prev < 126, win_prev
    assert below == 0, below
    assert mem <= 127
