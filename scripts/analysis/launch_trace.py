"""What the engine launches, case by case: for a fixed list of small cases that
between them take each walk and each lastAncestors path of the coordinate and rounds
step (not the split run's joined rows or the hand-off fallback), the multiset of
(kernel name, launches) from kernel_stats() with profiling on, the host round
trips (host_syncs) and the digest of the final state (tests/golden/digest.py).
Two builds that launch the same kernels the same number of times, wait on the
stream as often and end in the same state give the same JSON, so a refactor of the
host side is checked by diffing the file of the build before against the one after.

    python scripts/analysis/launch_trace.py [-o trace.json] [case ...]

Every case runs in a process of its own (the engine reads some switches from the
environment when it is created).  HGE_LIB picks the library as everywhere else.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

# name: (N, events, K, seed, mode, engine capacity (None: the events), online calls (None: all), environment)
CASES = {
    "n4_replay": (4, 600, 4, 3, "replay", None, None, {}),
    "n16_online": (16, 3000, 3, 1, "online", None, None, {}),
    "n16_online_nofast": (16, 3000, 3, 1, "online", None, None, {"HGE_NO_ONLINE_FAST": "1", "HGE_NO_FD_DIRECT": "1"}),
    "n32_online": (32, 2000, 32, 1, "online", None, None, {}),
    "n32_replay_walkers4": (32, 6000, 32, 1, "replay", None, None, {"HGE_WALKERS": "4"}),
    "n32_replay_walkers4_hcap8": (32, 6000, 32, 1, "replay", None, None, {"HGE_WALKERS": "4", "HGE_WALK_HCAP": "8"}),
    "n48_online": (48, 5000, 48, 1, "online", None, None, {}),
    "n48_replay": (48, 5000, 48, 1, "replay", None, None, {}),
    "n50_replay": (50, 5000, 50, 1, "replay", None, None, {}),
    "n64_replay_coop_walkers2": (64, 8000, 64, 1, "replay", None, None, {"HGE_COOP_WALKERS": "2"}),
    "n128_replay_lw_g3": (128, 15000, 128, 1, "replay", None, None, {"HGE_LW_G": "3"}),
    "n256_replay": (256, 25000, 256, 1, "replay", None, None, {}),
    "n256_online_40": (256, 25000, 256, 1, "online", None, 40, {}),
    "n64_replay_chain_limit60": (64, 8000, 64, 1, "replay", None, None, {"HGE_CHAIN_LIMIT": "60"}),
    "n256_replay_rounds_grow": (256, 400_000, 256, 78, "replay", 1024, None, {}),
    # chains past 65,534 events at N <= 32: int32 first-strong-seer rows, k_rounds_fss
    "n2_replay_long_chain": (2, 140_000, 35_000, 5, "replay", None, None, {}),
}


def run_case(name):
    import numpy as np
    from babble_amd.engine import Engine, events_array
    from babble_amd.gossip import random_gossip, schedule
    from digest import digest, engine_state
    n, E, K, seed, mode, cap, ncalls, _ = CASES[name]
    ev = events_array(random_gossip(n, E, seed=seed))
    calls = schedule(E, K)
    eng = Engine(n, E if cap is None else cap)
    try:
        eng.set_profiling(True)
        s0 = eng.host_syncs()
        if mode == "replay":
            status, order, counts = eng.replay(ev, calls)
        else:
            calls = calls[:ncalls]
            ids, per, prev = [], [], 0
            for c in calls:
                ids.append(eng.insert_events(ev[prev:c].copy()))
                per.append(len(eng.run_consensus()))
                prev = c
            status, order, counts = np.concatenate(ids), eng.consensus_events(), np.asarray(per, np.int64)
        syncs = eng.host_syncs() - s0
        stats = eng.kernel_stats()
        return {"launches": {k: int(v[1]) for k, v in sorted(stats.items())},
                "host_syncs": int(syncs), "calls": int(len(calls)), "ordered": int(len(order)),
                "rounds": int(eng.rounds()), "digest": digest(engine_state(eng, status, order, counts))}
    finally:
        eng.close()


def main():
    args = sys.argv[1:]
    if args[:1] == ["--case"]:
        print("TRACE " + json.dumps(run_case(args[1])))
        return
    out_path = None
    if args[:1] == ["-o"]:
        out_path, args = args[1], args[2:]
    out = {}
    for name in args or list(CASES):
        env = dict(os.environ)
        for k in [k for k in env if k.startswith("HGE_") and k != "HGE_LIB"]:
            del env[k]
        env.update(CASES[name][7])
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], env=env,
                           capture_output=True, text=True, timeout=300)
        line = next((l for l in p.stdout.splitlines() if l.startswith("TRACE ")), None)
        if p.returncode != 0 or line is None:
            # a case that died may have faulted the device: start nothing more on it
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"launch_trace: case {name} ended with status {p.returncode}")
        out[name] = json.loads(line[6:])
    text = json.dumps(out, indent=1, sort_keys=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
