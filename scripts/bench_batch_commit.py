#!/usr/bin/env python3
"""What delivering the batch engine's commit stream to host memory costs a run.

Workload: config 5's own batch, the graphs of tests/golden/make_mc_digests.py::graph_stream
(1,024 random-gossip hashgraphs, N = 32, 10,000 submissions each, K = 32), staged once in
one Batch.  Variants, alternated inside this one process, host clock around calls that
end in the run's synchronise:

  a  delivery off: run() alone (bench.py's timed step)
  b  delivery off: run(), then every graph's order and counts through hge_batch_results
     (two device-to-host copies per graph into preallocated arrays: how a caller gets them
     without the mode)
  c  run() with deliver(order=True)
  d  run() with deliver(order=True, received=True)

After the timed repetitions every graph's delivered order and counts (c and d) are compared
with what b fetched.  Every repetition goes into the output file.

  python scripts/bench_batch_commit.py [--graphs 1024] [--reps 7] [--warmup 3] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_commit", "delivery_1024x32x10k.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("at least five repetitions per variant")

    from babble_amd.engine import Batch, _p32, _p64
    from make_mc_digests import PARAMS, graph_stream

    b = Batch(PARAMS["n"])
    G = args.graphs
    for g in range(G):
        b.add(*graph_stream(g))
    b.stage()
    ordered = b.run()
    infos = [b.info(g) for g in range(G)]
    calls = sum(i["calls"] for i in infos)
    # variant b's destinations, allocated outside the timed region
    got = [(np.zeros(max(i["ordered"], 1), np.int32), np.zeros(max(i["calls"], 1), np.int64)) for i in infos]

    def fetch_all():
        for g, (o, c) in enumerate(got):
            b._check(b.L.hge_batch_results(b.h, g, _p32(o), _p64(c), None, None, None, None, None, None))

    def variant(name):
        if name in "ab":
            b.deliver(order=False)
        else:
            b.deliver(order=True, received=name == "d")
        b.stage()  # the delivery buffers are sized here, outside the timed region
        t0 = time.perf_counter()
        n = b.run()
        if name == "b":
            fetch_all()
        t1 = time.perf_counter()
        assert n == ordered
        return (t1 - t0) * 1e3

    names = "abcd"
    for _ in range(args.warmup):
        for v in names:
            variant(v)
    reps = {v: [] for v in names}
    modes = {}
    for _ in range(args.reps):
        for v in names:
            reps[v].append(round(variant(v), 4))
            modes[v] = b.delivered()

    # what c and d delivered against what b fetched
    variant("b")
    equal = {}
    for v in "cd":
        variant(v)
        ok = True
        for g, (o, c) in enumerate(got):
            s = b.commits(g)
            n, k = infos[g]["ordered"], infos[g]["calls"]
            ok = ok and np.array_equal(s["ids"], o[:n]) and np.array_equal(s["counts"], c[:k])
            ok = ok and (s["rr"] is None) == (v == "c")
        equal[v] = bool(ok)

    med = {v: statistics.median(reps[v]) for v in names}
    out = {
        "workload": {"graphs": G, **PARAMS, "ordered_per_run": ordered, "calls": calls},
        "method": ("one Batch staged once; variants alternated a, b, c, d inside one process; host clock "
                   "(time.perf_counter) around run() [+ the hge_batch_results calls for b], each ending in the "
                   f"run's stream synchronise; {args.warmup} warm-up rounds of all four, then {args.reps} timed"),
        "variants": {"a": "delivery off, run() alone",
                     "b": "delivery off, run() then order and counts of every graph through hge_batch_results",
                     "c": "run() with delivery bit 0 (order, counts)",
                     "d": "run() with delivery bits 0 and 1 (order, counts, rr, cts)"},
        "delivered_mode": modes,
        "delivered_bytes": {"c": ordered * 4 + calls * 8, "d": ordered * 16 + calls * 8},
        "ms": reps,
        "median_ms": {v: round(med[v], 4) for v in names},
        "a_spread_ms": {"min": min(reps["a"]), "max": max(reps["a"]),
                        "stdev": round(statistics.stdev(reps["a"]), 4)},
        "minus_a_ms": {v: round(med[v] - med["a"], 4) for v in "bcd"},
        "delivered_equals_b": equal,
    }
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("median_ms", "a_spread_ms", "minus_a_ms", "delivered_mode",
                                          "delivered_equals_b")}))
    if not all(equal.values()):
        sys.exit("delivered streams differ from hge_batch_results")


if __name__ == "__main__":
    main()
