#!/usr/bin/env python3
"""What it costs to get a Monte Carlo batch onto the device: generated there against
built on the host.

Workload: config 5's batch as counter_gossip states it (1,024 graphs, N = 32, 10,000 honest
events each, 10 forkers, fork_p 0.05, cascade_p 0.5, K = 32; graph g's seed is seed0 + g).
Variants, alternated inside this one process, host clock around calls that end in a stream
synchronise (stage() does):

  a  counter_gossip in Python for every graph, packed to hge_event records, add(), stage()
  b  add() + stage() alone, on the records a built
  c  generate() + stage(): the streams generated, admitted and laid out by kernels

Each starts from clear() on a Batch that has staged the workload before (allocations kept),
and is followed by a timed run(), to show that run() does not care where its tables came
from.  After the timed repetitions every graph's info and the consensus order of every 64th
graph are compared between the add-built and the generated batch.  Every repetition goes
into the output file.

  python scripts/bench_batch_generate.py [--graphs 1024] [--reps 5] [--warmup 1] [--variants abc] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAMS = dict(n=32, events=10000, k=32, forkers=10, fork_p=0.05, cascade_p=0.5, op_lag=0, seed0=50000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--events", type=int, default=PARAMS["events"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_generate", "front_1024x32x10k.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("at least five repetitions per variant")

    from babble_amd.engine import Batch, events_array
    from babble_amd.gossip import counter_gossip, schedule

    p = dict(PARAMS, events=args.events)
    G, n = args.graphs, p["n"]
    gen_args = (p["forkers"], p["fork_p"], p["cascade_p"], p["op_lag"])
    added, generated = Batch(n), Batch(n)
    built = []  # variant a's records and call points, variant b's input

    def build():
        built.clear()
        for g in range(G):
            dag = counter_gossip(n, p["events"], p["seed0"] + g, *gen_args)
            built.append((events_array(dag), schedule(len(dag["creator"]), p["k"])))

    def variant(name):
        b = generated if name == "c" else added
        t0 = time.perf_counter()
        b.clear()
        if name == "a":
            build()
        if name == "c":
            b.generate(p["events"], p["k"], G, p["seed0"], *gen_args)
        else:
            for ev, calls in built:
                b.add(ev, calls)
        b.stage()
        t1 = time.perf_counter()
        ordered = b.run()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, ordered

    names = args.variants
    if "a" not in names:
        build()
    front = {v: [] for v in names}
    run = {v: [] for v in names}
    ordered = set()
    for r in range(args.warmup + args.reps):
        for v in names:
            f, x, m = variant(v)
            ordered.add(m)
            if r >= args.warmup:
                front[v].append(round(f, 3))
                run[v].append(round(x, 3))
        print(f"round {r + 1} of {args.warmup + args.reps} done", flush=True)

    equal = None
    if "c" in names and len(names) > 1:
        equal = all(added.info(g) == generated.info(g) for g in range(G))
        for g in range(0, G, 64):
            equal = equal and np.array_equal(added.state(g)["order"], generated.state(g)["order"])
        equal = bool(equal and len(ordered) == 1)
    submissions = int(sum(len(ev) for ev, _ in built))

    def stats(reps):
        return {v: {"median": round(statistics.median(reps[v]), 3), "min": min(reps[v]), "max": max(reps[v])}
                for v in names}

    fm, rm = stats(front), stats(run)
    out = {
        "workload": {"graphs": G, **p, "submissions": submissions, "ordered_per_run": sorted(ordered)},
        "method": ("two Batches that staged the workload before (allocations kept); variants alternated inside "
                   "one process; host clock (time.perf_counter) from clear() to the end of stage(), which "
                   f"synchronises the stream, then around run(); {args.warmup} warm-up rounds, then {args.reps} timed"),
        "variants": {"a": "counter_gossip in Python + hge_event packing + add() + stage()",
                     "b": "add() + stage() on pre-built records",
                     "c": "generate() + stage() (kg_walk counting, kg_walk, kg_fill)"},
        "front_ms": front,
        "run_ms": run,
        "front_stats_ms": fm,
        "run_stats_ms": rm,
        "generated_equals_added": equal,
    }
    if "c" in names:
        c = fm["c"]["median"]
        out["ratios"] = {f"{v}_over_c": round(fm[v]["median"] / c, 2) for v in names if v != "c"}
        out["ratios"]["c_over_one_run"] = round(c / rm["c"]["median"], 3)
        out["c_below_b"] = bool("b" in names and max(front["c"]) < min(front["b"]))
    added.close()
    generated.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out.get(k) for k in ("front_stats_ms", "run_stats_ms", "ratios", "c_below_b",
                                              "generated_equals_added")}))
    if equal is False:
        sys.exit("the generated batch differs from the add-built one")


if __name__ == "__main__":
    main()
