#!/usr/bin/env python3
"""What it costs to read a Monte Carlo batch's consensus-latency statistics: reduced on
the device (Batch.stats, hge_batch_stats) against the only route without it, every graph's
state copied to the host and binned in numpy.

Workload: config 5's batch as generate() states it (1,024 graphs, N = 32, 10,000 honest
events each, 10 forkers, fork_p 0.05, cascade_p 0.5, K = 32; graph g's seed is seed0 + g),
generated and staged once.  Variants, alternated inside this one process, host clock around
calls that end in a stream synchronise:

  a  run()
  b  run() + stats() with the default spec
  c  run() + state(g) for every graph + the same statistics in numpy (each graph's
     submission statuses and timestamps are read back once, before the timed rounds: they
     do not change between runs)

After the timed repetitions b's rows and histograms are compared with c's.  Every
repetition goes into the output file.

  python scripts/bench_batch_stats.py [--graphs 1024] [--reps 5] [--warmup 1] [--out PATH]
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
U64 = (1 << 64) - 1


def host_stats(st, ts, callE, spec, fields):
    """One graph's row and histograms from its state, as tests/stats_expect.py states them
    (vectorised: the ts bins through the unsigned difference)."""
    E = len(ts)
    x = np.arange(E, dtype=np.int64)
    rr = st["rr"].astype(np.int64)
    sel = (rr >= 0) & (x >= spec.x_lo) & (x < spec.x_hi)
    ccall = np.full(E, -1, np.int64)
    ccall[st["order"]] = np.repeat(np.arange(len(callE)), st["counts"])
    xs = x[sel]
    dround = rr[sel] - st["rounds"][sel]
    cc = ccall[sel]
    dcall = cc - np.searchsorted(callE, xs, side="right")
    lag = callE[cc] - 1 - xs
    dts = st["cts"][sel] - ts[sel]
    below = dts < spec.ts_lo
    q = (dts.view(np.uint64) - np.uint64(spec.ts_lo & U64)) // np.uint64(spec.ts_bin)
    tsb = np.where(below, 0, 1 + np.minimum(q, np.uint64(spec.ts_bins)).astype(np.int64))
    hist = np.concatenate([np.bincount(np.minimum(dround, spec.round_bins - 1), minlength=spec.round_bins),
                           np.bincount(np.minimum(dcall, spec.call_bins - 1), minlength=spec.call_bins),
                           np.bincount(np.minimum(lag // spec.lag_bin, spec.lag_bins - 1), minlength=spec.lag_bins),
                           np.bincount(tsb, minlength=spec.ts_bins + 2)]).astype(np.int64)
    fame, R = st["fame"], int(st["scalars"][0])
    inr = int(((x >= spec.x_lo) & (x < spec.x_hi)).sum())
    row = np.zeros(fields, np.int64)
    row[:10] = [E, inr, len(xs), inr - len(xs), R, int(st["scalars"][1]), (fame[:R] >= 0).sum(), (fame[:R] == 1).sum(),
                (fame[:R] == 2).sum(), (fame[:R] == 0).sum()]
    if len(xs):
        row[10:19] = [dround.sum(), dround.max(), dcall.sum(), dcall.max(), lag.sum(), lag.max(), dts.sum(), dts.min(),
                      dts.max()]
    return row, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--events", type=int, default=PARAMS["events"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_stats", "stats_1024x32x10k.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("at least five repetitions per variant")

    from babble_amd.engine import STATS_FIELDS, Batch, StatsSpec
    from babble_amd.gossip import schedule

    p = dict(PARAMS, events=args.events)
    G, n = args.graphs, p["n"]
    spec = StatsSpec(lag_bin=n)
    b = Batch(n)
    b.generate(p["events"], p["k"], G, p["seed0"], p["forkers"], p["fork_p"], p["cascade_p"], p["op_lag"])
    b.stage()
    # what does not change between runs: each graph's accepted timestamps and call points
    ts, callE = [], []
    if "c" in args.variants:
        for g in range(G):
            sub = b.submissions(g)
            b.status[g] = sub["status"]
            acc = sub["status"] >= 0
            t = np.zeros(int(acc.sum()), np.int64)
            t[sub["status"][acc]] = sub["ts"][acc]
            ts.append(t)
            callE.append(np.cumsum(acc)[schedule(len(acc), p["k"]) - 1].astype(np.int64))
    last = {}

    def variant(name):
        t0 = time.perf_counter()
        ordered = b.run()
        if name == "b":
            last["b"] = b.stats(spec)
        if name == "c":
            rows, hist = [], 0
            for g in range(G):
                r, h = host_stats(b.state(g), ts[g], callE[g], spec, len(STATS_FIELDS))
                rows.append(r)
                hist = hist + h
            last["c"] = (np.array(rows), hist)
        return (time.perf_counter() - t0) * 1e3, ordered

    ms = {v: [] for v in args.variants}
    ordered = set()
    for r in range(args.warmup + args.reps):
        for v in args.variants:
            t, m = variant(v)
            ordered.add(m)
            if r >= args.warmup:
                ms[v].append(round(t, 3))
        print(f"round {r + 1} of {args.warmup + args.reps} done", flush=True)

    equal = None
    if "b" in last and "c" in last:
        got = last["b"]["graphs"].view(np.int64).reshape(G, -1)
        equal = bool(np.array_equal(got, last["c"][0]) and np.array_equal(last["b"]["hist"], last["c"][1]))
    st = {v: {"median": round(statistics.median(ms[v]), 3), "min": min(ms[v]), "max": max(ms[v])} for v in ms}
    out = {
        "workload": {"graphs": G, **p, "ordered_per_run": sorted(ordered), "fallbacks": b.fallbacks(),
                     "hist_len": spec.hist_len()},
        "method": ("one Batch, generated and staged once; variants alternated inside one process; host clock "
                   "(time.perf_counter) around run() and what follows it, each ending in a stream synchronise; "
                   f"{args.warmup} warm-up rounds, then {args.reps} timed"),
        "variants": {"a": "run()", "b": "run() + stats(default spec): ks_events, ks_finish, ks_total, one copy",
                     "c": "run() + state(g) for every graph + numpy"},
        "ms": ms,
        "stats_ms": st,
        "device_equals_host": equal,
    }
    if all(v in st for v in "abc"):
        a, bb, c = (st[v]["median"] for v in "abc")
        out["stats_over_run"] = round((bb - a) / a, 4)
        out["host_route_over_stats"] = round((c - a) / max(bb - a, 1e-6), 1)
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out.get(k) for k in ("stats_ms", "stats_over_run", "host_route_over_stats",
                                              "device_equals_host")}))
    if equal is False:
        sys.exit("the device's statistics differ from the host route's")


if __name__ == "__main__":
    main()
