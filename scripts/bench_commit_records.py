#!/usr/bin/env python3
"""What FindOrder's commit records cost when read on demand (hge_commit_records and the
_records calls), against the routes a caller had before them.

Whole log, the bench's own stream (256 participants, 10M events, a call every 256) after
one bulk replay; destinations allocated outside the timed region:

  records      hge_commit_records over the whole log: ids, rr, cts, sources
  plain        the same without sources
  tables       the only earlier route to the same data: hge_event_received (the rr and cts
               tables of every event) + hge_consensus_timestamp_sources over the whole
               order; `tables_joined` adds the host join rr[order], cts[order]

Online, per consensus call, on the first 512,000 submissions of that stream and on a
16-participant stream of 100,000 events; three engines fed the same stream, the variants
alternated call by call, only the consensus call timed (not hge_insert_events):

  run          hge_run_consensus alone
  records      hge_run_consensus_records (ids, rr, sources: what the Go shim asks for)
  shim         the shim's earlier sequence: hge_run_consensus for the batch, then
               hge_consensus_log + hge_consensus_timestamp_sources + one hge_round_received
               per ordered event

Host clock (time.perf_counter) around work that ends in a stream synchronise; one warm-up
and --reps timed repetitions (a repetition of an online workload is one pass over its
stream on engines reset in between).  Every repetition goes into the output file.

  python scripts/bench_commit_records.py [--reps 5] [--events 10000000] [--online 512000] [--out PATH]
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


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def whole_log(n, E, dag, reps):
    from babble_amd.engine import Engine, _p32, _p64, events_array
    from babble_amd.gossip import schedule
    eng = Engine(n, E)
    eng.prepare(events_array(dag), schedule(E, n))
    m = eng.run()
    L, h = eng.L, eng.h
    ev = eng.event_count()
    ids, rr, src = (np.zeros(m, np.int32) for _ in range(3))
    cts = np.zeros(m, np.int64)
    trr, tcts, tsrc = np.zeros(ev, np.int32), np.zeros(ev, np.int64), np.zeros(m, np.int32)

    def records():
        assert L.hge_commit_records(h, 0, m, _p32(ids), _p32(rr), _p64(cts), _p32(src)) == m

    def plain():
        assert L.hge_commit_records(h, 0, m, _p32(ids), _p32(rr), _p64(cts), None) == m

    joined = {}

    def tables():
        order = eng.order_view()
        eng._check(L.hge_event_received(h, _p32(trr), _p64(tcts), ev))
        eng._check(L.hge_consensus_timestamp_sources(h, _p32(order), m, _p32(tsrc)))
        t = time.perf_counter()
        joined["rr"], joined["cts"] = trr[order], tcts[order]
        joined["ms"] = (time.perf_counter() - t) * 1e3

    variants = {"records": records, "plain": plain, "tables": tables}
    ms = {k: [] for k in list(variants) + ["tables_joined"]}
    waits = {}
    for rep in range(reps + 1):  # the first round is the warm-up
        for name, fn in variants.items():
            w0 = eng.host_syncs()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            waits[name] = eng.host_syncs() - w0
            if rep:
                if name == "tables":
                    ms["tables"].append(round(dt - joined["ms"], 3))
                    ms["tables_joined"].append(round(dt, 3))
                else:
                    ms[name].append(round(dt, 3))
    records()
    tables()
    equal = bool(np.array_equal(ids, eng.order_view()) and np.array_equal(rr, joined["rr"]) and
                 np.array_equal(cts, joined["cts"]) and np.array_equal(src, tsrc))
    eng.close()
    return {"workload": f"{n} participants, {E} events, a call every {n}: {m} records after one bulk replay",
            "ms": ms, "stats_ms": {k: stats(v) for k, v in ms.items()}, "host_waits": waits,
            "records_equal_tables_route": equal}


def online(n, E, K, seed, reps, dag=None):
    from babble_amd.engine import Engine, _p32, _p64, events_array
    from babble_amd.gossip import random_gossip, schedule
    if dag is None:
        dag = random_gossip(n, E, seed=seed)
    ev = events_array(dag)[:E]
    calls = schedule(E, K)
    names = ("run", "records", "shim")
    engs = {k: Engine(n, E) for k in names}
    L = engs["run"].L
    cap = E
    ids, rr, src = (np.zeros(cap, np.int32) for _ in range(3))
    nn = ctypes.c_int64()

    def run(e):
        e._check(L.hge_run_consensus(e.h, _p32(ids), cap, ctypes.byref(nn)))

    def records(e):
        e._check(L.hge_run_consensus_records(e.h, cap, _p32(ids), _p32(rr), None, _p32(src), ctypes.byref(nn)))

    def shim(e):
        e._check(L.hge_run_consensus(e.h, None, 0, ctypes.byref(nn)))
        k = nn.value
        if k:
            L.hge_consensus_log(e.h, L.hge_consensus_count(e.h) - k, _p32(ids), k)
            e._check(L.hge_consensus_timestamp_sources(e.h, _p32(ids), k, _p32(src)))
            for q in range(k):
                rr[q] = L.hge_round_received(e.h, int(ids[q]))

    fns = {"run": run, "records": records, "shim": shim}
    per_call_us = {k: [] for k in names}
    waits_per_call = {}
    ordered = 0
    for rep in range(reps + 1):
        tot = {k: 0.0 for k in names}
        w = {k: 0 for k in names}
        for e in engs.values():
            e.reset()
        prev = 0
        got = {k: 0 for k in names}
        for c in calls:
            for k in names:
                e = engs[k]
                e.insert_events(ev[prev:c])
                w0 = e.host_syncs()
                t0 = time.perf_counter()
                fns[k](e)
                tot[k] += time.perf_counter() - t0
                w[k] += e.host_syncs() - w0
                got[k] += nn.value
            prev = c
        assert got["run"] == got["records"] == got["shim"]
        ordered = got["run"]
        if rep:
            for k in names:
                per_call_us[k].append(round(tot[k] / len(calls) * 1e6, 2))
            waits_per_call = {k: round(w[k] / len(calls), 3) for k in names}
    for e in engs.values():
        e.close()
    return {"workload": f"{n} participants, {E} events, a call every {K}: {len(calls)} calls, {ordered} ordered",
            "per_call_us": per_call_us, "stats_per_call_us": {k: stats(v) for k, v in per_call_us.items()},
            "host_waits_per_call": waits_per_call}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--participants", type=int, default=256)
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--online", type=int, default=512_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip", default="", help="comma list of: whole, online256, online16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commit_records", "records_256x10m.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("at least five repetitions per variant")
    skip = set(args.skip.split(","))
    from babble_amd.gossip import random_gossip
    n = args.participants
    out = {"method": ("host clock (time.perf_counter) around calls that end in a stream synchronise; variants "
                      f"alternated inside one process; one warm-up round, then {args.reps} timed")}
    ns = max(n, min(args.online, args.events) // n * n)
    dag = random_gossip(n, args.events, seed=args.seed) if not {"whole", "online256"} <= skip else None
    print(json.dumps({"stream": f"{n} participants, {args.events} events generated"}), flush=True)
    if "whole" not in skip:
        out["whole_log"] = whole_log(n, args.events, dag, args.reps)
        print(json.dumps({"whole_log": out["whole_log"]["stats_ms"]}), flush=True)
    if "online256" not in skip:
        out["online_prefix"] = online(n, ns, n, args.seed, args.reps, dag=dag)
        print(json.dumps({"online_prefix": out["online_prefix"]["stats_per_call_us"]}), flush=True)
    if "online16" not in skip:
        out["online_16_100k"] = online(16, 100_000, 16, args.seed, args.reps)
        print(json.dumps({"online_16_100k": out["online_16_100k"]["stats_per_call_us"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if "whole_log" in out and not out["whole_log"]["records_equal_tables_route"]:
        sys.exit("the records differ from the tables route")


if __name__ == "__main__":
    main()
