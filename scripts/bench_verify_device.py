#!/usr/bin/env python3
"""Event.Verify on the device against the host pipeline, same box, same stream.

verify:  a seeded signed stream of --events events (default 1M) at 16 and at 256 keys;
         one warm-up and --runs timed runs of engine.verify_events_device (HIP-event
         time of the kernels, and wall time with the copies), then the same stream
         through engine.verify_events on --threads host threads (the comparator).
         -> <out>/verify_1m.json
ingest:  one Engine.ingest_device line beside one Engine.ingest line at N = 256,
         200k events, k = 256.  -> <out>/ingest_256.json

Run it under a time limit of its own.  Without a GPU it fails: nothing falls back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from babble_amd import engine, signing  # noqa: E402
from babble_amd.engine import Engine, events_array  # noqa: E402
from babble_amd.gossip import random_gossip  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return {"median": med, "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / med, "runs": xs}


def signed_bodies(n_events, n_keys, seed, threads):
    """Bodies of an event body's size with seeded content, each signed by its creator."""
    rng = np.random.default_rng(seed)
    flat = rng.integers(0, 256, n_events * signing.BODY_BYTES, dtype=np.uint8)
    off = np.arange(n_events + 1, dtype=np.int64) * signing.BODY_BYTES
    cre = rng.integers(0, n_keys, n_events).astype(np.int32)
    pubs = signing.keys(n_keys, seed)
    sigs = signing.sign(flat, off, cre, n_keys, seed, threads)
    return pubs, flat, off, cre, sigs


def bench_verify(args):
    out = {"events": args.events, "runs": args.runs, "host_threads": args.threads, "body_bytes": signing.BODY_BYTES,
           "cases": []}
    for n_keys in (16, 256):
        pubs, flat, off, cre, sigs = signed_bodies(args.events, n_keys, 41 + n_keys, args.threads)
        sigs[args.events // 3, 5] ^= 1  # one bad signature: both paths must find exactly it
        dev_ms, dev_wall = [], []
        for run in range(args.runs + 1):
            t0 = time.perf_counter()
            ok, hashes, ms = engine.verify_events_device((flat, off), pubs, cre, sigs, device=args.device)
            wall = (time.perf_counter() - t0) * 1e3
            if run:  # the first run is the warm-up
                dev_ms.append(ms)
                dev_wall.append(wall)
        host_wall = []
        for run in range(args.host_runs + 1):
            t0 = time.perf_counter()
            hok, hhashes = engine.verify_events((flat, off), pubs[cre], sigs, threads=args.threads)
            wall = (time.perf_counter() - t0) * 1e3
            if run:
                host_wall.append(wall)
        assert np.array_equal(ok, hok) and np.array_equal(hashes, hhashes), "device and host verdicts differ"
        assert int((~ok).sum()) == 1 and not ok[args.events // 3]
        case = {"keys": n_keys, "device_kernel_ms": spread(dev_ms), "device_wall_ms": spread(dev_wall),
                "host_wall_ms": spread(host_wall)}
        case["device_kernel_events_per_s"] = args.events / (case["device_kernel_ms"]["median"] * 1e-3)
        case["device_wall_events_per_s"] = args.events / (case["device_wall_ms"]["median"] * 1e-3)
        case["host_events_per_s"] = args.events / (case["host_wall_ms"]["median"] * 1e-3)
        out["cases"].append(case)
        print(json.dumps(case), flush=True)
    return out


def bench_ingest(args):
    n, E, k = 256, args.ingest_events, 256
    dag = random_gossip(n, E, seed=12)
    pubs, bodies, sigs = signing.signed_stream(dag, seed=5, threads=args.threads)
    ev = events_array(dag)
    out = {"participants": n, "events": E, "k": k, "host_threads": args.threads, "lines": []}
    orders = {}
    for path in ("warm-up", "device", "host", "device", "host"):
        eng = Engine(n, E, device=args.device)
        if path == "host":
            rc, status, acc, tm = eng.ingest(ev, bodies, pubs, sigs, k, threads=args.threads)
        else:
            rc, status, acc, tm = eng.ingest_device(ev, bodies, pubs, sigs, k, verify_block=args.verify_block)
        assert rc == 0 and acc == E
        orders[path] = eng.consensus_log()
        eng.close()
        if path == "warm-up":
            continue
        line = {"path": path, **tm, "events_per_s": E / (tm["wall_ms"] * 1e-3)}
        out["lines"].append(line)
        print(json.dumps(line), flush=True)
    assert np.array_equal(orders["device"], orders["host"]), "the two paths order differently"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("verify", "ingest", "both"), default="both")
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--ingest-events", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--verify-block", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_device"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what in ("verify", "both"):
        with open(os.path.join(args.out, "verify_1m.json"), "w") as f:
            json.dump(bench_verify(args), f, indent=1)
    if args.what in ("ingest", "both"):
        with open(os.path.join(args.out, "ingest_256.json"), "w") as f:
            json.dump(bench_ingest(args), f, indent=1)


if __name__ == "__main__":
    main()
