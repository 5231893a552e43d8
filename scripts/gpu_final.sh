#!/bin/bash
# the round-end invocations as the driver runs them: smoke, then the default bench line with
# everything behind --full.  usage: scripts/gpu_final.sh [out_dir]
set -o pipefail
OUT=${1:-bench_out/final}
mkdir -p $OUT
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 600 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 2; }
python -c "
import json
d=json.loads(open('$OUT/bench.json').read().strip().splitlines()[-1])
print(round(d['value']/1e6,2), d['ms_per_step'], d['parity'][:200]); print(d['cpu_baseline']['value'], d['roofline']['frac'])
for k,v in d['secondary'].items(): print(k, v.get('value'), v.get('call_latency_us'), v.get('host_round_trips_per_call'), (v.get('parity') or '')[:40])"
