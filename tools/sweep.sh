#!/bin/bash
# bench sweep over batch size / contexts (GPU box); one line per config into $OUT/sweep.log (OUT defaults to bench_out)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; export OUT=${OUT:-bench_out}; mkdir -p $OUT
: > $OUT/sweep.log
for cfg in "$@"; do
  echo "== $cfg" >> $OUT/sweep.log
  timeout -k 10 300 python bench.py --full --no-cpu --latency-iters 3 $cfg >> $OUT/sweep.log 2>&1 || { echo "failed: $cfg"; tail -20 $OUT/sweep.log; exit 1; }
done
python - <<'P'
import json
import os
for l in open(os.path.join(os.environ['OUT'], 'sweep.log')):
    if l.startswith('=='): print(l.strip(), end=' ')
    elif l.startswith('{'):
        d=json.loads(l); r=d.get('roofline') or {}; print(d['value'], d['ms_per_step'], d['p50_latency_ms'], r.get('kernel'), r.get('achieved'), r.get('unit'), json.dumps(r.get('stages_ms')))
P
