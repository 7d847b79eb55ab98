#!/bin/bash
# GPU box: full bench line (config 3 + host ingest + CPU baseline), then the config 4 / 5 legs (logs under $OUT, default bench_out).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 600 python -u bench.py --full ${BENCH_ARGS:-} > $OUT/bench3.log 2>&1 || { echo "bench3 failed"; tail -30 $OUT/bench3.log; exit 1; }
grep '^{' $OUT/bench3.log | tail -1
timeout -k 10 300 python -u bench.py --config 4 --steps 5 --warmup 1 > $OUT/bench4.log 2>&1 || { echo "bench4 failed"; tail -30 $OUT/bench4.log; exit 1; }
grep '^{' $OUT/bench4.log | tail -1
timeout -k 10 300 python -u bench.py --config 5 --steps 10 --warmup 2 > $OUT/bench5.log 2>&1 || { echo "bench5 failed"; tail -30 $OUT/bench5.log; exit 1; }
grep '^{' $OUT/bench5.log | tail -1
