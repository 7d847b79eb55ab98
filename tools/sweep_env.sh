#!/bin/bash
# GPU box: short default bench under each value of one environment variable.
# usage: tools/sweep_env.sh VAR v1 v2 ...   (results under $OUT, default bench_out)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; OUT=${OUT:-bench_out}; mkdir -p $OUT
VAR=$1; shift
for v in "$@"; do
  env "$VAR=$v" timeout -k 10 150 python -u bench.py --full --steps 5 --warmup 2 --latency-iters 1 --no-cpu --ingest-steps 0 > $OUT/sw_$v.json 2> $OUT/sw_$v.err || exit 1
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(sys.argv[2],d['value'],round(d['roofline']['stages_ms']['rpp_first'],1),round(d['roofline']['stages_ms']['rpp_cand'],1))" $OUT/sw_$v.json "$VAR=$v"
done
