#!/bin/bash
# GPU box: short default bench at several context counts (and rig counts).
# usage: tools/sweep_ctx.sh "CTX:RIGS" ...   e.g. 2:3072 3:3072 4:3072   (results under $OUT, default bench_out)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"; OUT=${OUT:-bench_out}; mkdir -p $OUT
for cr in "$@"; do
  c=${cr%%:*}; r=${cr##*:}
  timeout -k 10 200 python -u bench.py --full --steps 4 --warmup 2 --latency-iters 1 --no-cpu --ingest-steps 0 --contexts $c --rigs $r > $OUT/ctx_${c}_$r.json 2> $OUT/ctx_${c}_$r.err || exit 1
  python3 -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(sys.argv[2],d['value'],d['ms_per_step'],{k:round(v,1) for k,v in d['roofline']['stages_ms'].items() if v>5})" $OUT/ctx_${c}_$r.json "ctx=$c rigs=$r"
done
