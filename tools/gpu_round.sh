#!/bin/bash
# GPU-box check: parity tests, smoke, full bench line, rocprofv3 kernel-trace summary (logs under $OUT, default bench_out).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo "gpu tests failed"; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -3 $OUT/gpu_tests.log
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo "smoke failed"; tail -30 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 400 python -u bench.py --full ${BENCH_ARGS:-} > $OUT/bench.log 2>&1 || { echo "bench failed"; tail -30 $OUT/bench.log; exit 1; }
tail -1 $OUT/bench.log
if [ -n "$PROF" ]; then
  export TMPDIR=/tmp
  cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats -f csv rocpd -d "$R/$OUT/prof" -o run -- python3 "$R/bench.py" --full --steps 3 --warmup 1 --no-cpu > "$R/$OUT/prof.log" 2>&1 || { echo "prof failed"; tail -30 "$R/$OUT/prof.log"; exit 1; }
  grep '^{' "$R/$OUT/prof.log" | tail -1
  python3 "$R/tools/prof_summary.py" "$R/$OUT/prof" "$R/$OUT/prof.md"
fi
