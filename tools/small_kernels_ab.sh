#!/bin/bash
# GPU suite subset touching row statistics / neighbour counts, then a traced bench.
# Results land in $OUT_DIR (default: bench_out/).
set -euo pipefail
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT/prof_sk"
export TMPDIR=/tmp
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/sk_tests.log" 2>&1
tail -1 "$OUT/sk_tests.log"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -f csv -d "$OUT/prof_sk/trace" -o run -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > "$OUT/prof_sk/bench.json" 2> "$OUT/prof_sk/bench.err"
python3 -c "
import csv, sys
for r in csv.DictReader(open(sys.argv[1] + '/prof_sk/trace/run_kernel_stats.csv')):
    print(r['Name'][:40], r['Calls'], round(float(r['AverageNs'])/1e6,3))
" "$OUT" | head -14
