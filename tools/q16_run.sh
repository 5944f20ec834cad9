#!/bin/bash
# GPU suite (incl. the 16-bit pass-1 tests) + a kernel trace of the bench.
# Results land in $OUT_DIR (default: bench_out/).
set -euo pipefail
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 1000 python3 -m pytest tests -m gpu -q -x > "$OUT/q16_tests.log" 2>&1
timeout -k 10 400 rocprofv3 --kernel-trace --stats -f csv -d "$OUT/prof_q16/trace" -o run -- \
    python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > "$OUT/q16_bench.json" 2> "$OUT/q16_bench.err"
