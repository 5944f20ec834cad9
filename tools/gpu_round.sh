#!/bin/bash
# Full GPU suite, then the round profile (trace + FETCH/WRITE + SQ) and one full
# bench line (bench.py --full).  Results land in $OUT_DIR (default: bench_out/).
set -euo pipefail
TAG=${1:-r01}
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
timeout -k 10 900 python3 -m pytest tests -m gpu -q -x > "$OUT/gpu_tests_${TAG}.log" 2>&1
bash tools/profile_round.sh "$TAG"
bash tools/pmc_sq.sh "$TAG"
timeout -k 10 400 python3 bench.py --full > "$OUT/bench_${TAG}.json" 2> "$OUT/bench_${TAG}.err"
