#!/bin/bash
# The default bench (C5, 65,536 calls on one GPU) + GPU tests matching $PYTEST_K.
set -e
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${SG_OUT:-$R/bench_out}  # where logs and result lines go
cd "$R"
mkdir -p $OUT
TAG=${1:-r02}
if [ -n "$PYTEST_K" ]; then bash tools/gpu_tests.sh; fi
timeout -k 10 ${BENCH_TIMEOUT:-600} python bench.py --full $BENCH_ARGS > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -30 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
