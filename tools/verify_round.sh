#!/bin/bash
# Round-end verification on a GPU box: the GPU parity tests, smoke(), and the whole
# bench line (bench.py --full: side configs, host-memory path, CPU baseline and the
# oracle parity check). Each step has its own time limit; the first failure ends
# the script. Logs go under $LOGS (default: logs/).
#   bash tools/verify_round.sh <tag>
set -o pipefail
TAG=${1:-final}
LOGS=${LOGS:-logs}
mkdir -p "$LOGS"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 240 --timeout-method thread > "$LOGS/gpu_tests_$TAG.log" 2>&1 || { tail -40 "$LOGS/gpu_tests_$TAG.log"; exit 1; }
tail -1 "$LOGS/gpu_tests_$TAG.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$LOGS/smoke_$TAG.log" 2>&1 || { tail "$LOGS/smoke_$TAG.log"; exit 1; }
tail -1 "$LOGS/smoke_$TAG.log"
timeout -k 10 400 python bench.py --full > "$LOGS/bench_$TAG.json" 2> "$LOGS/bench_$TAG.err" || { tail "$LOGS/bench_$TAG.err"; exit 1; }
echo ok
