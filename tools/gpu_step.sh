# scratch: the GPU step of the current session's latest gpurun call (round 5).
# The suite runs to the end unless it dies (test failures are read from the log;
# a fault, abort, signal or time limit ends the call), then smoke(), the whole bench
# line (bench.py --full) and the plain one, each under its own time limit. Logs go
# under $LOGS (default: logs/).
#   bash tools/gpu_step.sh r05a
set -o pipefail
TAG=${1:-r05}
LOGS=${LOGS:-logs}
mkdir -p $LOGS
timeout -k 10 900 python -u -m pytest tests -m gpu -q --maxfail=8 -rf --timeout 240 --timeout-method thread > $LOGS/gpu_tests_$TAG.log 2>&1
rc=$?
tail -15 $LOGS/gpu_tests_$TAG.log
[ $rc -le 1 ] || { echo "pytest rc $rc: stopping"; exit $rc; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $LOGS/smoke_$TAG.log 2>&1 || { tail $LOGS/smoke_$TAG.log; exit 1; }
tail -1 $LOGS/smoke_$TAG.log
timeout -k 10 400 python bench.py --full > $LOGS/bench_$TAG.json 2> $LOGS/bench_$TAG.err || { tail $LOGS/bench_$TAG.err; exit 1; }
[ $rc -eq 0 ] || { echo "pytest rc $rc"; exit $rc; }
timeout -k 10 300 python bench.py --steps 20 --warmup 5 > $LOGS/bench_${TAG}_driver.json 2> $LOGS/bench_${TAG}_driver.err || { tail $LOGS/bench_${TAG}_driver.err; exit 1; }
echo bench-ok
if [ -n "${ASAN:-}" ]; then
  ASAN_OPTIONS=detect_leaks=0 timeout -k 10 300 tests/cpp/build/test_checksum_asan --gpu > $LOGS/cpp_asan_$TAG.log 2>&1 || { tail -30 $LOGS/cpp_asan_$TAG.log; exit 1; }
  tail -1 $LOGS/cpp_asan_$TAG.log
fi
if [ -n "${FUZZ_SEED_BASE:-}" ]; then
  bash tools/fuzz_long.sh || exit 1
fi
[ -n "${PROF_CFGS:-}" ] || exit 0
CFGS="$PROF_CFGS" timeout -k 10 900 bash tools/profile.sh $TAG || exit 1
echo prof-ok
