# The GPU suite, then the whole benchmark (--full).  Writes under $MCS_OUT (default bench_out/).
set -o pipefail
cd "$(dirname "$0")/../.."; O=${MCS_OUT:-bench_out}; mkdir -p $O
TAG=${1:-x}
timeout -k 10 600 python -u -m pytest tests/ -x -v -m gpu --timeout 120 --timeout-method thread > $O/tests_$TAG.log 2>&1; rc=$?; echo "TESTS EXIT $rc" >> $O/tests_$TAG.log
tail -15 $O/tests_$TAG.log
[ $rc -eq 0 ] || exit 1
timeout -k 10 400 python bench.py --full ${BENCH_ARGS:---steps 10 --warmup 2} > $O/bench_$TAG.json 2> $O/bench_$TAG.err; rc=$?; echo "BENCH EXIT $rc"
cat $O/bench_$TAG.json; tail -3 $O/bench_$TAG.err
[ $rc -eq 0 ] || exit 1
if [ -n "$PROFILE" ]; then bash tools/gpu/profile.sh $TAG; fi
