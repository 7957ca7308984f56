# rocprofv3 passes for the bench workload (kernel trace + stats, then separate PMC passes).
set -o pipefail
cd "$(dirname "$0")/../.."; G=${MCS_OUT:-bench_out}; mkdir -p $G
export TMPDIR=/tmp
TAG=${1:-r01}
ARGS="--full --steps 5 --warmup 1 --no-cpu-baseline --ba-calls 3"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $G/prof_$TAG/stats -o run -- python3 bench.py $ARGS > $G/prof_${TAG}_stats.log 2>&1 || { echo "stats pass failed"; tail -20 $G/prof_${TAG}_stats.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $G/prof_$TAG/fetch -o run -- python3 bench.py $ARGS > $G/prof_${TAG}_fetch.log 2>&1 || { echo "fetch pass failed"; tail -20 $G/prof_${TAG}_fetch.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $G/prof_$TAG/write -o run -- python3 bench.py $ARGS > $G/prof_${TAG}_write.log 2>&1 || { echo "write pass failed"; tail -20 $G/prof_${TAG}_write.log; exit 1; }
find $G/prof_$TAG -name '*.csv' | head -20
F=$(find $G/prof_$TAG/fetch -name '*counter_collection.csv' | head -1)
W=$(find $G/prof_$TAG/write -name '*counter_collection.csv' | head -1)
python3 tools/pmc_traffic.py "$F" "$W" $G/prof_$TAG/pmc_traffic.json > /dev/null && echo "traffic ok"
S=$(find $G/prof_$TAG/stats -name '*kernel_stats.csv' | head -1)
cp "$S" $G/prof_$TAG/kernel_stats.csv && head -30 $G/prof_$TAG/kernel_stats.csv
