# LocalBA kernel timeline: per-kernel device time and the idle gaps of the last 3 calls.
set -o pipefail
cd "$(dirname "$0")/../.."; G=${MCS_OUT:-bench_out}; mkdir -p $G; export TMPDIR=/tmp
TAG=${1:-x}
timeout -k 10 120 python3 tools/gpu/lba_gaps.py 200 > $G/lba_wall_$TAG.log 2>&1 || { tail -5 $G/lba_wall_$TAG.log; exit 1; }
cat $G/lba_wall_$TAG.log
timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $G/lbag_$TAG -o run -- python3 tools/gpu/lba_gaps.py 3 > $G/lbag_$TAG.log 2>&1 || { tail -5 $G/lbag_$TAG.log; exit 1; }
T=$(find $G/lbag_$TAG -name '*kernel_trace.csv' | head -1)
python3 tools/ktrace_gaps.py "$T" 3 | tee $G/lba_gaps_$TAG.txt
