# LocalBA leg only (config C), three back-to-back bench runs: ms per call and host phases.
# Writes under $MCS_OUT (default bench_out/).
set -o pipefail
cd "$(dirname "$0")/../.."; O=${MCS_OUT:-bench_out}; mkdir -p $O
for i in 1 2 3; do
timeout -k 10 200 python bench.py --full --multiframes 2 --unique 2 --steps 1 --warmup 1 --no-cpu-baseline --ba-calls 40 --gba-calls 0 --d-multiframes 0 --bow-reps 0 --latency-reps 0 --tri-reps 0 > $O/lba_b.json 2> $O/lba_b.err || { tail -5 $O/lba_b.err; exit 1; }
python3 -c "import json; d=json.load(open('$O/lba_b.json'))['localba']; print(d['ms_per_call'], d['host_ms_per_call'])"
done
