# Time the extract+match leg for the default build and every lib/var_*/ variant
# (tools/build_variants.sh).  Usage: variants.sh [steps]     (writes under $MCS_OUT, default
# bench_out/)
set -o pipefail
cd "$(dirname "$0")/../.."; O=${MCS_OUT:-bench_out}; mkdir -p $O
STEPS=${1:-10}
for L in lib $(cd multicol-slam-annotation_amd && ls -d lib/var_* 2>/dev/null); do
  MCS_AMD_LIB=$PWD/multicol-slam-annotation_amd/$L/libmcs_amd.so timeout -k 10 200 python bench.py --full --steps $STEPS --warmup 2 --no-cpu-baseline --ba-calls 0 --gba-calls 0 --d-multiframes 0 --bow-reps 0 --latency-reps 0 > $O/var.json 2>$O/var.err || { echo "$L failed"; tail -3 $O/var.err; exit 1; }
  python3 -c "import json; d=json.load(open('$O/var.json')); print('$L', d['value'], d['roofline']['frac'], {k: round(v, 3) for k, v in d['stage_ms_per_step'].items()})"
done
