# kernel trace of a short config-3 bench run (replayed steps): bash tools/gpu_trace_c3.sh <tag>
set -o pipefail
T=$1
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --stats -T --output-format csv -d $OUT/prof_${T} -o run -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-dropin > $OUT/${T}_trace_bench.log 2>&1 || { tail -20 $OUT/${T}_trace_bench.log; exit 4; }
python3 tools/kseq.py $OUT/prof_${T}/run_kernel_trace.csv 3 | head -12
