set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${SG_OUT:-$R/bench_out}  # where logs and result lines go
cd "$R"
mkdir -p $OUT
PYTEST_K="${PYTEST_K:-envelope or c5}" bash tools/gpu_tests.sh
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p3 -o run -- python "$R/bench.py" --full --config c5 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/p3.log 2>&1
cut -d, -f1-5 $OUT/p3/run_kernel_stats.csv | head -20
