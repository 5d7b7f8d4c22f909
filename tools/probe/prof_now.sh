# kernel statistics of the bench's full run (timed and per-launch-timed steps), GPU box, repo root:  bash tools/probe/prof_now.sh OUT_DIR
ROOT=$PWD; OUT=$(realpath -m "${1:?usage: bash tools/probe/prof_now.sh OUT_DIR}"); mkdir -p "$OUT"; export TMPDIR=/tmp; cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_bench -- python3 $ROOT/bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > "$OUT/prof_bench.log" 2>&1
cd $ROOT
python3 tools/trace_by_grid.py /tmp/prof_bench 0.5 > "$OUT/bench_by_grid_now.txt" 2>&1
cp $(ls -t /tmp/prof_bench/*/*kernel_stats.csv | head -1) "$OUT/bench_kernel_stats_now.csv"
