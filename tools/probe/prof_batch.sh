# kernel trace of the bench's full batch64 run, GPU box, repo root:  bash tools/probe/prof_batch.sh OUT_DIR
ROOT=$PWD; OUT=$(realpath -m "${1:?usage: bash tools/probe/prof_batch.sh OUT_DIR}"); mkdir -p "$OUT"; export TMPDIR=/tmp; cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_batch -- python3 $ROOT/bench.py --full --workload batch64 --steps 1 --warmup 1 --no-cpu-baseline > "$OUT/prof_batch.log" 2>&1
cd $ROOT
python3 tools/trace_by_grid.py /tmp/prof_batch 0.5 > "$OUT/batch_by_grid_now.txt" 2>&1
