# round-5 bench evidence (GPU box, repo root):  bash tools/probe/final_evidence.sh OUT_DIR
OUT=${1:?usage: bash tools/probe/final_evidence.sh OUT_DIR}; mkdir -p "$OUT"
python bench.py --full > "$OUT/r05_bench_line.json" 2> "$OUT/r05_bench_line.err"
tail -c 400 "$OUT/r05_bench_line.err"
BENCH_SHARE_GPU=1 python bench.py --full --gpus 2 --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/r05_bench_gpus2_shared_gpu.json" 2> "$OUT/r05_bench_gpus2.err"
tail -c 300 "$OUT/r05_bench_gpus2_shared_gpu.json"
BENCH_FORCE_DIST=1 python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > "$OUT/r05_bench_forced_dist.json" 2> "$OUT/r05_bench_forced_dist.err"
tail -c 300 "$OUT/r05_bench_forced_dist.json"
python bench.py --full --workload batch64 --no-cpu-baseline > "$OUT/r05_bench_batch64.json" 2>/dev/null
tail -c 400 "$OUT/r05_bench_batch64.json"
