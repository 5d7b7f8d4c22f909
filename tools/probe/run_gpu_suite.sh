# GPU box, repo root:  bash tools/probe/run_gpu_suite.sh OUT_DIR  (the GPU tests, then one full bench line, summarised)
OUT=${1:?usage: bash tools/probe/run_gpu_suite.sh OUT_DIR}; mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > "$OUT/suite_tests.txt"; cat "$OUT/suite_tests.txt"
python bench.py --full > "$OUT/suite_bench.json" 2> "$OUT/suite_bench.err"; OUT="$OUT" python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ["OUT"], "suite_bench.json")).read().strip().splitlines()[-1])
print({k:d[k] for k in ("value","ms_per_step")}, d["roofline"]["frac"], d["profile"])
print([ (r["workload"], r["lobpcg_iterations"], round(r["ms"])) for r in d.get("scan_like",[])])
print([ (r["workload"], r["lobpcg_iterations"], round(r["ms"])) for r in d.get("config3",[])])
print(d.get("concurrent_solves"), d.get("batch64"))
PY
