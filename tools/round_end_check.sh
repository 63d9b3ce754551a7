# GPU suite, smoke and the complete benchmark line: bash tools/round_end_check.sh [OUT]
OUT=${1:-check_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/ -m gpu > "$OUT/full_t.log" 2>&1 || exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || exit 1
timeout -k 10 600 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err" || exit 1
