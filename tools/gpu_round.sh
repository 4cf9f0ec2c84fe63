# The record of a build on the GPU box: pytest -m gpu, bench.py --full, smoke().
# Usage: bash tools/gpu_round.sh [LOG_DIR]   (logs go to LOG_DIR, default: logs)
OUT=${1:-logs}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -q -s > "$OUT"/gputest.log 2>&1; echo "pytest rc=$?" >> "$OUT"/gputest.log
grep -E "passed|failed|error" "$OUT"/gputest.log | tail -n 5
grep -E "^FAILED|^k = |at-scale" "$OUT"/gputest.log | head -20
timeout 900 python bench.py --full > "$OUT"/bench.log 2> "$OUT"/bench.err; echo "bench rc=$?" >> "$OUT"/bench.err
tail -n 2 "$OUT"/bench.err
tail -n 1 "$OUT"/bench.log | head -c 6500
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT"/smoke.log 2>&1; tail -n 3 "$OUT"/smoke.log
