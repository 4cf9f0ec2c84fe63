# bench (every leg: --full) + smoke only (the full round script is tools/gpu_round.sh); logs go
# to the directory given as $1 (default: logs)
OUT=${1:-logs}
mkdir -p "$OUT"
timeout 900 python bench.py --full > "$OUT"/bench.log 2> "$OUT"/bench.err; echo "bench rc=$?" >> "$OUT"/bench.err
tail -n 2 "$OUT"/bench.err
tail -n 1 "$OUT"/bench.log | head -c 6500
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT"/smoke.log 2>&1; tail -n 3 "$OUT"/smoke.log
