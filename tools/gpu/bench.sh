# bench.py --full line only
set -o pipefail
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u bench.py --full > "$OUT"/bench.log 2>&1 && echo bench-ok && tail -1 "$OUT"/bench.log | cut -c1-200
