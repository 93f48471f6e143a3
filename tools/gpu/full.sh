# full GPU check: parity suite, then the bench.py --full line (round-end driver order)
set -o pipefail
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT"/gputest.log 2>&1 && echo tests-ok &&
timeout -k 10 400 python -u bench.py --full > "$OUT"/bench.log 2>&1 && echo bench-ok && tail -1 "$OUT"/bench.log
