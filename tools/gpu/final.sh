# round evidence, part 1: GPU parity suite, smoke, the bench.py --full line
set -o pipefail
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT"/gputest.log 2>&1 && echo tests-ok && tail -1 "$OUT"/gputest.log &&
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print(\"smoke ok\")" > "$OUT"/smoke.log 2>&1 && echo smoke-ok &&
timeout -k 10 500 python -u bench.py --full > "$OUT"/bench.log 2>&1 && echo bench-ok && tail -1 "$OUT"/bench.log | cut -c1-300
