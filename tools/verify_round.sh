#!/bin/bash
# What the round-end driver runs, in one place.  Here (no GPU):   bash tools/verify_round.sh cpu
# On an MI355X box (bash tools/verify_round.sh gpu [output dir, default build/verify]): GPU tests, smoke, the plain and the --full bench
# line, every configuration.
# Every step's exit status counts: the script stops with status 1 at the first failing step.
set -u -o pipefail
cd "$(dirname "$0")/.."
mode=${1:-cpu}
if [ "$mode" = cpu ]; then
  python -c "import __graft_entry__ as g; g.build(); print('build ok')" || exit 1
  python -m pytest tests -x -q -m "not gpu" || exit 1
else
  out=${2:-build/verify}
  mkdir -p "$out"
  python -m pytest tests -x -q -m gpu 2>&1 | tail -25 || exit 1
  python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 || exit 1
  python bench.py > "$out/verify_bench.json" 2> "$out/verify_bench.err" || { tail -5 "$out/verify_bench.err"; exit 1; }
  cut -c1-200 "$out/verify_bench.json"
  python bench.py --full > "$out/verify_bench_full.json" 2> "$out/verify_bench_full.err" || { tail -5 "$out/verify_bench_full.err"; exit 1; }
  cut -c1-200 "$out/verify_bench_full.json"
  for c in c3 c4 c5 eval; do
    python bench.py --config $c 2> "$out/verify_$c.err" > "$out/verify_$c.json" || { tail -5 "$out/verify_$c.err"; exit 1; }
    grep -o '"name": "[a-z0-9]*"\|"value": [0-9.]*\|"ms_per_step": [0-9.]*' "$out/verify_$c.json" | tr '\n' ' '; echo
  done
fi
