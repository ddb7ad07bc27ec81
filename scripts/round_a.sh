#!/bin/bash
# Round artefacts, part A (GPU box): the full -m gpu suite and the full bench line.
# usage: bash scripts/round_a.sh TAG   (part B: scripts/round_b.sh TAG -- kernel stats + PMC passes)
# Results go to $OUT (default out/).
TAG=${1:-r4}
OUT=${OUT:-out}
export TMPDIR=/tmp
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1
rc=$?; tail -3 $OUT/${TAG}_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python3 bench.py --full > $OUT/${TAG}_bench.log 2>&1 || { echo "bench failed"; tail -5 $OUT/${TAG}_bench.log; exit 1; }
tail -1 $OUT/${TAG}_bench.log > $OUT/${TAG}_bench_line.json
echo done
