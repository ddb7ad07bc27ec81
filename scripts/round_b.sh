#!/bin/bash
# Round artefacts, part B (GPU box): rocprofv3 kernel-trace stats of the bench command, then the
# PMC traffic passes (scripts/pmc.sh).  usage: bash scripts/round_b.sh TAG
# Results go to $OUT (default out/); the PMC passes keep their own folder.
TAG=${1:-r4}
OUT=${OUT:-out}
export TMPDIR=/tmp
mkdir -p "$OUT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- \
    python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-app-latency --no-probe > $OUT/${TAG}_prof.log 2>&1 || { echo "rocprof failed"; exit 1; }
rm -f $OUT/${TAG}_prof/run_kernel_trace.csv
bash scripts/pmc.sh ${TAG} || exit 1
echo done
