#!/bin/bash
# GPU box: rocprofv3 kernel stats of one Parakeet workload (PK_BENCH_ONLY=offline|stream).
# Results go to $OUT (default out/).
set -o pipefail
W=${1:-offline}; TAG=${2:-pkw}
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p "$OUT"
PK_BENCH_ONLY=$W timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- \
  python3 bench.py --full --parakeet-only --no-cpu-baseline --steps 3 --warmup 1 > $OUT/${TAG}_prof.log 2>&1 || { echo "rocprof failed"; exit 1; }
f=$(find $OUT/${TAG}_prof -name "*kernel_stats.csv" | head -1)
cp "$f" $OUT/${TAG}_kernel_stats.csv
python3 - "$TAG" "$OUT" <<'PY'
import csv, sys
tag, out = sys.argv[1], sys.argv[2]
rows = list(csv.DictReader(open(f"{out}/{tag}_kernel_stats.csv")))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
with open(f"{out}/{tag}_kernel_top.txt", "w") as f:
    for r in rows[:22]:
        line = f'{float(r["TotalDurationNs"])/tot*100:6.2f}% {int(r["Calls"]):7d} {float(r["AverageNs"])/1e3:9.2f}us  {r["Name"][:110]}'
        print(line); f.write(line + "\n")
PY
find $OUT/${TAG}_prof -name "*.csv" ! -name "*kernel_stats.csv" -delete
