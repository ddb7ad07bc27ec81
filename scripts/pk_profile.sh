#!/bin/bash
# GPU box: Parakeet-V3 bench line + rocprofv3 kernel stats of the same workload.
# Results go to $OUT (default out/).
set -o pipefail
TAG=${1:-pk}
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout -k 10 400 python -u bench.py --full --parakeet-only --steps 5 --warmup 1 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -20 $OUT/${TAG}_bench.err; exit 1; }
tail -c 2500 $OUT/${TAG}_bench.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- \
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
    for r in rows[:25]:
        line = f'{float(r["TotalDurationNs"])/tot*100:6.2f}% {int(r["Calls"]):7d} {float(r["AverageNs"])/1e3:9.2f}us  {r["Name"][:150]}'
        print(line); f.write(line + "\n")
PY
find $OUT/${TAG}_prof -name "*.csv" ! -name "*kernel_stats.csv" -delete
