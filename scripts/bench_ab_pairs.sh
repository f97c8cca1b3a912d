#!/bin/bash
# Alternating pairs of the default benchmark with two prebuilt libraries, one JSON line per run:
#   scripts/bench_ab_pairs.sh <parent.so> <new.so> <out.jsonl> [pairs=8]
# Every run is `python bench.py --gpus 1 --steps 200 --warmup 8` with LSA_LIB selecting the library, under a time limit of
# its own; the first run that fails ends the series.  The line is bench.py's result line with "lib": "parent" | "new" put
# in front.  Acceptance (ms_per_icp_iter): every new run below every parent run and the medians apart by 3 x the
# parent's own spread -- printed at the end.
A=$1; B=$2; OUT=$3; PAIRS=${4:-8}
: > "$OUT"
for ((i = 0; i < PAIRS; ++i)); do
  for v in parent new; do
    lib=$A; [ $v = new ] && lib=$B
    line=$(LSA_LIB=$lib timeout -k 10 240 python bench.py --gpus 1 --steps 200 --warmup 8 2>/dev/null | tail -n 1) || { echo "run $i $v failed" >&2; exit 1; }
    python -c "
import json, sys
d = json.loads(sys.argv[1])
print(json.dumps({'lib': sys.argv[2], **d}))" "$line" "$v" >> "$OUT" || exit 1
  done
done
python - "$OUT" <<'PY'
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1])]
p = [1e3 * r["ms_per_icp_iter"] for r in rows if r["lib"] == "parent"]
n = [1e3 * r["ms_per_icp_iter"] for r in rows if r["lib"] == "new"]
spread = max(p) - min(p)
gain = statistics.median(p) - statistics.median(n)
print("us per ICP iteration  parent", [round(v, 2) for v in p], " new", [round(v, 2) for v in n])
print("medians %.2f -> %.2f, gain %.2f us = %.1f x the parent's spread (%.2f); every new below every parent: %s" % (
    statistics.median(p), statistics.median(n), gain, gain / spread if spread else float("inf"), spread, max(n) < min(p)))
print("frames/s medians %.1f -> %.1f" % (statistics.median(r["value"] for r in rows if r["lib"] == "parent"), statistics.median(r["value"] for r in rows if r["lib"] == "new")))
for key in ("device_solve_fallbacks", "icp_gate_timeouts"):
    print(key, sorted({r["config"][key] for r in rows}))
PY
