#!/bin/bash
# Bench-level A/B of tuning knobs: tools/bench_ab.sh "pair_cfg=93" "pair_cfg=0" ...
# prints ms/step and the per-stage MRF launch averages for each VO_TUNE setting
# (bench.py --full: the per-stage averages come from its roofline pass); files under $OUT
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for c in "$@"; do
  VO_TUNE="$c" timeout -k 10 150 python bench.py --full --cpu-seconds 0 --steps 20 --no-configs > "$OUT/b.json" 2> "$OUT/b.err" || { tail -5 "$OUT/b.err"; exit 1; }
  python - "$c" "$OUT/b.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
s = d["roofline"]["all_stages"]
print(sys.argv[1], d["ms_per_step"], {k: v["avg_ms"] for k, v in s.items()}, flush=True)
PY
done
