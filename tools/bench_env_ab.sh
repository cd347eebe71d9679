#!/bin/bash
# Bench-level A/B of environment settings: tools/bench_env_ab.sh "VO_RB3=0" "VO_RB3=1" ...
# prints ms/step and the per-stage MRF launch averages for each setting
# (bench.py --full: the per-stage averages come from its roofline pass); files under $OUT
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for c in "$@"; do
  env $c timeout -k 10 150 python bench.py --full --cpu-seconds 0 --steps 20 --no-configs > "$OUT/b.json" 2> "$OUT/b.err" || { tail -5 "$OUT/b.err"; exit 1; }
  python - "$c" "$OUT/b.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
s = d["roofline"]["all_stages"]
print(sys.argv[1], d["ms_per_step"], {k: (v["avg_ms"], v["launches"]) for k, v in s.items()}, flush=True)
PY
done
