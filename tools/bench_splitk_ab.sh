set -o pipefail
OUT=${OUT:-bench_out}/ab
mkdir -p "$OUT"
for i in 1 2; do
for c in 0 2 1; do
  VO_TUNE=splitk_cfg=$c timeout -k 10 200 python bench.py --full --steps 20 --cpu-seconds 0 --no-kernel-timer > "$OUT/b_${c}_$i.out" 2>&1 || exit 1
  python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('splitk_cfg=$c', d['ms_per_step'])" "$OUT/b_${c}_$i.out"
done; done
