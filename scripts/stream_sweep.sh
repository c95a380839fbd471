set -e
OUT=${SWEEP_OUT:-sweep_out}
mkdir -p "$OUT"
for cfg in "8192 4" "8192 8" "8192 6" "4096 4" "4096 8"; do
  set -- $cfg
  timeout -k 10 120 python bench.py --full --global-envs $1 --streams $2 --no-cpu-baseline --no-secondary --steps 1000 --warmup 100 > "$OUT/e$1_s$2.json" 2> "$OUT/e$1_s$2.err"
done
