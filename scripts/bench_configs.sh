set -u
OUT=${1:-bench_out/cfgs}
mkdir -p "$OUT"
T0=$(date +%s)
for C in C1 C2 C3; do
  timeout 100 python bench.py --full --config $C --out "$OUT/bench_$C.json" > /dev/null 2> "$OUT/bench_$C.err"
  echo "$C rc=$? at $(( $(date +%s) - T0 )) s" >> "$OUT/steps.log"
done
cat "$OUT/steps.log"
