cd "$(dirname "$0")/.."
OUT="${OUT:-$PWD/logs}"
mkdir -p "$OUT"
for bp in 0 50 0 50 0 50; do
  timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --no-canary --busy-poll-us $bp > "$OUT/ab_$bp.json.tmp" 2>"$OUT/ab_err.log" || exit $?
  grep '^{' "$OUT/ab_$bp.json.tmp" >> "$OUT/ab_$bp.jsonl"
done
