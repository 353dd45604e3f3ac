ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
OUT="${OUT:-$ROOT/prof_out}"
mkdir -p "$OUT"
for pl in 1 2 0; do
  cd /tmp && export TMPDIR=/tmp
  FFTCONV_PLANES=$pl timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/r2_planes3_${pl}_trace" -- python3 "$ROOT/bench.py" --full --config cfgC --steps 40 --warmup 5 --no-cpu-baseline --no-end-to-end > "$OUT/r2_planes3_${pl}_trace.log" 2>&1
  cd "$ROOT"
  echo "== FFTCONV_PLANES=$pl"; python3 scripts/summarize_prof.py "$OUT" r2_planes3_${pl} | grep "fc::" | cut -c1-110
  grep "\"metric\"" "$OUT/r2_planes3_${pl}_trace.log" | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print('bench', round(d['roofline']['kernel_us'],1), 'us')"
done
