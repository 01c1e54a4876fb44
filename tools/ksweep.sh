# per-step time vs the number of timed steps (fixed pipeline fill/drain cost), one box
cd "$(dirname "$0")/.."; OUT=${LSLAM_OUT:-bench_out}; mkdir -p $OUT
for k in 20 50 100 20; do
  timeout -k 10 200 python -u bench.py --full --steps $k --warmup 3 --no-cpu-baseline --no-alone > $OUT/ks.json 2> $OUT/ks.err || { tail -5 $OUT/ks.err; exit 1; }
  echo "K=$k $(python3 -c "import json; d=json.load(open('$OUT/ks.json')); print(d['ms_per_step'], d['roofline']['kernel_ms'])")"
done
