# GPU tests of the given files, then config 4 and the 1/8 proxy bench (graph replay)
set -e
export OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest "$@" -x -q --timeout 120 --timeout-method thread > $OUT/tf.log 2>&1 || { grep -B5 "Error\|assert" $OUT/tf.log | tail -40; exit 1; }
tail -1 $OUT/tf.log
for n in 200000 25000; do
  timeout -k 10 300 python bench.py --full --points $n --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bf_$n.log 2>$OUT/bf_$n.err || { tail -20 $OUT/bf_$n.err; exit 1; }
  python -c "import json;d=json.loads(open('$OUT/bf_$n.log').read().strip().splitlines()[-1]);print('n=$n', round(d['ms_per_step'],3), d['execution'][:20], 'frac', round(d['roofline']['frac'],3))"
done
