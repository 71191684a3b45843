# same-box A/B of an environment knob on the default bench: bash tools/gpu_ab_env.sh VAR valA valB [bench args]
V=$1; A=$2; B=$3; shift 3
export OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
for r in 1 2; do
  for val in "$A" "$B"; do
    env $V=$val timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 20 "$@" > $OUT/ab_env.json 2> $OUT/ab_env.err || { tail -20 $OUT/ab_env.err; exit 1; }
    python -c "import json;r=json.load(open('$OUT/ab_env.json'));print('$V=$val', round(r['ms_per_step'],3), 'ms', 'pbwd', round(r['roofline']['mean_us'],1))"
  done
done
