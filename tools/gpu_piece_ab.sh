# Round 6: camera-direction piece length of a rank-of-8 shard (GASFM_MAX_PIECE) -- the proxy
export OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
for P in ${PIECES:-64 48 64 48 64 48}; do
  if [ "$P" = 0 ]; then unset GASFM_MAX_PIECE; else export GASFM_MAX_PIECE=$P; fi; timeout -k 10 200 python bench.py --full --emulate-world 8 --no-cpu-baseline --steps 20 --warmup 3 > $OUT/piece_em8.json 2> $OUT/piece_em8.err || { tail -20 $OUT/piece_em8.err; exit 1; }
  python -c "import json;d=json.loads(open('$OUT/piece_em8.json').read().strip().splitlines()[-1]);print('piece $P', round(d['ms_per_step'],3), 'pbwd', round(d['roofline']['mean_us'],1))"
done
