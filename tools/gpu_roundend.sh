# What the driver runs at round end: smoke, then the default bench (with the CPU baseline).
set -e
export OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1 || { tail -30 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
SECONDS=0; timeout -k 10 900 python bench.py --full > $OUT/bench_default.log 2> $OUT/bench_default.err || { tail -30 $OUT/bench_default.err; exit 1; }
tail -1 $OUT/bench_default.log
echo "bench wall: ${SECONDS}s"
