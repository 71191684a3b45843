# Full GPU parity suite, smoke, then the default bench line (what the driver runs at round end).
set -e
export OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread "$@" > $OUT/tg.log 2>&1 || { grep -B5 "Error\|assert" $OUT/tg.log | tail -60; tail -5 $OUT/tg.log; exit 1; }
tail -2 $OUT/tg.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -30 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
SECONDS=0; timeout -k 10 600 python bench.py --full > $OUT/bench_default.log 2> $OUT/bench_default.err || { tail -30 $OUT/bench_default.err; exit 1; }
tail -1 $OUT/bench_default.log
echo "bench wall: ${SECONDS}s"
