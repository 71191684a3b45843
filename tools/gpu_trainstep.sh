# scene-build / outlier / batch / loss parity tests, then the config-3 and config-5 training-step
# benches, the rank-0-of-8 proxy and a short config-4 bench line
set -e
export OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gpu_scene_device.py tests/test_gpu_outliers.py tests/test_gpu_batch.py tests/test_gpu_train_step.py tests/test_gpu_model.py tests/test_gpu_esfm_loss.py tests/test_distributed.py > $OUT/t_ts.log 2>&1 || { tail -30 $OUT/t_ts.log; exit 1; }
tail -1 $OUT/t_ts.log
timeout -k 10 300 python tools/train_step_bench.py --steps 6 > $OUT/tsb_c3.log 2>&1
grep ms_per_step $OUT/tsb_c3.log | cut -c1-400
timeout -k 10 300 python tools/train_step_bench.py --steps 6 --outliers 0.1 > $OUT/tsb_c5.log 2>&1
grep ms_per_step $OUT/tsb_c5.log | cut -c1-400
timeout -k 10 300 python bench.py --emulate-world 8 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/em8.json 2>/dev/null
python -c "import json;d=json.loads(open('$OUT/em8.json').read().strip().splitlines()[-1]);print('emulated rank 0 of 8:', round(d['ms_per_step'],3))"
timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/bench_rf.json 2> $OUT/bench_rf.err || { tail -20 $OUT/bench_rf.err; exit 1; }
python -c "import json;d=json.loads(open('$OUT/bench_rf.json').read().strip().splitlines()[-1]);print(d['ms_per_step'], json.dumps(d['roofline'])[:300])"
