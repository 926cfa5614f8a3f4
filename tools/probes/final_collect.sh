set -x
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT
python -m pytest tests -q -m gpu -x > $OUT/gpu_tests.log 2>&1; tail -3 $OUT/gpu_tests.log
bash tools/collect_profiles.sh r03 > $OUT/collect.log 2>&1
python bench.py --full > $OUT/r03_bench_default.json 2> $OUT/bench_default.err
python bench.py --full --labels blocky --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r03_bench_blocky.json
python bench.py --full --workload loss --steps 20 --warmup 5 --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r03_bench_loss.json
python bench.py --full --config 4 --steps 8 --warmup 3 --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r03_bench_config4.json
python bench.py --full --config 5 --steps 5 --warmup 2 --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r03_bench_config5.json
python tools/host_vs_gpu.py --lead > $OUT/r03_host_vs_gpu.txt 2>&1
OUT=$OUT python - <<'P'
import json, os
for n in ("default","blocky","loss","config4","config5"):
    try:
        d=json.loads(open(os.path.join(os.environ["OUT"], f"r03_bench_{n}.json")).read().strip().splitlines()[-1])
        print(n, d["ms_per_step"], d["value"], d.get("eager_gpu_step_ms"), d.get("speedup_vs_eager_gpu_step"), d.get("eager_gpu_step_ms_miopen_find"), d["roofline"]["frac"], d["roofline"].get("launch_ms"))
    except Exception as e: print(n, "ERR", e)
P
cat $OUT/r03_host_vs_gpu.txt | tail -3
