#!/bin/bash
# The round's bench lines (--full: rooflines, comparators) + suite + smoke on one GPU box:  bash tools/probes/final_lines.sh r05 [OUT]
# OUT (default bench_out/) receives <tag>_bench_*.json
T=${1:-r05}
cd ${GRAFT_REPO_ROOT:-.}
OUT=${2:-bench_out}; mkdir -p $OUT
python -m pytest tests -q -m gpu 2>&1 | tail -1
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1
python bench.py --full --detail-file $OUT/${T}_bench_default_detail.json 2>/dev/null | tail -1 > $OUT/${T}_bench_default.json
python bench.py --full --workload loss 2>/dev/null | tail -1 > $OUT/${T}_bench_loss.json
python bench.py --full --labels blocky --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/${T}_bench_blocky.json
python bench.py --full --config 4 --steps 10 --warmup 3 --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/${T}_bench_config4.json
python bench.py --full --config 5 --steps 10 --warmup 3 --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/${T}_bench_config5.json
for f in default loss blocky config4 config5; do python - <<PY
import json
d = json.load(open("$OUT/${T}_bench_$f.json"))
print("$f", d["ms_per_step"], d["value"], d.get("contrastive_loss_fwd_bwd_ms"), (d.get("roofline") or {}).get("frac"), len(json.dumps(d)))
PY
done
