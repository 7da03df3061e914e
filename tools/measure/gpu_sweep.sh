#!/bin/bash
# A/B sweep of library tuning knobs: one bench run (with per-layer profile) per setting.
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
cd $R; mkdir -p $OUT/sweep
python -m pytest tests -m gpu -q --tb=short -x -k "ops or fp32_matches" > $OUT/sweep/pytest.log 2>&1; echo "pytest exit $?" >> $OUT/sweep/pytest.log
tail -3 $OUT/sweep/pytest.log
i=0
for T in "$@"; do
  i=$((i+1))
  python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-also --tune "$T" ${WL:+--workload $WL} --profile-out $OUT/sweep/layers_$i.json > $OUT/sweep/bench_$i.json 2> $OUT/sweep/err_$i.log
  echo "$T" > $OUT/sweep/tune_$i.txt
  python - <<PY
import json
try:
    d=json.load(open("$OUT/sweep/bench_$i.json"))
    print("$T", d["value"], "fps", d["ms_per_step"], "ms/step  conv TF", d["roofline"]["achieved"], "kernel ms", d["roofline"]["kernel_ms_per_step"])
except Exception as e:
    print("$T FAILED", e)
PY
done
