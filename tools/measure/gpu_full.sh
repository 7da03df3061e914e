#!/bin/bash
# full GPU test-suite + bench variants
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
cd $R; mkdir -p $OUT/full
python -m pytest tests -m gpu -q --tb=short > $OUT/full/pytest.log 2>&1; echo "pytest exit $?" >> $OUT/full/pytest.log
tail -15 $OUT/full/pytest.log
i=0
for ARGS in "$@"; do
  i=$((i+1))
  python bench.py --full --no-cpu-baseline --no-also $ARGS --profile-out $OUT/full/layers_$i.json > $OUT/full/bench_$i.json 2> $OUT/full/err_$i.log
  python - <<PY
import json
try:
    d=json.load(open("$OUT/full/bench_$i.json"))
    print("$ARGS ->", d["value"], "fps", d["ms_per_step"], "ms/step  conv TF", d["roofline"]["achieved"], "kernel ms", d["roofline"]["kernel_ms_per_step"])
except Exception as e:
    print("$ARGS FAILED", e); print(open("$OUT/full/err_$i.log").read()[-1500:])
PY
done
