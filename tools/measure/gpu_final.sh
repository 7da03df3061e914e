#!/bin/bash
# fallback paths under SMK_TUNE + the default bench line with its layer profile
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
cd $R; mkdir -p $OUT
SMK_TUNE=chain=0,halo=0 timeout 600 python -m pytest tests/test_gpu_e2e.py tests/test_gpu_tracker.py -m gpu -x -q --tb=short 2>&1 | grep -v amdgpu.ids | tail -4
timeout 600 python bench.py --full --profile-out $OUT/bench_layers.json > $OUT/bench.json 2> $OUT/bench.err; echo "bench exit $?"
cat $OUT/bench.json
