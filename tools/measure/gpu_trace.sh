#!/bin/bash
# rocprofv3 kernel trace of the bench in graph-replay mode -> per-kernel durations and gaps
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
cd $R; mkdir -p $OUT
python bench.py --full --steps 50 --warmup 10 --no-cpu-baseline ${ALSO:---no-also} --tune "${TUNE:-stages=0}" --profile-out $OUT/bench_layers.json > $OUT/bench.json 2> $OUT/bench.err
cat $OUT/bench.json | head -c 1500; echo
cd /tmp && export TMPDIR=/tmp; rm -rf $OUT/prof
timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $OUT/prof -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-also --tune "${TUNE:-stages=0}" > $OUT/rocprof_bench.json 2> $OUT/rocprof.err
cd $R
python tools/measure/trace_stats.py $(ls $OUT/prof/*/*kernel_trace.csv | head -1)
find $OUT/prof -name "*kernel_trace.csv" -size +8M -delete
