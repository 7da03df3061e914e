#!/bin/bash
# smoke + bench (with per-layer launch profile) + rocprofv3 kernel trace of the same command.
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
mkdir -p $OUT
cd $R
python __graft_entry__.py smoke > $OUT/smoke.log 2>&1; echo "smoke exit $?" >> $OUT/smoke.log
python bench.py --full --steps ${STEPS:-50} --warmup 10 --profile-out $OUT/bench_layers.json > $OUT/bench.json 2> $OUT/bench.err
echo "bench exit $?" >> $OUT/bench.err
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof
timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $OUT/prof -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-also > $OUT/rocprof_bench.json 2> $OUT/rocprof.err
echo "rocprof exit $?" >> $OUT/rocprof.err
# keep only the small summaries (the raw kernel trace can be large)
find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
cd $R; tail -3 $OUT/smoke.log; cat $OUT/bench.json; tail -3 $OUT/bench.err
