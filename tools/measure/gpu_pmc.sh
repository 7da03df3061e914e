#!/bin/bash
# PMC passes (separate runs, kernel-trace only -- never with sys/hip traces) for the bench step.
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
cd $R; mkdir -p $OUT/pmc
rocprofv3 -L > $OUT/pmc/counters_list.txt 2>&1
# --serial: counter collection serialises the dispatches of ALL queues, which the pipelined step's gate kernels cannot survive (a gate waits
# for a kernel of the other queue that the profiler will not start before the gate ends: 0.2 s time-outs, the persistent launches behind the
# raised flag return at once and pollute every per-kernel average -- seen in round 5's first final run: 159 MB "per launch" instead of 647)
CMD="python $R/bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-also --no-long --serial --prewarm-seconds 0.3 ${WL:+--workload $WL}"
cd /tmp && export TMPDIR=/tmp
i=0
for SET in "$@"; do
  i=$((i+1))
  rm -rf $OUT/pmc/pass$i
  timeout 150 rocprofv3 --pmc $SET --kernel-trace -f csv -d $OUT/pmc/pass$i -- $CMD > $OUT/pmc/pass$i.out 2> $OUT/pmc/pass$i.err
  echo "pass $i [$SET] exit $?"
done
cd $R
python tools/measure/pmc_stats.py $OUT/pmc
# drop raw traces that are too large to bring back
find $OUT/pmc -name "*.csv" -size +12M -delete
