#!/bin/bash
# full parity suite + default bench line + rocprofv3 kernel stats + PMC passes (separate runs)
R=$(cd "$(dirname "$0")/../.." && pwd)
export OUT=${MEASURE_OUT:-$R/measure_out}
cd $R; mkdir -p $OUT
timeout 900 python -m pytest tests -m gpu -x -q --tb=short 2>&1 | grep -v amdgpu.ids | tail -8
timeout 600 python bench.py --full --profile-out $OUT/bench_layers.json > $OUT/bench.json 2> $OUT/bench.err; echo "bench exit $?"
cat $OUT/bench.json
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof
timeout 300 rocprofv3 --kernel-trace --stats -f csv -d $OUT/prof -- python $R/bench.py --full --steps 20 --warmup 5 --prewarm-seconds 0.3 --no-cpu-baseline --no-also > $OUT/rocprof_bench.json 2> $OUT/rocprof.err
echo "rocprof exit $?"
find $OUT/prof -name "*kernel_trace.csv" -delete
cd $R
[ -n "$NO_PMC" ] || bash tools/measure/gpu_pmc.sh "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU GRBM_GUI_ACTIVE" "FETCH_SIZE TCC_HIT_sum" "WRITE_SIZE TCC_MISS_sum TCC_REQ_sum" 2>&1 | tail -40
