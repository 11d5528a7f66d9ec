#!/bin/bash
# Round-3 evidence (run from the repo root on the GPU box): bench lines + per-layer tables, rocprofv3 kernel stats, PMC traffic
# passes (fp16 and INT8), MFMA-busy / effective clock and the SQ wave-cycle breakdown of the conv kernels.
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out
B="--steps 20 --warmup 5"
python3 $R/bench.py --full $B --layers > $O/r03_bench_default.json 2> $O/r03_layers.txt; echo "bench default $?"
python3 $R/bench.py --full --int8 $B --layers --no-cpu-baseline --no-dispatcher > $O/r03_int8_bench.json 2> $O/r03_int8_layers.txt; echo "bench int8 full $?"
python3 $R/bench.py --full --int8 --int8-recipe mixed $B --no-cpu-baseline --no-dispatcher > $O/r03_int8_mixed_bench.json 2> /dev/null; echo "bench int8 mixed $?"
python3 $R/bench.py --full --int8 --int8-predequantize $B --no-cpu-baseline --no-dispatcher > $O/r03_int8_predeq_bench.json 2> /dev/null; echo "bench int8 predeq $?"
cd /tmp && export TMPDIR=/tmp
Q="--no-cpu-baseline --no-int8-extra --no-dispatcher"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/r03f_kt -o p -- python3 $R/bench.py --full $B $Q > $O/r03f_kt.json 2> $O/r03f_kt.err; echo "kt $?"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/r03f_kt_i8 -o p -- python3 $R/bench.py --full --int8 $B $Q > $O/r03f_kt_i8.json 2> $O/r03f_kt_i8.err; echo "kt i8 $?"
for ctr in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $O/r03f_pmc_$ctr -o p -- python3 $R/bench.py --full --steps 3 --warmup 1 $Q > $O/r03f_pmc_$ctr.log 2>&1; echo "pmc $ctr $?"
  rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $O/r03f_pmc_i8_$ctr -o p -- python3 $R/bench.py --full --int8 --steps 3 --warmup 1 $Q > $O/r03f_pmc_i8_$ctr.log 2>&1; echo "pmc i8 $ctr $?"
done
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/r03f_mfma -o p -- python3 $R/bench.py --full --steps 3 --warmup 1 $Q > $O/r03f_mfma.log 2>&1; echo "pmc mfma $?"
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE --output-format csv -d $O/r03f_sq -o p -- python3 $R/bench.py --full --steps 3 --warmup 1 $Q > $O/r03f_sq.log 2>&1; echo "pmc sq $?"
cd $R
f() { find $O/$1 -name "*$2" | head -1; }
python3 tools/pmc_to_json.py $(f r03f_pmc_FETCH_SIZE counter_collection.csv) $(f r03f_pmc_WRITE_SIZE counter_collection.csv) $O/pmc_traffic.json "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) of \`bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-int8-extra --no-dispatcher\`, r03 final build" > /dev/null
python3 tools/pmc_to_json.py $(f r03f_pmc_i8_FETCH_SIZE counter_collection.csv) $(f r03f_pmc_i8_WRITE_SIZE counter_collection.csv) $O/pmc_traffic_int8.json "the same passes of \`bench.py --int8 ...\`, r03 final build" > /dev/null
python3 tools/mfma_util.py $(f r03f_mfma counter_collection.csv) $(f r03f_mfma kernel_trace.csv) $O/r03_mfma_util.json > $O/r03_mfma_util.txt
python3 tools/sq_breakdown.py $(f r03f_sq counter_collection.csv) $(f r03f_sq kernel_trace.csv) > $O/r03_sq_breakdown.txt
cp $(f r03f_kt kernel_stats.csv) $O/r03_kernel_stats.csv; cp $(f r03f_kt_i8 kernel_stats.csv) $O/r03_int8_kernel_stats.csv
head -5 $O/r03_mfma_util.txt; head -4 $O/r03_sq_breakdown.txt
