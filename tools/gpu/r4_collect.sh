# round 4: the evidence set for the CURRENT kernel build -- GPU test suite (optional), PMC HBM bytes of one C3 join (two separate --pmc
# passes) and of one C5 group-by, rocprofv3 kernel stats of the same commands, the headline line (which then carries roofline.traffic
# and extra.c2 / extra.c5), a spread of headline processes, C5 in five processes (+ null keys), shapes, operators at 1e8 / 1e9 rows,
# the fused multi-GPU simulation and the forced-distributed line through the C entry point.
# usage: bash tools/gpu/r4_collect.sh <tag>            (GDF_COLLECT_PYTEST=1 also runs the GPU suite first)
set -x
TAG=${1:-r4z}
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/$TAG
mkdir -p $O
cd $R
if [ -n "$GDF_COLLECT_PYTEST" ]; then timeout 3000 python -m pytest tests -m gpu -q 2>&1 | grep -E "passed|failed|error" | tail -3 > $O/pytest_gpu.txt; cat $O/pytest_gpu.txt; fi
cd /tmp && export TMPDIR=/tmp
B="python $R/bench.py --cpu-sample 0 --pandas-sample 0 --extra 0"
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o join -- $B --steps 1 --warmup 0 > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o join -- $B --steps 1 --warmup 0 > $O/pmc_write.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -o join -- $B --steps 3 --warmup 1 > $O/trace.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_c5_fetch -o c5 -- python $R/tools/bench_c5.py --reps 1 --no-checks > $O/pmc_c5_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_c5_write -o c5 -- python $R/tools/bench_c5.py --reps 1 --no-checks > $O/pmc_c5_write.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_c5 -o c5 -- python $R/tools/bench_c5.py --reps 3 --no-checks > $O/trace_c5.log 2>&1
cd $R
python tools/rocprof_summary.py $O/trace $O/kernel_stats.md
python tools/rocprof_summary.py $O/trace_c5 $O/kernel_stats_c5.md
python tools/pmc_hbm_json.py $(find $O/pmc_fetch -name "*counter_collection.csv" | head -1) $(find $O/pmc_write -name "*counter_collection.csv" | head -1) $O/pmc_hbm.json > $O/pmc_hbm.txt
python tools/pmc_hbm_json.py $(find $O/pmc_c5_fetch -name "*counter_collection.csv" | head -1) $(find $O/pmc_c5_write -name "*counter_collection.csv" | head -1) $O/pmc_hbm_c5.json "python tools/bench_c5.py --reps 1 --no-checks (a warm-up call + one timed call: divide by launches)" > $O/pmc_hbm_c5.txt
cp $O/pmc_hbm.json $R/profiles/zz_tmp_pmc_hbm.json          # so that THIS run's bench line already carries the traffic
python bench.py --full 2>$O/bench.err | grep '^{' | tail -1 > $O/bench.json
rm -f $R/profiles/zz_tmp_pmc_hbm.json
for i in 1 2 3; do python bench.py --steps 10 --warmup 3 --cpu-sample 0 --pandas-sample 0 --extra 0 2>/dev/null | grep '^{' | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps({'ms_per_step': d['ms_per_step'], 'kernels_ms_per_step': d['kernels_ms_per_step']}))" >> $O/bench_spread.jsonl; done
for i in 1 2 3 4 5; do python tools/bench_c5.py 2>/dev/null | tail -1 >> $O/bench_c5_five_processes.jsonl; done
python tools/bench_c5.py --null-keys 0.01 2>/dev/null | tail -1 > $O/bench_c5_nullkeys.json
for i in 1 2; do python tools/bench_c5.py --force GDF_GBP_NO_XCD 2>/dev/null | tail -1 >> $O/bench_c5_per_workgroup_segments.jsonl; done
python tools/bench_shapes.py > $O/bench_shapes.jsonl 2>/dev/null
python tools/bench_ops.py > $O/bench_ops.jsonl 2>/dev/null
python tools/bench_ops.py --rows 1000000000 --ops partition,scan,filter > $O/bench_ops_1e9.jsonl 2>/dev/null
python tools/sim_c4_fused.py 2>/dev/null | tail -4 > $O/sim_c4_fused.txt
python bench.py --force-distributed --strategy fused --steps 5 --warmup 2 --probe-rows 1000000000 --build-rows 125000000 --cpu-sample 0 --pandas-sample 0 2>/dev/null | grep '^{' | tail -1 > $O/bench_force_distributed_fused.json
rm -rf $O/trace/*/*.db $O/trace_c5/*/*.db; find $O -name "*kernel_trace.csv" -delete; find $O -name "*counter_collection.csv" -size +8M -delete; find $O -name "*.db" -delete
cut -c1-900 $O/bench.json; cat $O/bench_spread.jsonl; cut -c1-300 $O/bench_c5_five_processes.jsonl; cat $O/pmc_hbm.txt $O/pmc_hbm_c5.txt; head -30 $O/kernel_stats.md; du -sh $O
