# FETCH_SIZE / WRITE_SIZE passes of the default bench workload, the load / distributed GPU tests, a bench line; outputs under $OUT
set -x
O=${OUT:?set OUT to the output directory}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export SUSHI_BENCH_CACHE=/tmp/sushi_bench_cache
B="python bench.py --steps 3 --warmup 1 --no-cpu-baseline"
rm -rf $O/prof_fetch $O/prof_write
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/prof_fetch -o fetch -- $B > $O/fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/prof_write -o write -- $B > $O/write.log 2>&1
python tools/summarize_pmc.py $O/pmc_fw.csv $(find $O/prof_fetch $O/prof_write -name '*counter_collection.csv'); grep -E "kernel|mac|ifft|refine|tspec" $O/pmc_fw.csv
timeout 300 python -m pytest tests/test_load_gpu.py tests/test_distributed_gpu.py -m gpu -q -x -s 2>&1 | tail -8
python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $O/q_base.json 2>/dev/null; python -c "
import json;d=json.load(open('$O/q_base.json'));print('base',round(d['ms_per_step'],2),d['roofline']['stage_ms'])"
