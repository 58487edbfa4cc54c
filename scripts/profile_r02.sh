#!/bin/bash
# Round-2 evidence (run on the GPU box via gpurun): kernel-trace stats of the default bench, PMC traffic per operation
# (FETCH_SIZE / WRITE_SIZE in separate passes), and the bench lines of every configuration -> gpurun_out/r02/
set -u
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$REPO/gpurun_out/r02
mkdir -p "$OUT"
cd "$REPO"
scripts/trace_bench.sh r02_cfg2 --steps 20 --warmup 5 --spinup 0.2 > /dev/null 2>&1
cp gpurun_out/trace_bench_r02_cfg2.txt "$OUT/rocprofv3_kernel_stats_cfg2.txt"
for op in bloom_add bloom_check bloom_check_fresh cms_add cms_check cbf_add cbf_check cbf_remove; do
  scripts/pmc_op.sh $op 10000000 5 > /dev/null 2>&1
  cp gpurun_out/pmc_$op.json "$OUT/"
done
python bench.py --full > "$OUT/bench_cfg2_default.json" 2> /dev/null
python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_cfg2_steps20.json" 2> /dev/null
for c in cfg3 cfg4 cfg5; do python bench.py --full --config $c --no-cpu-baseline > "$OUT/bench_$c.json" 2> /dev/null; done
python bench.py --full --config cfg4 --no-combine --no-cpu-baseline --steps 3 --warmup 1 > "$OUT/bench_cfg4_nocombine.json" 2> /dev/null
PSK_BENCH_FORCE_DIST=1 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-detail > "$OUT/bench_cfg2_forced_dist_1rank.json" 2> /dev/null
ls -la "$OUT"
