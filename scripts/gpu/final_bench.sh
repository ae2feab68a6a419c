#!/bin/bash
# Round-end bench lines on the final build, after final_pmc.sh's traffic files were committed under
# profiles/ (each line's roofline.traffic comes from them): C2 with the CPU baseline, then C4, C5 and
# C3 (N = 1), then a rocprofv3 kernel-trace of the C2 bench (its per-kernel averages back the line's
# dominant-kernel time).  Each step under its own time limit; stops at the first failure.
mkdir -p bench_out
R=$(pwd)
timeout -k 10 600 python bench.py --full > bench_out/final_c2.json 2> bench_out/final_c2.log || exit $?
for c in ${CONFIGS:-c4 c5 c3}; do
  timeout -k 10 600 python bench.py --full --config $c --steps 10 --warmup 2 --no-cpu-baseline > bench_out/final_$c.json 2> bench_out/final_$c.log || exit $?
done
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $R/bench_out/final_prof -o run --output-format csv -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline > $R/bench_out/final_prof_bench.json 2> $R/bench_out/final_prof_bench.log || exit $?
