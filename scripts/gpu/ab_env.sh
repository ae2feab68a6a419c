#!/bin/bash
# A/B of environment switches on one box: the bench (AB_ARGS) with the default settings, then once per
# "NAME=VALUE" word of AB_ENVS (bench_out/ab_<NAME>.json).  Each run under its own time limit; stops
# at the first failure.
mkdir -p bench_out
timeout -k 10 400 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline ${AB_ARGS} > bench_out/ab_base.json 2> bench_out/ab_base.log || exit 1
for kv in ${AB_ENVS}; do
  n=${kv%%=*}
  env "$kv" timeout -k 10 400 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline ${AB_ARGS} > bench_out/ab_$n.json 2> bench_out/ab_$n.log || exit 1
done
