#!/bin/bash
# Round-end PMC traffic of every bench config on the final build (pmc_cfg.sh per config, FETCH_SIZE and
# WRITE_SIZE in separate rocprofv3 passes): bench_out/pmc_<cfg>_traffic.json, committed as
# profiles/pmc_latest.json (c2) and profiles/pmc_<cfg>_latest.json.  Stops at the first failure.
mkdir -p bench_out
for c in ${CONFIGS:-c2 c4 c5 c3}; do
  CFG=$c scripts/gpu/pmc_cfg.sh || exit $?
done
