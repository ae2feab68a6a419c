#!/usr/bin/env python3
"""Compare bench lines of an A/B call (bench_out/ab_*.json): step time and per-kernel ms per step."""
import glob
import json
import sys

rows = {}
for p in sorted(glob.glob(sys.argv[1] if len(sys.argv) > 1 else "bench_out/ab_*.json")):
    try:
        d = json.loads(open(p).read().strip().splitlines()[-1])
    except Exception as e:   # noqa: B902
        print(p, "unreadable:", e)
        continue
    rows[p.split("ab_")[-1][:-5]] = d
names = list(rows)
print("%-28s" % "", " ".join("%12s" % n for n in names))
print("%-28s" % "ms_per_step", " ".join("%12.3f" % rows[n]["ms_per_step"] for n in names))
print("%-28s" % "launches", " ".join("%12.1f" % rows[n].get("launches_per_step", 0) for n in names))
ks = sorted({k for n in names for k in rows[n]["kernels_ms_per_step"]},
            key=lambda k: -max(rows[n]["kernels_ms_per_step"].get(k, 0) for n in names))
for k in ks[:int(sys.argv[2]) if len(sys.argv) > 2 else 30]:
    print("%-28s" % k[:28], " ".join("%12.4f" % rows[n]["kernels_ms_per_step"].get(k, 0) for n in names))
