#!/usr/bin/env python
"""The device CRC32 (k_crc32, Engine.device_crc) off against on, on one box: raw JSON lines.

    python scripts/crc32_ab.py [--runs 3] [--reps 5] [--pairs 300000] [--out profiles/crc32_ab.jsonl]

The parent writes one seeded C2-model input BAM (synth.generate, level 1), never opens the GPU itself
and starts fresh worker processes, crc off and on alternating, --runs of each.  A worker measures

  kernel     device events (cc_kernel_times) over 1,024 pieces / members of 0xff00 bytes (the inflated
             BAM's bytes, repeated), --reps calls after one warm-up call:
               encoder: Engine.bgzf_deflate of the 1,024 pieces: scopes bgzf_deflate and, with crc on,
                        bgzf_crc32 over the same rounds;
               inflater: Engine.bgzf_inflate of those members (crc=on): scopes bgzf_inflate and, with
                        crc on, bgzf_crc32 over the same round;
             crc_gbps = bytes / bgzf_crc32's time, crc_over_codec = bgzf_crc32 / the codec's scope;
  open       Bam(path) with device_inflate on, --reps times: wall seconds and the process's CPU-seconds
             (user + system, every thread) of the whole-file open;
  write      Bam.write(level=1) of that handle with device_bgzf on (finish: deflate + write), likewise.

Nothing here is a baseline for another day or box: compare only lines of one invocation."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECE = 0xff00
MEMBERS = 1024


def cpu_s():
    t = os.times()
    return t.user + t.system


def worker(path, crc, reps):
    import gzip
    from consensuscruncher_amd.engine import Bam, Engine
    eng = Engine(0)
    eng.device_crc(crc)
    stream = gzip.open(path, "rb").read()
    data = (stream * (MEMBERS * PIECE // len(stream) + 1))[:MEMBERS * PIECE]
    res = {"crc": "device" if crc else "host", "bytes": len(data), "members": MEMBERS, "reps": reps}

    def timed(call):
        call()   # warm-up: buffers, code objects
        eng.set_profiling(True)
        for _ in range(reps):
            out = call()
        t = eng.kernel_times()
        eng.set_profiling(False)
        return out, {k: [round(v[0], 4), v[1]] for k, v in t.items() if k.startswith("bgzf_")}

    members, t = timed(lambda: eng.bgzf_deflate(data))
    res["encoder"] = t
    raw = b"".join(members)
    got, t = timed(lambda: eng.bgzf_inflate(raw, crc=crc))
    assert got[0] == data and all(got[1])
    res["inflater"] = t
    for side, codec in (("encoder", "bgzf_deflate"), ("inflater", "bgzf_inflate")):
        k = res[side]
        if "bgzf_crc32" in k:
            res[side + "_crc_gbps"] = round(reps * len(data) / (k["bgzf_crc32"][0] * 1e-3) / 1e9, 1)
            res[side + "_crc_over_codec"] = round(k["bgzf_crc32"][0] / k[codec][0], 5)

    eng.device_inflate(True)
    Bam(path).close()   # warm-up
    laps = []
    for i in range(reps):
        c, w = cpu_s(), time.perf_counter()
        b = Bam(path)
        laps.append([round(time.perf_counter() - w, 4), round(cpu_s() - c, 4)])
        if i < reps - 1:
            b.close()
    res["open_wall_cpu_s"] = laps
    eng.device_inflate(False)
    eng.device_bgzf(True)
    out = path + ".out.bam"
    b.write(out, level=1)   # warm-up
    laps = []
    for _ in range(reps):
        c, w = cpu_s(), time.perf_counter()
        b.write(out, level=1)
        laps.append([round(time.perf_counter() - w, 4), round(cpu_s() - c, 4)])
    res["write_wall_cpu_s"] = laps
    res["records"] = int(b.n)
    res["inflated_bytes"] = len(stream)
    eng.device_bgzf(False)
    os.remove(out)
    b.close()
    eng.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=300000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc32_ab.jsonl"))
    ap.add_argument("--worker", nargs=2, metavar=("BAM", "CRC"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1] == "1", a.reps)
    from consensuscruncher_amd import synth
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "input.bam")
    synth.write_bam_native(synth.generate(a.pairs, seed=synth.SEED_BASE + 32), path, level=1)
    with open(a.out, "a") as f:
        for run in range(a.runs):
            for crc in ("0", "1"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--worker", path, crc],
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:   # nothing more is started after a failed worker
                    sys.stderr.write(p.stderr[-3000:])
                    return p.returncode or 1
                line = json.dumps(dict(run=run + 1, **json.loads(p.stdout.strip().splitlines()[-1])))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
