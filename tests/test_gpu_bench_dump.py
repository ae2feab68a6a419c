"""bench.py's plain run and --dump-outputs: the result line of a plain run carries the headline
fields and none of the --full figures, --steps sets the timed steps, and two runs with the same
arguments but different step counts leave identical output arrays (float32/float64, within the
size bound)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--config", "c5", "--pairs", "20000", "--dump-outputs", out]
    line = subprocess.check_output(cmd, timeout=120).decode().strip().splitlines()[-1]
    return json.loads(line)


@pytest.mark.timeout(300)
def test_plain_run_dumps_the_same_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ra, rb = _bench(a, 1), _bench(b, 3)
    for r, steps in ((ra, 1), (rb, 3)):
        assert r["steps"] == steps and r["ms_per_step"] > 0
        assert r["unit"] == "reads/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
        assert abs(r["value"] - r["config"]["input_reads_per_rank"] / (r["ms_per_step"] / 1000.0)) <= 1e-3 * r["value"]
        for k in ("cpu_baseline", "kernels_ms_per_step", "roofline", "dominant_kernel"):
            assert k not in r, k
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a, "*.npy")))
    assert names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(b, "*.npy")))
    for stage in ("sscs", "dcs", "sc", "dcs_sc"):
        for part in ("counters", "rows", "records", "cons_seq", "cons_qual"):
            assert "%s_%s.npy" % (stage, part) in names
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert x.shape == y.shape and np.array_equal(x, y), n
        total += x.nbytes
    assert 0 < total <= 64 << 20
    # sampled SSCS records were voted: their consensus rows are not empty
    assert np.load(os.path.join(a, "sscs_cons_seq.npy")).any()
    assert np.load(os.path.join(a, "sscs_cons_qual.npy")).any()
