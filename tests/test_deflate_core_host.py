"""csrc/deflate_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the
stand-alone driver tests/asan/deflate_core_driver.cpp (its own main, nothing loaded into Python)
runs the code builder, symbol tables and header writer the device encoder compiles, on the crafted
buffers of tests/test_gpu_bgzf.py, on histograms that force the length limit and on the degenerate
trees, and inflates every stream with zlib.  Exit 0 and a silent stderr are the pass."""
import os
import struct
import subprocess
import zlib

import pytest

from parity import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "deflate_core_driver.cpp")
CORE = os.path.join(ROOT, "consensuscruncher_amd", "csrc", "deflate_core.h")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_core") / "deflate_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC, "-lz"])
    return exe


def _run(driver, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([driver] + list(args), env=env, capture_output=True, text=True, timeout=300)


def test_core_round_trips_under_sanitizers(driver):
    p = _run(driver)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]
    assert p.stderr == "", p.stderr[-3000:]


def test_core_on_real_bam_bytes(driver, tmp_path):
    raw = open(os.path.join(GOLDEN, "basic", "input.bam"), "rb").read()
    off, out = 0, bytearray()
    while off < len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        out += zlib.decompress(raw[off + 18:off + bsize - 8], -15)
        off += bsize
    f = tmp_path / "bam.bin"
    f.write_bytes(bytes(out))
    p = _run(driver, str(f))
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-3000:]
    assert p.stderr == "", p.stderr[-3000:]


def test_core_is_what_the_kernel_includes():
    inc = open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "bgzf_deflate.hip.inc")).read()
    assert '#include "deflate_core.h"' in inc and os.path.exists(CORE)
    for fn in ("huffman_lengths", "limit_lengths", "canonical_codes", "plan_header", "write_header", "tok_bits"):
        assert "dfl::" + fn in inc, fn
