"""csrc/inflate_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the
stand-alone driver tests/asan/inflate_core_driver.cpp (its own main, nothing loaded into Python)
runs the bit reader, block headers, table builder and symbol loop the device inflater compiles, with
input, output and tables in heap blocks of exactly the sizes the kernel contract names.  Python's
zlib is the judge: valid streams must come out byte-exact; corrupt ones must be refused or give
exactly what zlib gives.  Exit 0 and a silent stderr are the pass."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import inflate_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "inflate_core_driver.cpp")
CORE = os.path.join(ROOT, "consensuscruncher_amd", "csrc", "inflate_core.h")
KERNEL = os.path.join(ROOT, "consensuscruncher_amd", "csrc", "bgzf_inflate.hip.inc")

MUST, MAY, REFUSE = 2, 1, 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_core") / "inflate_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    return exe


def _record(stream, ulen, want, expect=b""):
    assert want == REFUSE or len(expect) == ulen
    return struct.pack("<IIB", len(stream), ulen, want) + stream + (expect if want != REFUSE else b"")


def _corrupt_record(stream, ulen):
    """zlib decides: a stream it refuses must be refused, one it accepts may be refused or must match."""
    got = IC.judge(stream, ulen)
    return _record(stream, ulen, REFUSE) if got is None else _record(stream, ulen, MAY, got)


def _run(driver, path, records):
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]
    _, cases, accepted = p.stdout.split()
    assert int(cases) == len(records)
    return int(accepted)


def test_valid_streams_come_out_exact(driver, tmp_path):
    streams = IC.valid_streams()
    names = set(n.split("/")[0] for n, _, _ in streams)
    assert names >= {"text", "zeros", "random", "ladder", "window", "bam", "eof", "dist32768"}
    for _, s, data in streams:
        assert IC.judge(s, len(data)) == data
    accepted = _run(driver, tmp_path / "valid.bin", [_record(s, len(d), MUST, d) for _, s, d in streams])
    assert accepted == len(streams)


def test_every_truncation_is_refused_or_exact(driver, tmp_path):
    smalls = [IC.raw_deflate(IC.text(300, 21), 6), IC.raw_deflate(IC.text(300, 22), 6, zlib.Z_FIXED),
              IC.raw_deflate(IC.random_bytes(200, 23), 0)]
    recs = []
    for n, s in zip((300, 300, 200), smalls):
        recs += [_corrupt_record(s[:cut], n) for cut in range(len(s))]
    _run(driver, tmp_path / "trunc.bin", recs)


def test_seeded_bit_flips_are_refused_or_exact(driver, tmp_path):
    r = np.random.RandomState(31)
    recs, accepted_by_zlib = [], 0
    sources = [(IC.raw_deflate(IC.text(2000, 24), 6), 2000), (IC.raw_deflate(IC.text(2000, 25), 9, zlib.Z_FIXED), 2000),
               (IC.raw_deflate(IC.bam_stream()[:6000], 6), 6000), (IC.raw_deflate(IC.random_bytes(500, 26), 0), 500)]
    for s, n in sources:
        for _ in range(400):
            bit = int(r.randint(8 * len(s)))
            bad = bytearray(s)
            bad[bit >> 3] ^= 1 << (bit & 7)
            rec = _corrupt_record(bytes(bad), n)
            accepted_by_zlib += rec[8] == MAY
            recs.append(rec)
    assert 0 < accepted_by_zlib < len(recs), "the flips must reach both kinds of stream"
    _run(driver, tmp_path / "flips.bin", recs)


def test_handmade_corrupt_streams_are_refused(driver, tmp_path):
    cases = IC.handmade_corrupt()
    assert {"distance_beyond_output", "oversubscribed_lengths", "symbol_286", "bad_nlen", "output_longer_than_ulen",
            "output_shorter_than_ulen"} <= set(n for n, _, _ in cases)
    accepted = _run(driver, tmp_path / "hand.bin", [_record(s, ulen, REFUSE) for _, s, ulen in cases])
    assert accepted == 0


def test_core_is_what_the_kernel_includes():
    inc = open(KERNEL).read()
    assert '#include "inflate_core.h"' in inc and os.path.exists(CORE)
    for fn in ("run", "Bits", "Tables", "State", "Huff"):
        assert "ifl::" + fn in inc, fn
    engine = open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")).read()
    assert '#include "bgzf_inflate.hip.inc"' in engine
