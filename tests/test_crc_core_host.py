"""csrc/crc_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
driver tests/asan/crc_core_driver.cpp (its own main, nothing loaded into Python) checks the generated
tables against the bit-by-bit definition, combine at every split of three short buffers, the
zero-start identity for pads 0 to 15, and the per-lane rule k_crc32 compiles, run lane by lane (256
lanes) over heap blocks of exactly the aligned span.  Python's zlib.crc32 is the judge.  Exit 0 and a
silent stderr are the pass."""
import os
import struct
import subprocess
import zlib

import pytest

import crc_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "crc_core_driver.cpp")
CSRC = os.path.join(ROOT, "consensuscruncher_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crc_core") / "crc_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    return exe


def _case(pad, data):
    return b"\x00" + struct.pack("<II", pad, len(data)) + data + struct.pack("<I", zlib.crc32(data))


def _splits(data):
    rec = b"\x01" + struct.pack("<I", len(data)) + data + struct.pack("<I", zlib.crc32(data))
    return rec + b"".join(struct.pack("<II", zlib.crc32(data[:s]), zlib.crc32(data[s:])) for s in range(len(data) + 1))


def _run(driver, path, records):
    with open(path, "wb") as f:
        f.write(b"".join(records))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]
    assert int(p.stdout.split()[1]) == len(records)


def test_tables_identities_and_lane_rule_at_every_length_and_alignment(driver, tmp_path):
    big = CC.contents(65536 + 16, seed=11)
    recs = []
    for n in CC.LENGTHS:
        for a in CC.ALIGNS:
            recs.append(_case(a, big["random"][a:a + n]))
    for name in ("zeros", "ff", "first_bit", "last_bit"):   # every content at the lengths around a word and a stride
        for n in (0, 1, 15, 16, 17, 4081, 4097, 65536):
            recs.append(_case(CC.ALIGNS[(n + len(name)) % len(CC.ALIGNS)], CC.contents(n)[name]))
    assert len(recs) == len(CC.LENGTHS) * len(CC.ALIGNS) + 32
    _run(driver, tmp_path / "cases.bin", recs)


def test_combine_at_every_split_of_three_short_buffers(driver, tmp_path):
    bufs = [CC.contents(37, seed=1)["random"], b"\x00" * 5 + b"\xff" * 20 + b"\x00" * 8,
            b"the quick brown fox jumps over the lazy dog"]
    _run(driver, tmp_path / "splits.bin", [_splits(b) for b in bufs])


def test_a_wrong_crc_is_noticed(driver, tmp_path):
    """The driver really compares: one flipped bit in zlib's value fails the case."""
    data = CC.contents(100)["random"]
    rec = bytearray(_case(3, data))
    rec[-1] ^= 0x10
    with open(tmp_path / "bad.bin", "wb") as f:
        f.write(bytes(rec))
    p = subprocess.run([driver, str(tmp_path / "bad.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "case 0" in p.stderr


def test_core_is_what_the_kernel_includes():
    inc = open(os.path.join(CSRC, "bgzf_crc32.hip.inc")).read()
    assert '#include "crc_core.h"' in inc and os.path.exists(os.path.join(CSRC, "crc_core.h"))
    for fn in ("lane", "finish", "slice_entry", "stride_entry", "Tables"):
        assert "crc::" + fn in inc, fn
    engine = open(os.path.join(CSRC, "cc_engine.hip")).read()
    assert '#include "bgzf_crc32.hip.inc"' in engine
    assert "crc::combine" in open(os.path.join(CSRC, "bgzf_inflate.hip.inc")).read()
