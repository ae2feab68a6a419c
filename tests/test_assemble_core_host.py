"""csrc/assemble_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the
stand-alone driver tests/asan/assemble_core_driver.cpp (its own main, nothing loaded into Python;
libccio is linked as the reference) runs the header's host instantiation over tests/assemble_cases.py
and compares each stream and at[] with ccio_write_bam_ex(..., CCIO_W_MEMORY), sorted and unsorted;
the refusals must name their spec.  Exit 0 and a silent stderr are the pass."""
import os
import struct
import subprocess

import numpy as np
import pytest

import assemble_cases as AC
from consensuscruncher_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "assemble_core_driver.cpp")
CSRC = os.path.join(ROOT, "consensuscruncher_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    N.io()   # libccio.so is built
    exe = str(tmp_path_factory.mktemp("assemble_core") / "assemble_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC, "-L" + N.LIBDIR, "-lccio", "-Wl,-rpath," + N.LIBDIR,
                           "-lpthread", "-ldl"])
    return exe


def _blob(b):
    return struct.pack("<Q", len(b)) + bytes(b)


def _case(case, d, sort, refused=-1):
    out = struct.pack("<I", len(case.sources))
    for p in case.write_sources(d):
        out += struct.pack("<I", len(p)) + p.encode()
    out += _blob(AC.header_bytes(case.pad)) + struct.pack("<I", int(sort))
    out += struct.pack("<Q", len(case.specs)) + np.ascontiguousarray(case.specs, N.OUT_SPEC_DTYPE).tobytes()
    out += struct.pack("<Q", len(case.names)) + case.name_off.tobytes() + case.names_blob[:-1].tobytes()
    out += _blob(case.cons_seq.tobytes()) + _blob(case.cons_qual.tobytes())
    out += struct.pack("<I", len(case.rgs)) + b"".join(struct.pack("<I", len(v)) + v for v in case.rgs)
    return out + struct.pack("<q", refused)


def _run(driver, path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-800:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]
    assert int(p.stdout.split()[1]) == len(cases)


def test_streams_match_the_host_writer(driver, tmp_path):
    cases = [AC.main_case(AC.header_pad(r)) for r in (0, 1, 15)]
    cases += [AC.empty_case(AC.header_pad(15)), AC.lowdigit_case(), AC.toptid_case(), AC.slice_case()]
    cases += [AC.one_case(k) for k in (0, 1, 2)]
    _run(driver, tmp_path / "cases.bin", [_case(c, tmp_path, s) for c in cases for s in (False, True)])


def test_refusals_name_their_spec(driver, tmp_path):
    _run(driver, tmp_path / "bad.bin", [_case(c, tmp_path, False, refused=bad) for _, c, bad, _ in AC.refusals()])


def test_core_is_what_the_kernel_includes():
    inc = open(os.path.join(CSRC, "bam_assemble.hip.inc")).read()
    assert '#include "assemble_core.h"' in inc
    for fn in ("layout", "out16", "key_digits", "slice_records", "Tables", "Spec"):
        assert "asmb::" + fn in inc, fn
    assert '#include "bam_assemble.hip.inc"' in open(os.path.join(CSRC, "cc_engine.hip")).read()
