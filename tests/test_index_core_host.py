"""csrc/index_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
driver tests/asan/index_core_driver.cpp (its own main, nothing loaded into Python; libccio is linked)
runs the header's host instantiation over hand-built records (n_cigar_op 0, 1 and 300, every op code,
flag & 4 with a cigar, pos -1, tid -1, a saturating reference length, a cigar past block_size,
block_size 31) and compares each field with a straight restatement.  Exit 0 and a silent stderr are
the pass."""
import os
import subprocess

import pytest

from consensuscruncher_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "index_core_driver.cpp")
CSRC = os.path.join(ROOT, "consensuscruncher_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    N.io()   # libccio.so is built
    exe = str(tmp_path_factory.mktemp("index_core") / "index_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC, "-L" + N.LIBDIR, "-lccio", "-Wl,-rpath," + N.LIBDIR,
                           "-lpthread", "-ldl"])
    return exe


def test_fields_match_the_restatement(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok 11"), (p.stdout[-800:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]


def test_core_is_what_the_kernel_and_the_index_include():
    inc = open(os.path.join(CSRC, "bam_index.hip.inc")).read()
    assert '#include "index_core.h"' in inc and "idx::field" in inc
    assert '#include "bam_index.hip.inc"' in open(os.path.join(CSRC, "cc_engine.hip")).read()
    io = open(os.path.join(CSRC, "ccio.cpp")).read()
    assert '#include "index_core.h"' in io
    for fn in ("idx::field", "idx::interval", "idx::reg2bin"):
        assert fn in io, fn
