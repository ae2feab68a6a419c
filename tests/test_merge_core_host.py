"""csrc/merge_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
driver tests/asan/merge_core_driver.cpp (its own main, nothing loaded into Python) checks mrg::key
against a straight restatement (tid -1, pos -1, pos 2^31 - 2, both reverse bits), every refusal code on
heap blocks of exactly the source's size, lower / upper on empty, one-key, all-equal and strictly
increasing arrays, and the place rule on 2, 3 and 8 small sources against std::stable_sort of the
concatenation.  Exit 0 and a silent stderr are the pass."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "merge_core_driver.cpp")
CSRC = os.path.join(ROOT, "consensuscruncher_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merge_core") / "merge_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC, "-lpthread", "-ldl"])
    return exe


def test_core_matches_the_restatement_and_the_stable_sort(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-800:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]


def test_core_is_what_the_kernels_include():
    inc = open(os.path.join(CSRC, "bam_merge.hip.inc")).read()
    assert '#include "merge_core.h"' in inc
    for fn in ("mrg::record", "mrg::lower", "mrg::upper"):
        assert fn in inc, fn
    assert '#include "bam_merge.hip.inc"' in open(os.path.join(CSRC, "cc_engine.hip")).read()
    core = open(os.path.join(CSRC, "merge_core.h")).read()
    for name in ("MRG_MAX_SRC = 8", "MRG_TILE", "MRG_WIN"):
        assert name in core, name
