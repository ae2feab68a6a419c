"""csrc/name_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
driver tests/asan/name_core_driver.cpp (its own main, nothing loaded into Python; libccio is linked
as the reference) runs the header's host instantiation over tests/name_cases.py and compares each
blob and off[] with ccio_format_csn_names / ccio_format_dcs_names; the refusals must name their
name.  Exit 0 and a silent stderr are the pass.  The pipelines' names= option is checked here too,
without a device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import name_cases as NC
from consensuscruncher_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "name_core_driver.cpp")
CSRC = os.path.join(ROOT, "consensuscruncher_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    N.io()   # libccio.so is built
    exe = str(tmp_path_factory.mktemp("name_core") / "name_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC, "-L" + N.LIBDIR, "-lccio", "-Wl,-rpath," + N.LIBDIR,
                           "-lpthread", "-ldl"])
    return exe


def _strs(strs):
    return struct.pack("<I", len(strs)) + b"".join(struct.pack("<I", len(s)) + s for s in strs)


def _csn(case, host=True):
    return (struct.pack("<IqI", 0, case.refused, int(host)) + _strs(case.bcs) + _strs(case.cgs) +
            struct.pack("<Q", len(case.suf)) + case.f9.tobytes() + case.suf.tobytes())


def _dcs(case, d, host=True):
    p = case.write(d).encode()
    return (struct.pack("<IqI", 1, case.refused, int(host)) + struct.pack("<I", len(p)) + p +
            struct.pack("<Q", len(case.rec_tag)) + case.rec_tag.tobytes() + case.rec_ds.tobytes())


def _run(driver, path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-800:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]
    assert int(p.stdout.split()[1]) == len(cases)


def test_csn_names_match_the_host_formatter(driver, tmp_path):
    _run(driver, tmp_path / "csn.bin", [_csn(c) for c in NC.csn_cases()])


def test_dcs_names_match_the_host_formatter(driver, tmp_path):
    _run(driver, tmp_path / "dcs.bin", [_dcs(c, tmp_path) for c in NC.dcs_cases()])


def test_refusals_name_their_name(driver, tmp_path):
    cases = [_csn(c) for _, c, _ in NC.csn_refusals()]
    cases += [_dcs(c, tmp_path, host) for _, c, _, host in NC.dcs_refusals()]
    _run(driver, tmp_path / "bad.bin", cases)


def test_cases_cover_what_they_claim():
    """The shared list holds the shapes the formatter's tests are about (lengths from the host function)."""
    from consensuscruncher_amd.engine import csn_names
    want = max(len(NC.E32), len(NC.EU32), len(NC.E64), len(NC.F7))
    assert all(len(c.suf) >= want for c in NC.csn_cases() if c.name in ("n63", "n4097"))
    assert {I for I in (NC.I32_MIN, NC.I32_MAX, -1, -9, -10, 0, 9, 10)} <= set(NC.E32)
    assert {0x80000000, 0xffffffff} <= set(NC.EU32) and {1, NC.I64_MAX, -1, NC.I64_MIN} <= set(NC.E64)
    for c in NC.csn_cases():
        if c.name in ("residues", "long"):
            blob, off = csn_names(c.interner(), c.f9, c.suf)
            ln = np.diff(off)
            assert (ln > 254).all() if c.name == "long" else ({int(o) % 16 for o in off[:-1]} == set(range(16)) and
                                                               (ln == 33).all())
    assert {len(q) for q in NC.QNAMES} >= {1, 7, 8, 9, 254}


def test_core_is_what_the_kernel_includes():
    inc = open(os.path.join(CSRC, "name_format.hip.inc")).read()
    assert '#include "name_core.h"' in inc
    for fn in ("csn_layout", "csn_out16", "dcs_layout", "dcs_out16", "dcs_pack", "dcs_unpack", "Strs"):
        assert "nmc::" + fn in inc, fn
    assert '#include "name_format.hip.inc"' in open(os.path.join(CSRC, "cc_engine.hip")).read()
    core = open(os.path.join(CSRC, "name_core.h")).read()
    assert "hip/" not in core and "#include <hip" not in core, "the core takes no HIP header"


@pytest.mark.parametrize("which", ["pipeline", "sharded"])
def test_names_option_is_validated(which, tmp_path):
    """names= takes "host" or "device" only, on both pipelines, before anything else happens."""
    missing = str(tmp_path / "missing.bam")
    with pytest.raises(ValueError, match="names must be"):
        if which == "pipeline":
            from consensuscruncher_amd.pipeline import consensus_pipeline
            consensus_pipeline(missing, str(tmp_path), names="bogus")
        else:
            from consensuscruncher_amd.sharded import sharded_pipeline
            sharded_pipeline(missing, str(tmp_path), "False", None, None, names="bogus")
