"""csrc/intern_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
driver tests/asan/intern_core_driver.cpp (its own main, nothing loaded into Python) runs the three key
finders and the key hash the device interner compiles, each record in a heap block of exactly its
size.  Every case is either refused, or gives what tests/ids_cases.py's restatement of the rules gives
for the same bytes, with every key inside the record.  Exit 0 and a silent stderr are the pass."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ids_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "intern_core_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("intern_core") / "intern_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    return exe


def _case(raw, mode, delim):
    k = IC.keys_of(raw, mode, delim)
    out = struct.pack("<I", len(raw)) + raw + struct.pack("<iI", mode, len(delim)) + delim
    if k.refuse:
        return out + b"\x00", 0
    out += b"\x01"
    for s in k.span:
        out += struct.pack("<IIB", 0, 0, 1) if s is None else struct.pack("<IIB", s[0], s[1], 0)
    return out + struct.pack("<B", k.flags), 1


def _run(driver, path, cases):
    with open(path, "wb") as f:
        f.write(b"".join(c for c, _ in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]
    _, ncases, accepted, _ = p.stdout.split()
    assert int(ncases) == len(cases) and int(accepted) == sum(a for _, a in cases)
    return int(accepted)


def test_every_aux_name_and_cigar_form(driver, tmp_path):
    cases = [_case(r.raw, 0, b"|") for r in IC.aux_records() + IC.cigar_records()]
    cases += [_case(IC.rec(n, aux=b"RGZg\x00").raw, 0, d) for n, d in IC.BARCODE_MODE0]
    cases += [_case(IC.rec(n).raw, 0, b"") for n, _ in IC.BARCODE_MODE0[:3]]
    cases += [_case(r.raw, 1, b"|") for r in IC.name_records(1) + IC.aux_records()]
    assert all(a for _, a in cases)
    bad = [_case(r.raw, 0, b"|") for r in IC.aux_records(IC.RG_MALFORMED)]
    assert not any(a for _, a in bad), "every malformed form must be one the rules refuse"
    assert _run(driver, tmp_path / "forms.bin", cases + bad) == len(cases)


def _smalls():
    return [IC.rec(b"q|AC.GT", aux=IC.RG_FORMS["after_every_type"], lseq=3), IC.rec(b"a_b", cigar=(), aux=IC.RG_FORMS["B_then_Z"], lseq=0),
            IC.rec(b"r||x", cigar=((0, 2), (4, 1)), aux=b"NMC\x03XSZabc\x00RGAx", lseq=5)]


def test_every_truncation_is_refused_or_exact(driver, tmp_path):
    """A record cut at every byte, as it stands (the parser refuses it) and with its block_size set to
    what is left (the aux fields end at every byte of themselves)."""
    cases = []
    for r in _smalls():
        for cut in range(len(r.raw) + 1):
            cases.append(_case(r.raw[:cut], 0, b"|"))
            if cut >= 4:
                cases.append(_case(struct.pack("<i", cut - 4) + r.raw[4:cut], cut % 2, b"|"))
    accepted = _run(driver, tmp_path / "trunc.bin", cases)
    assert 3 < accepted < len(cases), "the cuts must reach refused and accepted records"
    assert any(not a for c, a in cases if len(c) > 60), "an aux field cut short must be among the refusals"


def test_seeded_flips_in_the_aux_bytes(driver, tmp_path):
    r = np.random.RandomState(17)
    recs = _smalls() + IC.aux_records()
    cases = []
    for _ in range(1500):
        rec = recs[int(r.randint(len(recs)))]
        aux_off, raw = rec.fields["aux_off"], bytearray(rec.raw)
        if aux_off == len(raw):
            continue
        for _ in range(1 + int(r.randint(2))):
            raw[aux_off + int(r.randint(len(raw) - aux_off))] ^= 1 << int(r.randint(8))
        cases.append(_case(bytes(raw), int(r.randint(2)), b"|"))
    accepted = _run(driver, tmp_path / "flips.bin", cases)
    assert len(cases) >= 1000 and 0 < accepted < len(cases), "the flips must reach refused and accepted records"
