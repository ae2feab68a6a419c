"""csrc/unpack_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the
stand-alone driver tests/asan/unpack_core_driver.cpp (its own main, nothing loaded into Python) runs
the record parser, rec_digest and the slot writer the device unpacker compiles, over streams held in
heap blocks of exactly the stream's size.  Valid records must parse to the values tests/unpack_cases.py
computed with struct when it built them (fields, offsets, digest, both slots byte for byte); cut or
corrupted ones must be refused, or parsed with every offset inside the record and the stream.  Exit 0
and a silent stderr are the pass."""
import os
import struct
import subprocess

import numpy as np
import pytest

import unpack_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "asan", "unpack_core_driver.cpp")
CORE = os.path.join(ROOT, "consensuscruncher_amd", "csrc", "unpack_core.h")
KERNEL = os.path.join(ROOT, "consensuscruncher_amd", "csrc", "table_unpack.hip.inc")

MUST, MAY, REFUSE = 2, 1, 0
FIELDS = ("bs", "tid", "pos", "l_read_name", "mapq", "n_cigar", "flag", "lseq", "mtid", "mpos", "tlen", "qn_len", "qlen")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unpack_core") / "unpack_core_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                           "-static-libubsan", "-o", exe, SRC])
    return exe


def _expect(rec):
    f = rec.fields
    return (struct.pack("<13i", *[f[k] for k in FIELDS]) +
            struct.pack("<4I", f["cig_off"], f["seq_off"], f["qual_off"], f["aux_off"]) +
            struct.pack("<BQII", f["rflags"], rec.rdig, len(rec.pay), len(rec.qn)) + rec.pay + rec.qn)


def _case(stream, entries):
    """entries: (offset, want, Rec or None)"""
    out = struct.pack("<II", len(stream), len(entries)) + stream
    for off, want, rec in entries:
        out += struct.pack("<QB", int(off), want) + (_expect(rec) if want == MUST else b"")
    return out, len(entries)


def _run(driver, path, cases):
    with open(path, "wb") as f:
        f.write(b"".join(c for c, _ in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-3000:])
    assert p.stderr == "", p.stderr[-3000:]
    _, records, accepted = p.stdout.split()
    assert int(records) == sum(n for _, n in cases)
    return int(accepted)


def _smalls():
    rng = np.random.default_rng(5)
    return [[UC.make(rng, 0, 17, 9, aux=UC.AUXES[1]), UC.make(rng, 1, 0, 1, cigar="none"), UC.make(rng, 2, 33, 16, cigar="all")],
            [UC.make(rng, 3, 1, 2, qual_ff=True), UC.make(rng, 4, 150, 17, aux=UC.AUXES[4]), UC.make(rng, 5, 2, 8)],
            [UC.make(rng, 6, 129, 255), UC.make(rng, 7, 16, 1), UC.make(rng, 8, 15, 9, cigar="none", aux=UC.AUXES[3])]]


def test_valid_records_parse_to_the_struct_values(driver, tmp_path):
    recs = UC.shapes()
    assert {r.fields["lseq"] for r in recs} >= set(UC.LSEQS) and {r.fields["l_read_name"] for r in recs} >= set(UC.LQNS)
    stream, off = UC.stream_of(recs)
    assert {int(o) % 16 for o in off} == set(range(16)), "record starts must fall on every alignment mod 16"
    assert any(r.fields["qlen"] == -1 for r in recs) and any(r.fields["rflags"] == 2 and r.fields["lseq"] for r in recs)
    accepted = _run(driver, tmp_path / "valid.bin", [_case(stream, [(o, MUST, r) for o, r in zip(off, recs)])])
    assert accepted == len(recs)


def test_every_truncation_is_refused_or_exact(driver, tmp_path):
    cases = []
    for recs in _smalls():
        stream, off = UC.stream_of(recs)
        for cut in range(len(stream)):
            ent = []
            for o, r in zip(off, recs):
                if int(o) > cut:
                    continue
                ent.append((o, MUST, r) if int(o) + len(r.raw) <= cut else (o, REFUSE, None))
            cases.append(_case(stream[:cut], ent))
    _run(driver, tmp_path / "trunc.bin", cases)


def test_seeded_flips_in_the_length_fields_are_refused_or_inside_bounds(driver, tmp_path):
    r = np.random.RandomState(31)
    cases, accepted_possible = [], 0
    length_bytes = [0, 1, 2, 3, 4 + 8, 4 + 12, 4 + 13, 4 + 16, 4 + 17, 4 + 18, 4 + 19]   # block_size, l_read_name, n_cigar, l_seq
    for recs in _smalls() + [UC.shapes()[:12]]:
        stream, off = UC.stream_of(recs)
        for _ in range(120):
            k = int(r.randint(len(recs)))
            at = int(off[k]) + length_bytes[int(r.randint(len(length_bytes)))]
            bad = bytearray(stream)
            bad[at] ^= 1 << int(r.randint(8))
            ent = [(o, MAY if i == k else MUST, None if i == k else rec) for i, (o, rec) in enumerate(zip(off, recs))]
            cases.append(_case(bytes(bad), ent))
            accepted_possible += 1
    assert len(cases) >= 400
    accepted = _run(driver, tmp_path / "flips.bin", cases)
    others = sum(n for _, n in cases) - len(cases)
    assert others <= accepted < others + len(cases), "the flips must reach both refused and accepted records"


def test_handmade_bad_records_are_refused(driver, tmp_path):
    rng = np.random.default_rng(9)
    good = UC.make(rng, 0, 40, 12).raw
    def patched(at, fmt, v):
        b = bytearray(good)
        b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, v)
        return bytes(b)
    bad = {"bs_below_32": patched(0, "<i", 31), "bs_negative": patched(0, "<i", -1),
           "bs_past_stream": patched(0, "<i", len(good)), "lseq_negative": patched(4 + 16, "<i", -5),
           "lseq_overruns_bs": patched(4 + 16, "<i", 4000), "lseq_huge": patched(4 + 16, "<i", 0x7fffffff),
           "ncigar_overruns_bs": patched(4 + 12, "<H", 0xffff), "lqn_overruns_bs": patched(4 + 8, "<B", 255),
           "cut_mid_record": good[:50], "three_bytes": good[:3], "empty": b""}
    accepted = _run(driver, tmp_path / "hand.bin", [_case(s, [(0, REFUSE, None)]) for s in bad.values()])
    assert accepted == 0


def test_core_is_what_the_kernel_includes():
    inc = open(KERNEL).read()
    assert '#include "unpack_core.h"' in inc and os.path.exists(CORE)
    for fn in ("parse", "rec_digest", "pay_chunk", "qn_chunk", "pay_slot", "qn_slot", "Rec"):
        assert "upk::" + fn in inc, fn
    engine = open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")).read()
    assert '#include "table_unpack.hip.inc"' in engine
    ccio = open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "ccio.cpp")).read()
    assert '#include "unpack_core.h"' in ccio and "upk::rec_digest" in ccio and "upk::pay_slot" in ccio and "upk::parse" in ccio
