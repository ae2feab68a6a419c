"""The device BGZF inflater (k_bgzf_inflate behind cc_bgzf_inflate and the readers' hook).  The judge
is Python's zlib, never the project's inflater: every good member must come out byte-exact, every
hand-made corrupt member must be refused without touching its neighbours, and the readers and the
pipeline must give what they give with the option off."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as IC
import pysam  # the oracle shim
from parity import GOLDEN

pytestmark = pytest.mark.gpu

INPUT = IC.INPUT
OUTPUTS = ("sscs", "singleton", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction", "uncorrected",
           "dcs_sc", "all_unique")


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _member(stream, data):
    """A BGZF member around a raw DEFLATE stream (ISIZE and CRC32 of data)."""
    return (struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(stream) + 25) + stream +
            struct.pack("<II", zlib.crc32(data), len(data)))


@pytest.fixture(scope="module")
def valid():
    """Every buffer under every variant, each piece a member, judged by zlib once."""
    out = []
    for name, stream, data in IC.valid_streams():
        assert IC.judge(stream, len(data)) == data, name
        out.append((name, _member(stream, data), data))
    return out


def test_every_variant_inflates_exactly(engine, valid):
    raw = b"".join(m for _, m, _ in valid)
    want = b"".join(d for _, _, d in valid)
    data, ok = engine.bgzf_inflate(raw)
    bad = [valid[j][0] for j, v in enumerate(ok) if not v]
    assert not bad, bad
    assert len(ok) == len(valid)
    if data != want:
        off = 0
        for name, _, d in valid:
            assert data[off:off + len(d)] == d, name
            off += len(d)
    assert any(len(d) == 0 for _, _, d in valid), "a zero-length member is among them"
    again, ok2 = engine.bgzf_inflate(raw)
    assert again == data and ok2 == ok, "a second call must return the same bytes"


def test_device_members_round_trip(engine):
    """Members made by the device encoder come back through the device inflater."""
    data = IC.bam_stream()[:3 * IC.PIECE + 123] + bytes(IC.PIECE) + IC.random_bytes(IC.PIECE + 5, 41)
    members = engine.bgzf_deflate(data)
    assert len(members) >= 6
    for j, m in enumerate(members):   # zlib first: the encoder's members are what they claim
        assert zlib.decompress(m[18:-8], -15) == data[j * IC.PIECE:(j + 1) * IC.PIECE]
    got, ok = engine.bgzf_inflate(b"".join(members) + IC.EOF_MEMBER)
    assert all(ok) and len(ok) == len(members) + 1
    assert got == data


def test_more_members_than_one_round(engine):
    """1100 members of a few hundred bytes: two rounds, both streams and both buffers take turns."""
    r = np.random.RandomState(43)
    src = IC.bam_stream()
    parts = []
    for j in range(1100):
        n = 200 + int(r.randint(400))
        o = int(r.randint(len(src) - n))
        parts.append(src[o:o + n])
    levels = (1, 6, 9, 0)
    raw = b"".join(_member(IC.raw_deflate(p, levels[j % 4]), p) for j, p in enumerate(parts))
    got, ok = engine.bgzf_inflate(raw)
    assert len(ok) == 1100 and all(ok)
    assert got == b"".join(parts)
    assert engine.bgzf_inflate(raw) == (got, ok)


def _call(engine, comp, coff, clen, uoff, ulen, out):
    a = [np.asarray(v, t) for v, t in ((coff, np.uint64), (clen, np.uint32), (uoff, np.uint64), (ulen, np.uint32))]
    ok = np.full(len(coff), 7, np.uint8)
    comp = np.frombuffer(comp, np.uint8)
    bad = engine.lib.cc_bgzf_inflate(engine.h, comp.ctypes.data_as(C.c_void_p), a[0].ctypes.data_as(C.c_void_p),
                                     a[1].ctypes.data_as(C.c_void_p), a[2].ctypes.data_as(C.c_void_p),
                                     a[3].ctypes.data_as(C.c_void_p), len(coff), out.ctypes.data_as(C.c_void_p),
                                     ok.ctypes.data_as(C.c_void_p))
    return int(bad), ok


def test_canaries_around_every_member(engine):
    """Members scattered over the output with gaps between them: the gaps keep their bytes."""
    streams = [(IC.raw_deflate(d, 6), d) for d in (IC.text(1000, 51), IC.ladder(), b"", IC.window_repeat(), IC.text(1, 52))]
    comp, coff, clen, uoff, ulen = bytearray(), [], [], [], []
    at = 64
    for s, d in streams:
        comp += b"\xee" * 3   # payloads at odd offsets
        coff.append(len(comp))
        clen.append(len(s))
        comp += s
        uoff.append(at)
        ulen.append(len(d))
        at += len(d) + 37
    out = np.full(at + 64, 0xc3, np.uint8)
    bad, ok = _call(engine, bytes(comp), coff, clen, uoff, ulen, out)
    assert bad == 0 and ok.tolist() == [1] * len(streams)
    covered = np.zeros(out.size, bool)
    for (s, d), o in zip(streams, uoff):
        assert out[o:o + len(d)].tobytes() == d
        covered[o:o + len(d)] = True
    assert (out[~covered] == 0xc3).all(), "bytes outside the members' ranges were written"


def test_handmade_corrupt_members_are_refused(engine):
    """The host driver's hand-made corrupt streams (tests/test_inflate_core_host.py guards them first)
    between good members: refused, the neighbours exact, nothing outside any member's range touched.
    A kernel that follows the core's bounds cannot fault on them."""
    cases = IC.handmade_corrupt()
    good = [IC.text(3000, 61), IC.bam_stream()[:20000], IC.random_bytes(777, 62)]
    plan = []   # (stream, ulen, expected bytes or None)
    for j, (name, s, ulen) in enumerate(cases):
        g = good[j % len(good)]
        plan.append((IC.raw_deflate(g, (1, 6, 9)[j % 3]), len(g), g))
        plan.append((s, ulen, None))
    plan.append((IC.raw_deflate(good[0], 6), len(good[0]), good[0]))
    comp, coff, clen, uoff, ulen = bytearray(), [], [], [], []
    at = 16
    for s, n, _ in plan:
        coff.append(len(comp))
        clen.append(len(s))
        comp += s
        uoff.append(at)
        ulen.append(n)
        at += n + 16
    out = np.full(at, 0x5a, np.uint8)
    bad, ok = _call(engine, bytes(comp), coff, clen, uoff, ulen, out)
    assert bad == len(cases)
    covered = np.zeros(out.size, bool)
    for j, (s, n, want) in enumerate(plan):
        covered[uoff[j]:uoff[j] + n] = True
        if want is None:
            assert ok[j] == 0, cases[j // 2][0]
        else:
            assert ok[j] == 1 and out[uoff[j]:uoff[j] + n].tobytes() == want, j
    assert (out[~covered] == 0x5a).all(), "bytes outside the members' ranges were written"


def _indexed(tmp_path):
    from consensuscruncher_amd.engine import Bam
    p = str(tmp_path / "input.bam")
    Bam(INPUT).write(p, level=6, index=True)
    return p


def _whole(path):
    from consensuscruncher_amd.engine import Bam
    b = Bam(path)
    return [b.qname(i) for i in range(b.n)], [c.tolist() for c in b.cores()]


def _fetch(path, regions):
    from consensuscruncher_amd.engine import Bam
    t, b, e = zip(*regions)
    part = Bam.open_regions(path, t, b, e)
    return [part.qname(i) for i in range(part.n)], [c.tolist() for c in part.cores()]


def test_readers_give_the_same_records(engine, tmp_path):
    p = _indexed(tmp_path)
    regions = ([(0, 0, 5000)], [(0, 20000, 60000), (0, 100000, 150000)])
    want = _whole(INPUT), _whole(p), [_fetch(p, r) for r in regions]
    assert len(want[0][0]) > 1000 and all(len(f[0]) > 0 for f in want[2])
    engine.set_profiling(True)
    assert engine.device_inflate(True) is False and engine.inflate_device
    try:
        got = _whole(INPUT), _whole(p), [_fetch(p, r) for r in regions]
        times = engine.kernel_times()
    finally:
        assert engine.device_inflate(False) is True
        engine.set_profiling(False)
    assert got == want
    assert "bgzf_inflate" in times and "bgzf_in_upload" in times and "bgzf_in_download" in times
    assert not engine.inflate_device


def _pipeline(engine, tmp, inflate):
    import json
    import shutil
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, "basic")
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    os.makedirs(tmp)
    shutil.copy(INPUT, os.path.join(tmp, "sample.bam"))
    kw["level"] = 1
    return consensus_pipeline(os.path.join(tmp, "sample.bam"), tmp, engine=engine, inflate=inflate, **kw)


def test_pipeline_outputs_are_byte_identical(engine, tmp_path):
    engine.set_profiling(True)
    dev = _pipeline(engine, str(tmp_path / "device"), "device")
    times = engine.kernel_times()
    engine.set_profiling(False)
    assert not engine.inflate_device, "the option is wired for the call only"
    assert "bgzf_inflate" in times, "the inflater's kernel ran and was timed under its scope name"
    host = _pipeline(engine, str(tmp_path / "host"), "host")
    exp = os.path.join(GOLDEN, "basic", "expected")
    for k in OUTPUTS:
        assert open(dev[k], "rb").read() == open(host[k], "rb").read(), k
        assert pysam.sam_lines(dev[k]) == pysam.sam_lines(os.path.join(exp, k + ".bam")), k
    # every BAM and every index either run left behind, not only the nine named ones
    hroot, droot, bais = str(tmp_path / "host"), str(tmp_path / "device"), 0
    for base, _, files in os.walk(hroot):
        for f in files:
            if f.endswith(".bam") or f.endswith(".bai"):
                rel = os.path.relpath(os.path.join(base, f), hroot)
                assert open(os.path.join(droot, rel), "rb").read() == open(os.path.join(hroot, rel), "rb").read(), rel
                bais += f.endswith(".bai")
    assert bais >= 1
    with pytest.raises(ValueError):
        _pipeline(engine, str(tmp_path / "gpu"), "gpu")


def test_environment_option_and_hook_ownership(engine, monkeypatch):
    """CC_INFLATE_DEVICE=1 wires a new engine's inflater; the hook has one owner, and closing an engine
    that lost it leaves the owner's hook in place."""
    from consensuscruncher_amd.engine import Engine
    want = _whole(INPUT)
    monkeypatch.setenv("CC_INFLATE_DEVICE", "1")
    first = Engine(0)
    try:
        assert first.inflate_device
        monkeypatch.delenv("CC_INFLATE_DEVICE")
        first.set_profiling(True)
        assert _whole(INPUT) == want
        assert "bgzf_inflate" in first.kernel_times()
        engine.device_inflate(True)        # the module's engine takes the hook over
        assert engine.inflate_device and not first.inflate_device
    finally:
        first.close()                      # must not unset the new owner's hook
    try:
        engine.set_profiling(True)
        assert _whole(INPUT) == want
        assert "bgzf_inflate" in engine.kernel_times(), "the owner's inflater still serves the readers"
    finally:
        engine.set_profiling(False)
        engine.device_inflate(False)
    engine.set_profiling(True)
    assert _whole(INPUT) == want
    assert "bgzf_inflate" not in engine.kernel_times(), "unwired: the host codec alone"
    engine.set_profiling(False)
