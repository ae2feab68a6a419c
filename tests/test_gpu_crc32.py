"""The device CRC32 (k_crc32) behind Engine.crc32 / resident_crc32, the inflater's crc output, the
readers' crc hooks, the encoder's CRC fields and the pipeline option.  Python's zlib.crc32 is the judge
everywhere; the project's own CRC code never is.  With the switch on, every reader returns the bytes
it returns with it off and every written member is byte for byte the same."""
import contextlib
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import crc_cases as CC
import inflate_cases as IC
from consensuscruncher_amd import native as N
from parity import GOLDEN

pytestmark = pytest.mark.gpu

INPUT = IC.INPUT
PIECE = IC.PIECE
OUTPUTS = ("sscs", "singleton", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction", "uncorrected",
           "dcs_sc", "all_unique")
REGIONS = ([(0, 0, 5000)], [(0, 20000, 60000), (0, 100000, 150000)])


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def crc_on(engine, **switches):
    """device_crc on, and the other switches named (inflate, decode, resident, bgzf), for one block."""
    order = ("resident", "decode", "inflate", "bgzf")
    was_crc = engine.device_crc(True)
    was = [(k, getattr(engine, "device_" + k)(True)) for k in order if switches.get(k)]
    try:
        yield engine
    finally:
        for k, w in reversed(was):
            getattr(engine, "device_" + k)(w)
        engine.device_crc(was_crc)


def _member(stream, data, crc=None):
    """A BGZF member around a raw DEFLATE stream (ISIZE and CRC32 of data)."""
    return (struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(stream) + 25) + stream +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data)))


# ---------------------------------------------------------------- Engine.crc32
def _laid_out(name):
    """Every length at every start alignment, back to back in one buffer of content `name`: the
    buffer, the ranges and zlib's values."""
    buf, ranges, want = bytearray(), [], []
    for n in CC.LENGTHS:
        piece = CC.contents(n, seed=n + 1)[name]
        for a in CC.ALIGNS:
            buf += b"\x5a" * ((-len(buf)) % 16 + a)   # junk before the range: the first word's pad bytes
            ranges.append((len(buf), n))
            buf += piece
            want.append(zlib.crc32(piece))
    buf += b"\x5a" * 3   # and behind the last one
    return bytes(buf), ranges, want


@pytest.mark.parametrize("name", ["zeros", "ff", "random", "first_bit", "last_bit"])
def test_every_length_and_alignment(engine, name):
    buf, ranges, want = _laid_out(name)
    assert sorted(set(o % 16 for o, _ in ranges)) == list(CC.ALIGNS)
    got = engine.crc32(buf, ranges)
    bad = [(r, hex(g), hex(w)) for r, g, w in zip(ranges, got, want) if g != w]
    assert not bad, bad[:5]


def test_overlapping_ranges_and_the_whole_buffer(engine):
    buf = CC.contents(70000, seed=3)["random"]
    ranges = [(0, 70000 - 4464), (1, 65536), (1, 65535), (100, 4096), (101, 4096), (4000, 200), (4000, 200),
              (69999, 1), (70000, 0), (33333, 7)]
    assert engine.crc32(buf, ranges) == [zlib.crc32(buf[o:o + n]) for o, n in ranges]
    assert engine.crc32(buf) == [zlib.crc32(buf)]
    assert engine.crc32(b"") == [0]


def test_long_ranges_are_split_and_joined(engine):
    buf = CC.contents((1 << 20) + 3 + 29, seed=5)["random"]
    ranges = [(13, n) for n in CC.LONG] + [(0, CC.LONG[0]), (29, CC.LONG[2]), (7, 2 * 65536), (7, 2 * 65536 + 1)]
    assert engine.crc32(buf, ranges) == [zlib.crc32(buf[o:o + n]) for o, n in ranges]


def test_empty_list_and_out_of_bounds(engine):
    buf = CC.contents(1000)["random"]
    assert engine.crc32(buf, []) == []
    for bad in ([(0, 1001)], [(1001, 0)], [(10, 5), (999, 2)], [(2 ** 63, 2 ** 63)]):
        with pytest.raises(N.CCError) as e:
            engine.crc32(buf, bad)
        assert e.value.code == N.CC_E_INVALID
    assert engine.crc32(buf, [(1000, 0), (999, 1)]) == [0, zlib.crc32(buf[999:])]


def test_the_kernel_is_timed_under_its_scope(engine):
    engine.set_profiling(True)
    try:
        engine.crc32(b"abc" * 50000)
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert times["bgzf_crc32"][1] == 1 and times["bgzf_crc32"][0] > 0


# ---------------------------------------------------------------- the inflater's crc output
def test_inflater_reports_every_members_crc(engine):
    valid = [(name, _member(stream, data), data) for name, stream, data in IC.valid_streams()]
    assert any(len(d) == 0 for _, _, d in valid), "a zero-length member is among them"
    raw = b"".join(m for _, m, _ in valid)
    data, ok, crcs = engine.bgzf_inflate(raw, crc=True)
    assert all(ok) and len(ok) == len(valid)
    assert data == b"".join(d for _, _, d in valid)
    bad = [valid[j][0] for j, c in enumerate(crcs) if c != zlib.crc32(valid[j][2])]
    assert not bad, bad
    assert engine.bgzf_inflate(raw, crc=True) == (data, ok, crcs), "a second call must return the same values"
    assert engine.bgzf_inflate(raw) == (data, ok)


def test_crcs_over_more_members_than_one_round(engine):
    """1,100 small members: two rounds, both streams and both CRC buffers take turns."""
    r = np.random.RandomState(43)
    src = IC.bam_stream()
    parts = []
    for j in range(1100):
        n = 200 + int(r.randint(400))
        o = int(r.randint(len(src) - n))
        parts.append(src[o:o + n])
    raw = b"".join(_member(IC.raw_deflate(p, (1, 6, 9, 0)[j % 4]), p) for j, p in enumerate(parts))
    got, ok, crcs = engine.bgzf_inflate(raw, crc=True)
    assert len(ok) == 1100 and all(ok) and got == b"".join(parts)
    assert crcs == [zlib.crc32(p) for p in parts]
    assert engine.bgzf_inflate(raw, crc=True) == (got, ok, crcs)


# ---------------------------------------------------------------- resident streams
def _keep_crc(engine, parts):
    """parts kept at odd offsets of a resident stream by cc_bgzf_inflate_keep_crc: uoff, total, out, ok, crc, id."""
    comp, coff, clen, uoff, ulen = bytearray(), [], [], [], []
    at = 3
    for j, p in enumerate(parts):
        s = IC.raw_deflate(p, (1, 6)[j % 2])
        comp += b"\xee" * (j % 3)
        coff.append(len(comp))
        clen.append(len(s))
        comp += s
        uoff.append(at)
        ulen.append(len(p))
        at += len(p) + 1 + 2 * (j % 4)
    total = at + 5
    a = [np.asarray(v, t) for v, t in ((coff, np.uint64), (clen, np.uint32), (uoff, np.uint64), (ulen, np.uint32))]
    out = np.full(total, 0xc3, np.uint8)
    ok = np.full(len(parts), 7, np.uint8)
    crc = np.full(len(parts), 0xdeadbeef, np.uint32)
    rid = C.c_int64(-5)
    compa = np.frombuffer(bytes(comp), np.uint8)
    bad = engine.lib.cc_bgzf_inflate_keep_crc(engine.h, N.ptr(compa), N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), N.ptr(a[3]),
                                              len(parts), N.ptr(out), N.ptr(ok), total, C.byref(rid), N.ptr(crc))
    assert int(bad) == 0 and ok.tolist() == [1] * len(parts) and rid.value > 0
    return uoff, total, out, [int(c) for c in crc], int(rid.value)


def test_resident_stream_crcs(engine):
    src = IC.bam_stream()
    parts = [src[:PIECE], IC.text(777, 5), src[1000:1000 + 65536], IC.random_bytes(4081, 9), b"x", src[5:5 + 4097],
             IC.text(33, 6)]
    uoff, total, out, crcs, rid = _keep_crc(engine, parts)
    fields = [zlib.crc32(p) for p in parts]   # what a member's CRC32 field holds
    try:
        assert len(set(o % 16 for o in uoff)) >= 4 and any(o % 2 for o in uoff), "members at odd offsets"
        for p, o in zip(parts, uoff):
            assert out[o:o + len(p)].tobytes() == p
        assert crcs == fields, "the CRCs the rounds' kernels took from the resident stream"
        ranges = [(o, len(p)) for o, p in zip(uoff, parts)]
        assert engine.resident_crc32(rid, ranges) == fields
        assert engine.resident_crc32(rid, []) == []
        # a patched range: the new bytes' CRC
        new = IC.random_bytes(len(parts[1]), 77)
        buf = np.frombuffer(new, np.uint8)
        assert engine.lib.cc_resident_patch(engine.h, rid, uoff[1], N.ptr(buf), buf.size) == 0
        got = engine.resident_crc32(rid, ranges)
        assert got[1] == zlib.crc32(new) != fields[1] and got[:1] + got[2:] == fields[:1] + fields[2:]
        # a range that spans members and gaps: the host splits it; the resident bytes are the judge's input
        whole = np.zeros(total, np.uint8)
        assert int(engine.lib.cc_resident_fetch(engine.h, rid, N.ptr(whole), total)) == total
        assert engine.resident_crc32(rid, [(1, total - 1)]) == [zlib.crc32(whole[1:].tobytes())]
        with pytest.raises(N.CCError) as e:
            engine.resident_crc32(rid, [(total, 1)])
        assert e.value.code == N.CC_E_INVALID
    finally:
        assert engine.lib.cc_resident_free(engine.h, rid) == 0
    with pytest.raises(N.CCError) as e:
        engine.resident_crc32(rid, [(0, 1)])
    assert e.value.code == N.CC_E_INVALID
    assert int(engine.lib.cc_resident_count(engine.h)) == 0


# ---------------------------------------------------------------- readers
def _everything(b):
    return [b.qname(i) for i in range(b.n)], [c.tolist() for c in b.cores()], b.pack(np.arange(b.n)).tobytes()


def _reads(path):
    from consensuscruncher_amd.engine import Bam
    out = [_everything(Bam(path))]
    for r in REGIONS:
        t, b, e = zip(*r)
        out.append(_everything(Bam.open_regions(path, t, b, e)))
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The golden input written sorted with its index (several members), and a copy of it with the
    CRC32 field of its second member flipped (the index is the same: no payload moved)."""
    from consensuscruncher_amd.engine import Bam
    d = tmp_path_factory.mktemp("crc_readers")
    good = str(d / "input.bam")
    Bam(INPUT).write(good, level=6, index=True)
    raw = bytearray(open(good, "rb").read())
    off = struct.unpack_from("<H", raw, 16)[0] + 1
    bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
    assert bsize > 1000 and off + bsize < len(raw) - 28, "a full member in the middle of the file"
    raw[off + bsize - 8] ^= 0x01
    flipped = str(d / "flipped.bam")
    open(flipped, "wb").write(bytes(raw))
    open(flipped + ".bai", "wb").write(open(good + ".bai", "rb").read())
    return good, flipped


def test_readers_return_the_same_bytes(engine, files):
    good, flipped = files
    want = _reads(good)
    assert len(want[0][0]) > 1000 and all(len(w[0]) > 0 for w in want)
    assert _reads(flipped) == want, "the host codec checks no CRC: today's outcome for the flipped file"
    engine.set_profiling(True)
    try:
        with crc_on(engine, inflate=True):
            assert engine.crc_device and engine.inflate_device
            assert _reads(good) == want
            times = engine.kernel_times()
            assert _reads(flipped) == want, "the host codec takes the member whose field differs"
            # toggled while the hook is wired: the plain hook serves again, then the crc hook
            assert engine.device_crc(False) is True
            n = engine.kernel_times()["bgzf_crc32"][1]
            assert _reads(good) == want and engine.kernel_times()["bgzf_crc32"][1] == n
            assert engine.device_crc(True) is False
            assert _reads(good) == want and engine.kernel_times()["bgzf_crc32"][1] > n
    finally:
        engine.set_profiling(False)
    assert times["bgzf_crc32"][1] >= 1 and times["bgzf_crc32"][1] == times["bgzf_inflate"][1]
    assert not engine.crc_device and not engine.inflate_device
    assert _reads(good) == want, "and with everything unwired again"


@pytest.mark.parametrize("which", ["good", "flipped"])
def test_resident_table_equals_the_host_table(engine, files, which):
    from consensuscruncher_amd.engine import Bam, Interner
    from test_gpu_resident import assert_same_tables, count, host_table
    path = files[which == "flipped"]
    hb = Bam(path)
    rec, host = host_table(engine, hb, Interner())
    dev = None
    try:
        engine.set_profiling(True)
        with crc_on(engine, resident=True, decode=True, inflate=True):
            bam = Bam(path)
            assert bam.resident() is not None and count(engine) == 1
            assert _everything(bam) == _everything(hb)
            drec, dev = engine.unpack(bam, Interner(), 0)
            times = engine.kernel_times()
        assert count(engine) == 0
        assert times["bgzf_crc32"][1] >= 1 and times.get("unpack_stream_upload", (0.0, 0))[1] == 0
        assert drec.n == rec.n
        assert_same_tables(engine, dev, host, rec)
    finally:
        engine.set_profiling(False)
        engine.free_table(host)
        if dev is not None:
            engine.free_table(dev)


def test_switch_alone_and_the_environment(engine, monkeypatch):
    from consensuscruncher_amd.engine import Engine
    assert engine.device_crc(True) is False and engine.device_crc(True) is True   # nothing wired: no effect, no error
    assert not engine.inflate_device and not engine.bgzf_device
    assert engine.device_crc(False) is True
    monkeypatch.setenv("CC_CRC_DEVICE", "1")
    e = Engine(0)
    try:
        assert e.crc_device and not e.inflate_device
    finally:
        e.close()
    assert not engine.crc_device


# ---------------------------------------------------------------- encoder
@pytest.mark.parametrize("effort", [1, 2])
def test_encoder_members_are_identical_and_their_fields_zlibs(engine, effort):
    data = IC.bam_stream()[:3 * PIECE + 123] + bytes(PIECE) + IC.random_bytes(PIECE, 41) + IC.text(777, 3)
    pieces = [data[o:o + PIECE] for o in range(0, len(data), PIECE)]
    host = engine.bgzf_deflate(data, effort=effort)
    engine.set_profiling(True)
    try:
        with crc_on(engine):
            dev = engine.bgzf_deflate(data, effort=effort)
            times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert times["bgzf_crc32"][1] == times["bgzf_deflate"][1] >= 1
    assert len(dev) == len(pieces) >= 6
    for j, (m, p) in enumerate(zip(dev, pieces)):
        assert struct.unpack_from("<II", m, len(m) - 8) == (zlib.crc32(p), len(p)), j
        assert zlib.decompress(m[18:-8], -15) == p, j
    assert dev == host
    assert engine.bgzf_deflate(b"", effort=effort) == []


# ---------------------------------------------------------------- pipeline
def _pipeline(engine, tmp, **options):
    import json
    import shutil
    from consensuscruncher_amd.pipeline import consensus_pipeline
    kw = dict(json.load(open(os.path.join(GOLDEN, "basic", "params.json")))["run"])
    os.makedirs(tmp)
    shutil.copy(INPUT, os.path.join(tmp, "sample.bam"))
    kw["level"] = 1
    kw.update(options)
    return consensus_pipeline(os.path.join(tmp, "sample.bam"), tmp, engine=engine, **kw)


def test_pipeline_outputs_are_byte_identical(engine, tmp_path):
    engine.set_profiling(True)
    try:
        dev = _pipeline(engine, str(tmp_path / "device"), crc="device", inflate="device", bgzf="device")
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert not engine.crc_device and not engine.inflate_device and not engine.bgzf_device, "wired for the call only"
    assert times["bgzf_crc32"][1] >= 2, "the CRC kernel ran for the readers and the writers"
    host = _pipeline(engine, str(tmp_path / "host"), crc="host", inflate="device", bgzf="device")
    for k in OUTPUTS:
        assert open(dev[k], "rb").read() == open(host[k], "rb").read(), k
    with pytest.raises(ValueError):
        _pipeline(engine, str(tmp_path / "gpu"), crc="gpu")
