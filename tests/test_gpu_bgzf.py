"""The device BGZF encoder (k_bgzf_deflate behind cc_bgzf_deflate and the writers' hook).  The
judge is Python's zlib, never the project's inflater: every member must be a well-formed BGZF
member whose raw DEFLATE payload inflates, within a 32 KiB window, to exactly its piece."""
import os
import struct
import zlib

import numpy as np
import pytest

import pysam  # the oracle shim
from parity import GOLDEN

pytestmark = pytest.mark.gpu

PIECE = 0xff00
INPUT = os.path.join(GOLDEN, "basic", "input.bam")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
OUTPUTS = ("sscs", "singleton", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction", "uncorrected",
           "dcs_sc", "all_unique")


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _rng(seed):
    return np.random.RandomState(seed)


def _random(n, seed):
    return _rng(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def _text(n, seed):
    words = [b"ACGT", b"chr1", b"\t", b"NNNN", b"IIIIHHGG", b"read", b":", b"0", b"147", b"\n", b"GATTACA", b"="]
    r = _rng(seed)
    out = bytearray()
    while len(out) < n:
        out += words[r.randint(len(words))]
        if r.randint(5) == 0:
            out.append(33 + r.randint(60))
    return bytes(out[:n])


def _bam_stream():
    raw = open(INPUT, "rb").read()
    off, out = 0, bytearray()
    while off < len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        out += zlib.decompress(raw[off + 18:off + bsize - 8], -15)
        off += bsize
    return bytes(out)


def _ladder():
    seed = _random(300, 11)
    out = bytearray(seed)
    for ln in range(3, 259):
        out += seed[:ln] + bytes([seed[ln] ^ 0x55])
    return bytes(out)


def _tail(extra):
    t = _text(500, 17)
    return t + t[100:160] + bytes(0xf0 + k for k in range(extra))


def _buffers():
    b = {}
    for n in (0, 1, 2, 3, 4, 255, 256, 257, 0xfeff, 0xff00, 0xff01, 2 * 0xff00 + 3):
        b["text%d" % n] = _text(n, n + 1)
    b["zeros"] = bytes(PIECE)
    b["random"] = _random(PIECE, 7)
    b["ladder"] = _ladder()
    for gap in (32768, 32769):
        r = _random(gap, 13)
        b["window%d" % gap] = r + r[:20000]
    for extra in range(4):
        b["tail%d" % extra] = _tail(extra)
    b["bam"] = _bam_stream()
    b["three"] = bytes(PIECE) + _random(PIECE, 19) + _bam_stream()[:PIECE]
    return b


BUFFERS = _buffers()


def _check_members(members, data, name):
    """Every assertion of the function-level contract; returns each member's block type."""
    assert len(members) == (len(data) + PIECE - 1) // PIECE, name
    btypes = []
    for j, m in enumerate(members):
        piece = data[j * PIECE:(j + 1) * PIECE]
        assert 28 <= len(m) <= 0x10000, (name, j, len(m))
        assert m[:16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0]), (name, j)
        assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m), (name, j)
        z = zlib.decompressobj(-15)
        got = z.decompress(m[18:-8])
        assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b"", (name, j)
        assert got == piece, (name, j)
        crc, isize = struct.unpack_from("<II", m, len(m) - 8)
        assert crc == zlib.crc32(piece) and isize == len(piece), (name, j)
        assert m[18] & 1, (name, j)   # one final block
        btypes.append((m[18] >> 1) & 3)
    return btypes


@pytest.mark.parametrize("name", sorted(BUFFERS))
def test_members_inflate_to_their_pieces(engine, name):
    data = BUFFERS[name]
    members = engine.bgzf_deflate(data)
    btypes = _check_members(members, data, name)
    assert engine.bgzf_deflate(data) == members, "a second call must return the same bytes"
    total = sum(len(m) for m in members)
    assert total <= len(data) + 31 * len(members), "never larger than stored"
    if name == "random":
        assert btypes == [0]
    if name == "zeros":
        assert btypes == [1] or btypes == [2]
        assert len(members[0]) < 600   # length-258 matches at distance 1: about 2 bits per 258 bytes
    if name == "bam":
        assert 2 in btypes, "real BAM bytes must take the dynamic form"
        assert total < len(data) // 2
    if name == "three":
        assert btypes[0] != 0 and btypes[1] == 0 and btypes[2] == 2


def test_zero_bytes_give_no_members(engine):
    assert engine.bgzf_deflate(b"") == []


def test_more_than_one_launch(engine):
    """More pieces than one launch holds (256): both streams and their buffers take turns."""
    bam = _bam_stream()
    data = (bam * (300 * PIECE // len(bam) + 1))[:300 * PIECE + 77]
    members = engine.bgzf_deflate(data)
    _check_members(members, data, "launches")
    assert len(members) == 301


def _pipeline(engine, tmp, bgzf):
    import json
    import shutil
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, "basic")
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    os.makedirs(tmp)
    shutil.copy(INPUT, os.path.join(tmp, "sample.bam"))
    kw["level"] = 1
    return consensus_pipeline(os.path.join(tmp, "sample.bam"), tmp, engine=engine, bgzf=bgzf, **kw)


def _fetch(path, regions):
    from consensuscruncher_amd.engine import Bam
    t, b, e = zip(*regions)
    part = Bam.open_regions(path, t, b, e)
    return [part.qname(i) for i in range(part.n)], [c.tolist() for c in part.cores()]


def test_pipeline_writes_the_same_records(engine, tmp_path, monkeypatch):
    from consensuscruncher_amd import native as N
    flags = []
    real = N.io().ccio_write_bam_ex

    def spy(*a):
        flags.append(a[13])
        return real(*a)
    monkeypatch.setattr(N.io(), "ccio_write_bam_ex", spy)
    engine.set_profiling(True)
    dev = _pipeline(engine, str(tmp_path / "device"), "device")
    times = engine.kernel_times()
    engine.set_profiling(False)
    assert not engine.bgzf_device, "the option is wired for the call only"
    assert sum(1 for f in flags if f & N.W_ASYNC) >= len(OUTPUTS) - 3, "the stage outputs are written in the background"
    host = _pipeline(engine, str(tmp_path / "host"), "host")
    assert "bgzf_deflate" in times, "the encoder's kernel ran and was timed under its scope name"
    exp = os.path.join(GOLDEN, "basic", "expected")
    differ = 0
    for k in OUTPUTS:
        a, b = pysam.sam_lines(dev[k]), pysam.sam_lines(host[k])
        assert a == b, k
        assert a == pysam.sam_lines(os.path.join(exp, k + ".bam")), k
        raw = open(dev[k], "rb").read()
        assert raw[-28:] == EOF_MEMBER, k
        differ += raw != open(host[k], "rb").read()
        if a:
            for regions in ([(0, 0, 40000)], [(0, 50000, 90000), (0, 120000, 10 ** 8)]):
                assert _fetch(dev[k], regions) == _fetch(host[k], regions), (k, regions)
    assert differ, "the device encoder wrote none of the files"


def test_option_off_leaves_the_writers_unchanged(engine, tmp_path):
    """After device_bgzf(False) a write gives the bytes of a process that never set the hook."""
    import subprocess
    import sys
    from consensuscruncher_amd.engine import Bam
    src = Bam(INPUT)
    engine.device_bgzf(True)
    on = str(tmp_path / "on.bam")
    src.write(on, level=1, index=True)
    engine.device_bgzf(False)
    off = str(tmp_path / "off.bam")
    src.write(off, level=1, index=True)
    fresh = str(tmp_path / "fresh.bam")
    code = ("import sys; sys.path[:0] = %r\n"
            "from consensuscruncher_amd.engine import Bam\n"
            "Bam(%r).write(%r, level=1, index=True)\n" % (sys.path, INPUT, fresh))
    subprocess.check_call([sys.executable, "-c", code])
    assert open(off, "rb").read() == open(fresh, "rb").read()
    assert open(off + ".bai", "rb").read() == open(fresh + ".bai", "rb").read()
    assert open(on, "rb").read() != open(off, "rb").read()
    assert pysam.sam_lines(on) == pysam.sam_lines(off)


STORED_MEMBER = PIECE + 5 + 26


def test_pieces_just_under_stored(engine):
    """A Huffman form is chosen when it is as little as one bit under the stored block, and its last
    codes then lie in the last words of the payload area.  Random bytes behind a run of k zeros: the
    dynamic block costs about 8 bits per random byte plus its header, the run saves about k bytes,
    so a sweep over k crosses the point where the two forms meet one byte at a time.  Every member
    must inflate, and the sweep must have produced Huffman members 1 to 4 bytes under stored."""
    rnd = _random(PIECE, 23)
    near = []
    for k in range(0, 400):
        data = bytes(k) + rnd[k:]
        members = engine.bgzf_deflate(data)
        btypes = _check_members(members, data, "zeros%d+random" % k)
        assert len(members[0]) <= STORED_MEMBER
        if btypes[0] != 0 and STORED_MEMBER - len(members[0]) <= 4:
            near.append((k, STORED_MEMBER - len(members[0])))
    assert near, "no Huffman member within 4 bytes of the stored size: the sweep missed the boundary"


def test_environment_option_and_hook_ownership(engine, tmp_path, monkeypatch):
    """CC_BGZF_DEVICE=1 wires a new engine's encoder; the hook has one owner, and closing an engine
    that lost it leaves the owner's hook in place."""
    from consensuscruncher_amd.engine import Bam, Engine
    src = Bam(INPUT)
    host = str(tmp_path / "host.bam")
    src.write(host, level=1)
    monkeypatch.setenv("CC_BGZF_DEVICE", "1")
    first = Engine(0)
    try:
        assert first.bgzf_device
        monkeypatch.delenv("CC_BGZF_DEVICE")
        a = str(tmp_path / "a.bam")
        src.write(a, level=1)
        assert open(a, "rb").read() != open(host, "rb").read()
        assert pysam.sam_lines(a) == pysam.sam_lines(host)
        engine.device_bgzf(True)           # the module's engine takes the hook over
        assert engine.bgzf_device and not first.bgzf_device
    finally:
        first.close()                      # must not unset the new owner's hook
    try:
        b = str(tmp_path / "b.bam")
        src.write(b, level=1)
        assert open(b, "rb").read() == open(a, "rb").read(), "the owner's encoder still serves the writers"
    finally:
        engine.device_bgzf(False)
    c = str(tmp_path / "c.bam")
    src.write(c, level=1)
    assert open(c, "rb").read() == open(host, "rb").read()
