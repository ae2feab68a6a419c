"""libccio's deflate hook (ccio_set_deflate_hook), without a GPU: a Python callback that compresses
with zlib level 1 stands in for the device encoder.  A file written through the hook holds the
input's records and a working index; a hook that fails or reports an impossible size leaves the
bytes the host encoder writes; level 0 never reaches the hook."""
import ctypes as C
import os
import struct
import zlib

import pytest

import pysam  # the oracle shim
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam
from parity import GOLDEN

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
PIECE = 0xff00


def _member(piece):
    z = zlib.compressobj(1, zlib.DEFLATED, -15)
    body = z.compress(piece) + z.flush()
    return (struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(body) + 25) + body +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


class Hook(object):
    """A ccio_deflate_fn and its call log; mode: "zlib", "fail" (returns 1) or "oversize"."""

    def __init__(self, mode):
        self.mode = mode
        self.calls = 0
        self.pieces = 0
        self.bad = []   # contract violations seen inside the callback (ctypes swallows exceptions there)
        self.fn = N.DEFLATE_FN(self._call)   # held as long as the hook may be called

    def _call(self, user, data, n, stage, slot, out_len, pieces):
        self.calls += 1
        if self.mode == "fail":
            return 1
        raw = C.string_at(data, n)
        if pieces != (n + PIECE - 1) // PIECE or slot < 0x10000 or pieces > 1024:
            self.bad.append((n, slot, pieces))
            return 1
        for j in range(pieces):
            m = _member(raw[j * PIECE:(j + 1) * PIECE])
            C.memmove(stage + j * slot, m, len(m))
            out_len[j] = 0x10001 if self.mode == "oversize" and j == pieces - 1 else len(m)
        self.pieces += pieces
        return 0


@pytest.fixture
def hooked():
    """Sets a hook for one test and always unsets it."""
    io = N.io()
    live = []

    def use(mode):
        h = Hook(mode)
        live.append(h)
        io.ccio_set_deflate_hook(C.cast(h.fn, N.P), None)
        return h
    yield use
    io.ccio_flush()
    io.ccio_set_deflate_hook(None, None)


@pytest.fixture(scope="module")
def source():
    b = Bam(INPUT)
    assert b.is_sorted(1) and b.n > 1000
    return b


@pytest.fixture(scope="module")
def host_bytes(source, tmp_path_factory):
    """What the host encoder writes with no hook set (level 1), file and index."""
    p = str(tmp_path_factory.mktemp("host") / "host.bam")
    source.write(p, level=1, index=True)
    return open(p, "rb").read(), open(p + ".bai", "rb").read()


def _members(raw):
    off, out = 0, []
    while off < len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        out.append(raw[off:off + bsize])
        off += bsize
    assert off == len(raw)
    return out


def _region_lines(path, regions):
    t, b, e = zip(*regions)
    part = Bam.open_regions(path, t, b, e)
    return [part.qname(i) for i in range(part.n)], part.cores()


def test_hooked_write_keeps_records_and_index(hooked, source, host_bytes, tmp_path):
    h = hooked("zlib")
    p = str(tmp_path / "hooked.bam")
    source.write(p, level=1, index=True)
    assert h.calls >= 1 and h.pieces >= 2 and not h.bad
    raw = open(p, "rb").read()
    assert raw != host_bytes[0], "the hook's members were not used"
    ms = _members(raw)
    assert ms[-1] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    # every other member is the callback's, byte for byte
    assert all(m == _member(zlib.decompress(m[18:-8], -15)) for m in ms[:-1])
    assert pysam.sam_lines(p) == pysam.sam_lines(INPUT)
    # the index addresses the hook's members: region fetches equal those on the host-written file
    hp = str(tmp_path / "host.bam")
    open(hp, "wb").write(host_bytes[0])
    open(hp + ".bai", "wb").write(host_bytes[1])
    for regions in ([(0, 0, 5000)], [(0, 20000, 60000), (0, 100000, 150000)]):
        got, want = _region_lines(p, regions), _region_lines(hp, regions)
        assert got[0] == want[0] and len(want[0]) > 0
        assert all((a == b).all() for a, b in zip(got[1], want[1]))


@pytest.mark.parametrize("mode", ["fail", "oversize"])
def test_rejected_hook_leaves_the_host_bytes(hooked, source, host_bytes, tmp_path, mode):
    h = hooked(mode)
    p = str(tmp_path / "fallback.bam")
    source.write(p, level=1, index=True)
    assert h.calls >= 1
    assert open(p, "rb").read() == host_bytes[0]
    assert open(p + ".bai", "rb").read() == host_bytes[1]


def test_write_all_through_the_hook(hooked, source, host_bytes, tmp_path):
    h = hooked("zlib")
    p = str(tmp_path / "all.bam")
    source.write_all(p, level=1)
    assert h.calls >= 1 and h.pieces >= 2 and not h.bad
    assert pysam.sam_lines(p) == pysam.sam_lines(INPUT)
    # an index built over the hook's members serves region fetches
    from consensuscruncher_amd.engine import index_bam
    index_bam(p)
    hp = str(tmp_path / "host.bam")
    open(hp, "wb").write(host_bytes[0])
    open(hp + ".bai", "wb").write(host_bytes[1])
    for regions in ([(0, 0, 5000)], [(0, 20000, 60000), (0, 100000, 150000)]):
        got, want = _region_lines(p, regions), _region_lines(hp, regions)
        assert got[0] == want[0] and len(want[0]) > 0
        assert all((a == b).all() for a, b in zip(got[1], want[1]))


def test_level_0_never_calls_the_hook(hooked, source, tmp_path):
    h = hooked("zlib")
    p = str(tmp_path / "stored.bam")
    source.write(p, level=0)
    assert h.calls == 0
    assert pysam.sam_lines(p) == pysam.sam_lines(INPUT)


def test_unset_hook_is_the_host_encoder_again(hooked, source, host_bytes, tmp_path):
    h = hooked("zlib")
    N.io().ccio_set_deflate_hook(None, None)
    p = str(tmp_path / "unset.bam")
    source.write(p, level=1, index=True)
    assert h.calls == 0
    assert open(p, "rb").read() == host_bytes[0]
