"""libccio's inflate hook (ccio_set_inflate_hook), without a GPU: a Python callback that inflates with
zlib stands in for the device inflater.  The hooked readers return what the unhooked ones return; a
callback that writes wrong bytes is caught by the CRC32 check; a member the callback refuses, or a
nonzero return, is inflated by the host codec; a genuinely corrupt file fails the same way with and
without the hook."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam
from parity import GOLDEN

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
REGIONS = ([(0, 0, 5000)], [(0, 20000, 60000), (0, 100000, 150000)])


class Hook(object):
    """A ccio_inflate_fn and its call log; mode: "zlib", "corrupt" (flips a bit in every 61st byte of
    one member per call, more often than once a record, and still reports it ok), "refuse" (ok = 0
    for every other member) or "fail" (returns 1)."""

    def __init__(self, mode):
        self.mode = mode
        self.calls = 0
        self.members = 0
        self.sizes = []   # members per call
        self.corrupted = []   # (call, member, bytes flipped) of every member "corrupt" damaged
        self.bad = []     # contract violations seen inside the callback (ctypes swallows exceptions there)
        self.fn = N.INFLATE_FN(self._call)   # held as long as the hook may be called

    def _call(self, user, comp, coff, clen, uoff, ulen, members, out, ok):
        self.calls += 1
        self.sizes.append(members)
        if self.mode == "fail":
            return 1
        for j in range(members):
            if ulen[j] == 0:
                self.bad.append(("empty member handed to the hook", j))
            try:
                data = zlib.decompress(C.string_at(comp + coff[j], clen[j]), -15)
            except zlib.error:
                ok[j] = 0
                continue
            if len(data) != ulen[j]:
                ok[j] = 0
                continue
            if self.mode == "corrupt" and j == members // 2:
                bad = bytearray(data)
                for k in range(0, len(bad), 61):
                    bad[k] ^= 0x40
                data = bytes(bad)
                self.corrupted.append((self.calls, j, len(range(0, len(bad), 61))))
            C.memmove(out + uoff[j], data, len(data))
            ok[j] = 0 if self.mode == "refuse" and j % 2 else 1
        self.members += members
        return 0


@pytest.fixture
def hooked():
    """Sets a hook for one test and always unsets it."""
    io = N.io()
    live = []

    def use(mode):
        h = Hook(mode)
        live.append(h)
        io.ccio_set_inflate_hook(C.cast(h.fn, N.P), None)
        return h
    yield use
    io.ccio_set_inflate_hook(None, None)


def _everything(b):
    """Names, cores and every byte of every record (sequence, qualities and tags included)."""
    return [b.qname(i) for i in range(b.n)], [c.tolist() for c in b.cores()], b.pack(np.arange(b.n)).tobytes()


def _whole(path):
    return _everything(Bam(path))


def _regions(path, regions):
    t, b, e = zip(*regions)
    return _everything(Bam.open_regions(path, t, b, e))


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    """The golden input written sorted with its .bai (the region reads need one), several members long."""
    N.io().ccio_set_inflate_hook(None, None)
    p = str(tmp_path_factory.mktemp("indexed") / "input.bam")
    src = Bam(INPUT)
    assert src.is_sorted(1)
    src.write(p, level=6, index=True)
    return p


@pytest.fixture(scope="module")
def unhooked(indexed):
    whole = _whole(indexed)
    assert len(whole[0]) > 1000 and whole == _whole(INPUT)
    parts = [_regions(indexed, r) for r in REGIONS]
    assert all(len(p[0]) > 0 for p in parts)
    return whole, parts


@pytest.mark.parametrize("mode", ["zlib", "corrupt", "refuse", "fail"])
def test_hooked_readers_return_the_same_records(hooked, indexed, unhooked, mode):
    h = hooked(mode)
    assert _whole(indexed) == unhooked[0]
    whole_calls = h.calls
    assert whole_calls >= 1 and max(h.sizes) >= 2, "the whole-file open goes through the hook"
    for r, want in zip(REGIONS, unhooked[1]):
        before = h.calls
        assert _regions(indexed, r) == want
        assert h.calls >= before + 2, "the header read and the region read both go through the hook"
    assert not h.bad
    if mode != "fail":
        assert h.members >= 2
    if mode == "corrupt":
        # the whole-file open had a damaged member, and so had the region reads (not only their header reads)
        assert any(c <= whole_calls and n >= 100 for c, _, n in h.corrupted), h.corrupted
        assert sum(1 for c, _, n in h.corrupted if c > whole_calls and n >= 100) >= 1, h.corrupted


def test_unset_hook_is_never_called(hooked, indexed, unhooked):
    h = hooked("zlib")
    N.io().ccio_set_inflate_hook(None, None)
    assert _whole(indexed) == unhooked[0]
    assert _regions(indexed, REGIONS[0]) == unhooked[1][0]
    assert h.calls == 0


def _break_a_member(tmp_path):
    """INPUT with the payload of its second member made undecodable (block type 3)."""
    raw = bytearray(open(INPUT, "rb").read())
    off = struct.unpack_from("<H", raw, 16)[0] + 1   # the second member
    assert struct.unpack_from("<H", raw, off + 16)[0] + 1 > 100
    raw[off + 18] |= 0x06
    p = str(tmp_path / "broken.bam")
    open(p, "wb").write(bytes(raw))
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(raw[off + 18:off + 60]), -15)
    return p


def test_corrupt_file_fails_the_same_hooked_or_not(hooked, tmp_path):
    p = _break_a_member(tmp_path)
    with pytest.raises(Exception) as plain:
        Bam(p)
    h = hooked("zlib")
    with pytest.raises(Exception) as with_hook:
        Bam(p)
    assert h.calls >= 1
    assert type(with_hook.value) is type(plain.value) and str(with_hook.value) == str(plain.value)
    assert "inflate failed" in str(plain.value)
