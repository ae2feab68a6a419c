"""libccio's crc hooks (ccio_set_inflate_crc_hook, ccio_set_inflate_keep_crc_hook), without a GPU:
Python callbacks that inflate with zlib and report zlib's CRC32 of what they wrote stand in for the
device inflater and its CRC kernel.  A crc hook takes its plain sibling's place; libccio accepts a
member when the hook reports it ok and its crc equals the member's CRC32 field, and hands every other
member to the host codec (and, for a kept copy, to patch), so the readers return what they return
without any hook."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam
from parity import GOLDEN
from test_inflate_hook import Hook as PlainHook
from test_resident_hook import Keeper as PlainKeeper

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
REGIONS = ([(0, 0, 5000)], [(0, 20000, 60000), (0, 100000, 150000)])
TOKEN = 0x5eed0002


class CrcHook(object):
    """A ccio_inflate_crc_fn and its call log.  mode: "zlib" (honest), "wrong_crc" (right bytes, but
    crc[j] off by one bit for one member per call), "damaged" (one member per call written with flipped
    bits and its crc the damaged bytes' own: an honest report of wrong bytes), "refuse" (ok = 0 for
    every other member, their crc left at the field's value), "fail" (returns 1)."""

    def __init__(self, mode):
        self.mode = mode
        self.calls = 0
        self.sizes = []
        self.odd = []     # (call, member) of every member reported with a crc that is not its field
        self.bad = []
        self.fn = N.INFLATE_CRC_FN(self._call)

    def _call(self, user, comp, coff, clen, uoff, ulen, members, out, ok, crc):
        self.calls += 1
        self.sizes.append(members)
        if self.mode == "fail":
            return 1
        for j in range(members):
            if ulen[j] == 0:
                self.bad.append(("empty member handed to the hook", j))
            data = zlib.decompress(C.string_at(comp + coff[j], clen[j]), -15)
            field = int.from_bytes(C.string_at(comp + coff[j] + clen[j], 4), "little")
            if zlib.crc32(data) != field or len(data) != ulen[j]:
                self.bad.append(("the file's own member is wrong", j))
            value = zlib.crc32(data)
            if j == members // 2 and self.mode == "wrong_crc":
                value ^= 0x00010000
                self.odd.append((self.calls, j))
            if j == members // 2 and self.mode == "damaged":
                data = bytes(b ^ 0x40 if k % 61 == 0 else b for k, b in enumerate(data))
                value = zlib.crc32(data)
                self.odd.append((self.calls, j))
            C.memmove(out + uoff[j], data, len(data))
            crc[j] = value
            ok[j] = 0 if self.mode == "refuse" and j % 2 else 1
        return 0


class CrcKeeper(object):
    """A ccio_inflate_keep_crc_fn / ccio_resident_patch_fn pair: member j is refused when j % 3 == 1,
    and written right but reported with a wrong crc when j == 3 (the copy gets the same bytes)."""

    def __init__(self):
        self.keeps, self.refused, self.wrong, self.patches, self.bad = [], [], [], [], []
        self.copy = None
        self.keep = N.INFLATE_KEEP_CRC_FN(self._keep)
        self.patch = N.RESIDENT_PATCH_FN(self._patch)

    def _keep(self, user, comp, coff, clen, uoff, ulen, members, out, ok, total, token, crc):
        self.keeps.append((members, total))
        self.copy = bytearray(b"\xee" * total)
        for j in range(members):
            data = zlib.decompress(C.string_at(comp + coff[j], clen[j]), -15)
            if j % 3 == 1:
                ok[j] = 0
                crc[j] = zlib.crc32(data)   # (a refused member's crc is not read)
                self.refused.append((uoff[j], ulen[j]))
                continue
            C.memmove(out + uoff[j], data, len(data))
            self.copy[uoff[j]:uoff[j] + ulen[j]] = data if j != 3 else b"\x11" * len(data)
            crc[j] = zlib.crc32(data) ^ (1 if j == 3 else 0)
            if j == 3:
                self.wrong.append((uoff[j], ulen[j]))
            ok[j] = 1
        token[0] = TOKEN
        return 0

    def _patch(self, user, token, off, data, n):
        self.patches.append((token, off, n))
        if token != TOKEN or off + n > len(self.copy):
            self.bad.append(("patch outside the copy", token, off, n))
            return 1
        self.copy[off:off + n] = C.string_at(data, n)
        return 0


@pytest.fixture
def hooks():
    """Every inflate hook unset before and after a test; the test sets what it needs."""
    io = N.io()

    def clear():
        io.ccio_set_inflate_hook(None, None)
        io.ccio_set_inflate_crc_hook(None, None)
        io.ccio_set_inflate_keep_hook(None, None, None)
        io.ccio_set_inflate_keep_crc_hook(None, None, None)
    clear()
    yield io
    clear()


def _everything(b):
    return [b.qname(i) for i in range(b.n)], [c.tolist() for c in b.cores()], b.pack(np.arange(b.n)).tobytes()


def _regions(path, regions):
    t, b, e = zip(*regions)
    return _everything(Bam.open_regions(path, t, b, e))


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    io = N.io()
    io.ccio_set_inflate_crc_hook(None, None)
    io.ccio_set_inflate_keep_crc_hook(None, None, None)
    p = str(tmp_path_factory.mktemp("crc_hook") / "input.bam")
    src = Bam(INPUT)
    src.write(p, level=6, index=True)
    whole = _everything(Bam(p))
    assert len(whole[0]) > 1000 and whole == _everything(src)
    parts = [_regions(p, r) for r in REGIONS]
    assert all(len(x[0]) > 0 for x in parts)
    return p, whole, parts


@pytest.mark.parametrize("mode", ["zlib", "wrong_crc", "damaged", "refuse", "fail"])
def test_crc_hooked_readers_return_the_same_records(hooks, indexed, mode):
    path, whole, parts = indexed
    h = CrcHook(mode)
    hooks.ccio_set_inflate_crc_hook(C.cast(h.fn, N.P), None)
    assert _everything(Bam(path)) == whole
    whole_calls = h.calls
    assert whole_calls >= 1 and max(h.sizes) >= 2, "the whole-file open goes through the crc hook"
    for r, want in zip(REGIONS, parts):
        before = h.calls
        assert _regions(path, r) == want
        assert h.calls >= before + 2, "the header read and the region read both go through the crc hook"
    assert not h.bad
    if mode in ("wrong_crc", "damaged"):
        assert any(c <= whole_calls for c, _ in h.odd) and any(c > whole_calls for c, _ in h.odd)


def test_keep_crc_hook_patches_what_the_host_codec_inflated(hooks, indexed):
    path, whole, _ = indexed
    inflated = gzip.open(path, "rb").read()
    k = CrcKeeper()
    hooks.ccio_set_inflate_keep_crc_hook(C.cast(k.keep, N.P), C.cast(k.patch, N.P), None)
    b = Bam(path)
    assert not k.bad and len(k.keeps) == 1 and k.keeps[0][1] == len(inflated)
    assert len(k.refused) >= 1 and len(k.wrong) == 1, "the file has more than four members"
    assert sorted((o, n) for _, o, n in k.patches) == sorted(k.refused + k.wrong)
    assert all(t == TOKEN for t, _, _ in k.patches)
    assert bytes(k.copy) == inflated, "the copy, patched where the hook left it wrong, is the inflated file"
    tok, base = C.c_int64(-1), C.c_uint64(0)
    assert hooks.ccio_bam_resident(b.h, C.byref(tok), C.byref(base)) == 1 and tok.value == TOKEN
    assert _everything(b) == whole
    # the region reads and the header read keep to the plain-shaped hooks: no keep call
    assert _regions(path, REGIONS[0]) == indexed[2][0] and len(k.keeps) == 1


def test_crc_hooks_take_precedence_and_unsetting_restores_the_plain_ones(hooks, indexed):
    path, whole, parts = indexed
    plain, crc = PlainHook("zlib"), CrcHook("zlib")
    hooks.ccio_set_inflate_hook(C.cast(plain.fn, N.P), None)
    hooks.ccio_set_inflate_crc_hook(C.cast(crc.fn, N.P), None)
    assert _everything(Bam(path)) == whole and _regions(path, REGIONS[1]) == parts[1]
    assert crc.calls >= 3 and plain.calls == 0, "the crc hook stands in for the plain one"
    hooks.ccio_set_inflate_crc_hook(None, None)
    seen = crc.calls
    assert _everything(Bam(path)) == whole and _regions(path, REGIONS[1]) == parts[1]
    assert crc.calls == seen and plain.calls >= 3, "unset, the plain hook serves again"
    assert not plain.bad and not crc.bad
    # the keeping pair likewise (the whole-file open)
    pk, ck = PlainKeeper(), CrcKeeper()
    hooks.ccio_set_inflate_keep_hook(C.cast(pk.keep, N.P), C.cast(pk.patch, N.P), None)
    hooks.ccio_set_inflate_keep_crc_hook(C.cast(ck.keep, N.P), C.cast(ck.patch, N.P), None)
    assert _everything(Bam(path)) == whole
    assert len(ck.keeps) == 1 and pk.keeps == []
    hooks.ccio_set_inflate_keep_crc_hook(None, None, None)
    assert _everything(Bam(path)) == whole
    assert len(ck.keeps) == 1 and len(pk.keeps) == 1


def test_unset_crc_hook_is_never_called(hooks, indexed):
    path, whole, parts = indexed
    h = CrcHook("zlib")
    hooks.ccio_set_inflate_crc_hook(C.cast(h.fn, N.P), None)
    hooks.ccio_set_inflate_crc_hook(None, None)
    assert _everything(Bam(path)) == whole and _regions(path, REGIONS[0]) == parts[0]
    assert h.calls == 0
