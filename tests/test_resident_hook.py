"""libccio's keep hook (ccio_set_inflate_keep_hook, ccio_bam_resident), without a GPU: a Python pair
stands in for the device inflater's resident streams.  The fake keep inflates with zlib into `out`
and into a copy of its own, refuses some members and damages one; the fake patch overwrites the copy.
After a whole-file open the copy must be the inflated file, patched exactly where the fake left it
wrong, and the handle must name the copy and the offset of its first record; region opens never call
keep; a failing patch or keep leaves a handle without a token and with the right records."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam
from parity import GOLDEN

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
REGION = [(0, 20000, 60000)]
TOKEN = 0x5eed0001


class Keeper(object):
    """A ccio_inflate_keep_fn / ccio_resident_patch_fn pair and their call logs.  Member j of a keep
    call is refused (ok = 0, nothing written to the copy) when j % 3 == 1 and damaged in `out` and in
    the copy alike, yet reported ok, when j == 3; mode "fail_keep" returns 1 from keep, "fail_patch"
    from every patch."""

    def __init__(self, mode="ok"):
        self.mode = mode
        self.keeps = []      # (members, total) per keep call
        self.refused = []    # (uoff, ulen)
        self.damaged = []
        self.patches = []    # (token, off, n)
        self.copy = None
        self.bad = []        # contract violations seen inside the callbacks
        self.keep = N.INFLATE_KEEP_FN(self._keep)
        self.patch = N.RESIDENT_PATCH_FN(self._patch)

    def _keep(self, user, comp, coff, clen, uoff, ulen, members, out, ok, total, token):
        self.keeps.append((members, total))
        if self.mode == "fail_keep":
            return 1
        self.copy = bytearray(b"\xee" * total)
        for j in range(members):
            if uoff[j] + ulen[j] > total:
                self.bad.append(("member outside total", j))
            data = zlib.decompress(C.string_at(comp + coff[j], clen[j]), -15)
            if j % 3 == 1:
                ok[j] = 0
                self.refused.append((uoff[j], ulen[j]))
                continue
            if j == 3:
                data = bytes(b ^ 0x40 if k % 61 == 0 else b for k, b in enumerate(data))
                self.damaged.append((uoff[j], ulen[j]))
            C.memmove(out + uoff[j], data, len(data))
            self.copy[uoff[j]:uoff[j] + ulen[j]] = data
            ok[j] = 1
        token[0] = TOKEN
        return 0

    def _patch(self, user, token, off, data, n):
        self.patches.append((token, off, n))
        if self.mode == "fail_patch":
            return 1
        if token != TOKEN or off + n > len(self.copy):
            self.bad.append(("patch outside the copy", token, off, n))
            return 1
        self.copy[off:off + n] = C.string_at(data, n)
        return 0


@pytest.fixture
def kept():
    """Sets a keep hook (and no plain hook) for one test and always unsets it."""
    io = N.io()
    live = []

    def use(mode="ok"):
        k = Keeper(mode)
        live.append(k)
        io.ccio_set_inflate_hook(None, None)
        io.ccio_set_inflate_keep_hook(C.cast(k.keep, N.P), C.cast(k.patch, N.P), None)
        return k
    yield use
    io.ccio_set_inflate_keep_hook(None, None, None)


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    """(the golden input in members of 8 KiB, so there are many; the same written with its .bai for the
    region reads; the inflated file)"""
    N.io().ccio_set_inflate_keep_hook(None, None, None)
    p = str(tmp_path_factory.mktemp("resident") / "input.bam")
    Bam(INPUT).write(p, level=6, index=True)
    inflated = gzip.open(p, "rb").read()
    small = str(tmp_path_factory.mktemp("resident") / "small.bam")
    with open(small, "wb") as f:
        for at in range(0, len(inflated), 8192):
            piece = inflated[at:at + 8192]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            body = c.compress(piece) + c.flush()
            f.write(struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25))
            f.write(body + struct.pack("<II", zlib.crc32(piece), len(piece)))
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return small, p, inflated


def _everything(b):
    return [b.qname(i) for i in range(b.n)], [c.tolist() for c in b.cores()], b.pack(np.arange(b.n)).tobytes()


def _resident(b):
    tok, base = C.c_int64(-1), C.c_uint64(0)
    got = N.io().ccio_bam_resident(b.h, C.byref(tok), C.byref(base))
    return (tok.value, base.value) if got else None


def test_whole_file_open_keeps_and_patches(kept, indexed):
    small, _, inflated = indexed
    want = _everything(Bam(small))
    k = kept()
    b = Bam(small)
    assert not k.bad
    members = (len(inflated) + 8191) // 8192
    assert k.keeps == [(members, len(inflated))], "one keep call, the non-empty members, the file's size"
    assert len(k.refused) >= 2 and len(k.damaged) == 1
    assert sorted((o, n) for _, o, n in k.patches) == sorted(k.refused + k.damaged)
    assert all(t == TOKEN for t, _, _ in k.patches)
    assert bytes(k.copy) == inflated
    assert _everything(b) == want
    tok, base = _resident(b)
    assert tok == TOKEN
    first = b.pack([0]).tobytes()
    assert struct.unpack_from("<i", inflated, base)[0] + 4 == len(first)
    assert inflated[base:base + len(first)] == first
    assert inflated[base:] == want[2], "the records are the stream from base on"


def test_region_opens_never_call_keep(kept, indexed):
    _, p, _ = indexed
    t, b, e = zip(*REGION)
    want = _everything(Bam.open_regions(p, t, b, e))
    assert len(want[0]) > 0
    k = kept()
    r = Bam.open_regions(p, t, b, e)
    assert k.keeps == [] and k.patches == []
    assert _everything(r) == want
    assert _resident(r) is None


def test_views_and_combined_handles_have_no_token(kept, indexed):
    small = indexed[0]
    kept()
    b = Bam(small)
    assert _resident(b) is not None
    assert _resident(Bam.combine([b])) is None
    assert _resident(b.route(None)) is None


@pytest.mark.parametrize("mode", ["fail_patch", "fail_keep"])
def test_failure_leaves_no_token_and_correct_records(kept, indexed, mode):
    small = indexed[0]
    want = _everything(Bam(small))
    k = kept(mode)
    b = Bam(small)
    assert len(k.keeps) == 1
    assert len(k.patches) == (1 if mode == "fail_patch" else 0), "nothing more is patched after a failure"
    assert _resident(b) is None
    assert _everything(b) == want


def test_unset_pair_is_never_called(kept, indexed):
    small = indexed[0]
    k = kept()
    N.io().ccio_set_inflate_keep_hook(None, None, None)
    b = Bam(small)
    assert k.keeps == [] and _resident(b) is None
