"""libccio's resident output set (ccio_set_out_resident), without a GPU: Python callbacks stand in
for the device (assemble-keep, resident deflate, index fields, fetch, release) on the first 300
records of the golden basic input, written sorted and indexed.  Whatever the set refuses or gets
wrong falls back to the host's bytes; what it gets right gives the host's records and a .bai that is
byte for byte the walk's over the same members; need_host follows the kept handle; every token is
released exactly once, also by a CCIO_W_ASYNC writer thread."""
import bisect
import ctypes as C
import os
import shutil
import struct
import zlib

import numpy as np
import pytest

import pysam  # the oracle shim
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam, Interner, Sink, flush_writes, index_bam, make_specs, write_bam
from parity import GOLDEN

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
NREC = 300


def _offsets(stream, start):
    at, a = [], start
    while a < len(stream):
        at.append(a)
        a += 4 + int.from_bytes(stream[a:a + 4], "little")
    assert a == len(stream)
    return at + [a]


def _fields(stream, at):
    """What cc_index_fields gives, restated."""
    out = np.zeros(len(at) - 1, N.INDEX_FIELD_DTYPE)
    for i, a in enumerate(at[:-1]):
        bs, tid, pos, lqn, _, _, ncig, flag = struct.unpack_from("<iiiBBHHH", stream, a)
        rl = 0
        if not flag & 4:
            for k in range(ncig):
                c = struct.unpack_from("<I", stream, a + 36 + lqn + 4 * k)[0]
                if c & 15 in (0, 2, 3, 7, 8):
                    rl += c >> 4
        out[i] = (tid, pos, bs, min(rl, 0x7fffffff) | (0x80000000 if flag & 4 else 0))
    return out


def _member(piece):
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    raw = co.compress(piece) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


class Dev(object):
    """The five callbacks and their log.  mode: "good", "refuse_assemble", "refuse_deflate",
    "refuse_fields", "bad_field", "swapped" or "header"."""

    def __init__(self, mode, stream, header_bytes):
        self.mode, self.stream, self.hb = mode, stream, header_bytes
        self.tokens, self.released, self.next = {}, [], 41
        self.need_host, self.allocs, self.deflates, self.fetches, self.field_calls = [], 0, 0, [], 0
        self.keep = (N.ASSEMBLE_KEEP_FN(self._assemble), N.DEFLATE_RESIDENT_FN(self._deflate),
                     N.INDEX_FIELDS_FN(self._index), N.RESIDENT_FETCH_FN(self._fetch), N.RESIDENT_RELEASE_FN(self._release))
        self.cb = N.ccio_out_resident(*[C.cast(f, N.P) for f in self.keep])

    def _assemble(self, user, header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
                  cons_seq_bytes, cons_qual, cons_qual_bytes, rg_blob, rg_off, n_rg, flags, alloc, actx, need_host, at,
                  total, token):
        self.need_host.append(need_host)
        if self.mode == "refuse_assemble":
            return 1
        stream = bytearray(self.stream)
        if self.mode == "header":
            stream[self.hb - 1] ^= 1
        offs = _offsets(self.stream, self.hb)
        if self.mode == "swapped":
            offs[7], offs[8] = offs[8], offs[7]
        if need_host:
            self.allocs += 1
            buf = alloc(actx, len(stream))
            if not buf:
                return 1
            C.memmove(buf, bytes(stream), len(stream))
        for i, v in enumerate(offs):
            at[i] = v
        total[0] = len(stream)
        token[0] = self.next
        self.tokens[self.next] = bytes(stream)
        self.next += 1
        return 0

    def _deflate(self, user, token, off, n, stage, slot, out_len, pieces):
        self.deflates += 1
        if self.mode == "refuse_deflate" or off % (0xff00 * 1024):
            return 1
        data = self.tokens[token][off:off + n]
        for j in range(pieces):
            m = _member(data[j * 0xff00:(j + 1) * 0xff00])
            C.memmove(stage + j * slot, m, len(m))
            out_len[j] = len(m)
        return 0

    def _index(self, user, token, at, n, fields):
        self.field_calls += 1
        if self.mode == "refuse_fields":
            return 1
        f = _fields(self.tokens[token], [at[i] for i in range(n + 1)])
        if self.mode == "bad_field":
            f[5]["block_size"] -= 3
        C.memmove(fields, f.ctypes.data, f.nbytes)
        return 0

    def _fetch(self, user, token, off, n, dst):
        self.fetches.append((off, n))
        C.memmove(dst, self.tokens[token][off:off + n], n)
        return 0

    def _release(self, user, token):
        self.released.append(token)


@pytest.fixture(scope="module")
def source():
    return Bam(INPUT)


def _sink(path, keep=False, async_writes=False):
    return Sink(fused=[path], keep=[path] if keep else [], async_writes=async_writes)


@pytest.fixture(scope="module")
def job(source, tmp_path_factory):
    """NREC raw copies of the input's first records; the host's sorted, indexed file for them."""
    sp = make_specs(NREC)
    sp["kind"] = N.OUT_RAW
    sp["src_rec"] = np.arange(NREC)
    p = str(tmp_path_factory.mktemp("host") / "host.bam")
    out = write_bam(p, source, Interner(), sp, [source], level=1, sink=_sink(p))
    stream = pysam.bgzf_decompress(open(out, "rb").read())
    hb = len(stream) - len(source.pack(np.arange(NREC, dtype=np.int64)).tobytes())
    return dict(specs=sp, bam=open(out, "rb").read(), bai=open(out + ".bai", "rb").read(), stream=stream, hb=hb)


@pytest.fixture
def wired(job):
    io = N.io()
    live = []

    def use(mode):
        d = Dev(mode, job["stream"], job["hb"])
        live.append(d)
        io.ccio_set_out_resident(C.byref(d.cb), None)
        return d
    yield use
    io.ccio_flush()
    io.ccio_set_out_resident(None, None)


def _write(source, job, tmp_path, keep=False, async_writes=False):
    p = str(tmp_path / "out.bam")
    sink = _sink(p, keep, async_writes)
    out = write_bam(p, source, Interner(), job["specs"], [source], level=1, sink=sink)
    if async_writes:
        flush_writes()
    return out, sink


def _once(d):
    assert sorted(d.released) == sorted(d.tokens) and len(set(d.released)) == len(d.released)


@pytest.mark.parametrize("mode", ["refuse_assemble", "refuse_deflate", "bad_field", "swapped", "header"])
def test_refusals_and_failed_checks_leave_the_host_bytes(wired, source, job, tmp_path, mode):
    d = wired(mode)
    out, _ = _write(source, job, tmp_path)
    assert open(out, "rb").read() == job["bam"]
    assert open(out + ".bai", "rb").read() == job["bai"]
    assert len(d.need_host) == 1
    if mode == "refuse_deflate":
        assert d.deflates >= 1 and d.field_calls == 1   # the rounds fetched, the index still from the fields
        assert any(o == 0 and n == len(job["stream"]) for o, n in d.fetches)
    _once(d)


def test_refused_fields_give_the_same_files_from_the_walk(wired, source, job, tmp_path):
    good = wired("good")
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    ref, _ = _write(source, job, tmp_path / "a")
    d = wired("refuse_fields")
    out, _ = _write(source, job, tmp_path / "b")
    assert d.field_calls == 1 and d.deflates >= 1 and (0, len(job["stream"])) in d.fetches
    assert open(out, "rb").read() == open(ref, "rb").read()
    assert open(out + ".bai", "rb").read() == open(ref + ".bai", "rb").read()
    _once(good)
    _once(d)


def _bai(path):
    b = open(path, "rb").read()
    assert b[:4] == b"BAI\x01"
    nref = struct.unpack_from("<i", b, 4)[0]
    p, refs = 8, []
    for _ in range(nref):
        nbin = struct.unpack_from("<i", b, p)[0]
        p += 4
        bins = {}
        for _ in range(nbin):
            bn, nch = struct.unpack_from("<Ii", b, p)
            p += 8
            bins[bn] = [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(nch)]
            p += 16 * nch
        nint = struct.unpack_from("<i", b, p)[0]
        p += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % nint, b, p))))
        p += 8 * nint
    return nref, refs, struct.unpack_from("<Q", b, p)[0]


def _reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _check_bai(bam, stream, hb):
    """The invariants of a .bai against the file it indexes (every record in its bin's chunks, the
    linear index below it and monotone, the pseudo-bin's counts, the no-coordinate count)."""
    raw = open(bam, "rb").read()
    blocks, off, u = [], 0, 0
    while off < len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        isize = struct.unpack_from("<I", raw, off + bsize - 4)[0]
        if isize:
            blocks.append((off, u))
            u += isize
        off += bsize
    starts = [b[1] for b in blocks]
    at = _offsets(stream, hb)
    f = _fields(stream, at)
    nref, refs, no_coor = _bai(bam + ".bai")
    assert no_coor == int((f["tid"] < 0).sum())
    for i in range(len(f)):
        tid, pos, rl = int(f["tid"][i]), int(f["pos"][i]), int(f["rl"][i]) & 0x7fffffff
        if tid < 0:
            continue
        k = bisect.bisect_right(starts, at[i]) - 1
        vo = (blocks[k][0] << 16) | (at[i] - blocks[k][1])
        bins, lin = refs[tid]
        beg = max(pos, 0)
        assert any(a <= vo < z for a, z in bins[_reg2bin(beg, beg + (rl or 1))]), (tid, pos)
        assert lin[beg >> 14] <= vo
        assert all(lin[j] <= lin[j + 1] for j in range(len(lin) - 1))
    for tid in range(nref):
        mine = f[f["tid"] == tid]
        if len(mine):
            un = int((mine["rl"] >> 31).sum())
            assert refs[tid][0][37450][1] == (len(mine) - un, un)
        else:
            assert 37450 not in refs[tid][0]


@pytest.mark.parametrize("async_writes", [False, True])
def test_zlib_deflate_gives_the_host_records_and_a_sound_index(wired, source, job, tmp_path, async_writes):
    d = wired("good")
    out, _ = _write(source, job, tmp_path, async_writes=async_writes)
    assert pysam.bgzf_decompress(open(out, "rb").read()) == job["stream"]
    assert open(out, "rb").read() != job["bam"]   # the callback's members, not the host codec's
    _check_bai(out, job["stream"], job["hb"])
    # the same members walked by the host give the same index, byte for byte
    cp = str(tmp_path / "copy.sorted.bam")
    shutil.copy(out, cp)
    index_bam(cp)
    assert open(cp + ".bai", "rb").read() == open(out + ".bai", "rb").read()
    # no host copy: nothing allocated, only the header fetched
    assert d.need_host == [0] and d.allocs == 0
    assert d.fetches == [(0, job["hb"])]
    _once(d)


def test_need_host_follows_the_kept_handle(wired, source, job, tmp_path):
    d = wired("good")
    out, sink = _write(source, job, tmp_path, keep=True)
    assert d.need_host == [1] and d.allocs == 1
    kept = sink.take(out)
    assert kept is not None and kept.n == NREC
    assert kept.pack(np.arange(NREC, dtype=np.int64)).tobytes() == job["stream"][job["hb"]:]
    assert pysam.bgzf_decompress(open(out, "rb").read()) == job["stream"]
    _once(d)
    kept.close()


def test_async_kept_write_releases_once_after_flush(wired, source, job, tmp_path):
    d = wired("good")
    out, sink = _write(source, job, tmp_path, keep=True, async_writes=True)
    assert d.need_host == [1]
    _once(d)
    assert pysam.bgzf_decompress(open(out, "rb").read()) == job["stream"]
    sink.take(out).close()


def test_set_resident_names_the_copy(source):
    io = N.io()
    tok, base = C.c_int64(0), C.c_uint64(0)
    assert io.ccio_bam_resident(source.h, C.byref(tok), C.byref(base)) == 0
    data, nbytes, rec0 = N.P(), C.c_uint64(0), C.c_uint64(0)
    assert io.ccio_bam_stream(source.h, C.byref(data), C.byref(nbytes), C.byref(rec0)) == 0
    assert io.ccio_bam_set_resident(source.h, 77, rec0.value + 1) == -1   # not where the records start
    assert io.ccio_bam_set_resident(source.h, 77, rec0.value) == 0
    assert io.ccio_bam_resident(source.h, C.byref(tok), C.byref(base)) == 1
    assert (tok.value, base.value) == (77, rec0.value)
    assert io.ccio_bam_set_resident(source.h, 0, 0) == 0
    assert io.ccio_bam_resident(source.h, C.byref(tok), C.byref(base)) == 0


def test_unset_is_the_host_writer_again(wired, source, job, tmp_path):
    d = wired("good")
    N.io().ccio_set_out_resident(None, None)
    out, _ = _write(source, job, tmp_path)
    assert d.need_host == [] and open(out, "rb").read() == job["bam"]
