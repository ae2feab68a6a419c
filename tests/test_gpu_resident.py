"""Resident streams: the device inflater's output kept on the device (cc_bgzf_inflate_keep,
cc_resident_*) and read in place by the record unpacker (cc_table_unpack_resident), through libccio's
keep hook and Engine.device_resident.

With inflate, decode and resident on, a whole-file open followed by Engine.unpack must give the table
Bam.decode + Engine.upload give, byte for byte, without the record stream's upload (the profiling
scope unpack_stream_upload stays empty).  The resident stream itself is compared with zlib's bytes for
members of 0xff00 bytes, of odd sizes (offsets on no 16-B multiple, records straddling members) and for
more members than one round; members far apart or out of order close a round.  Refused members are
patched, bad arguments are CC_E_INVALID without a fault, and every path that has no resident stream
(regions, combined handles, the inflater off) gives today's table and leaves no stream behind."""
import contextlib
import ctypes as C
import json
import os
import shutil
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as IC
import unpack_cases as UC
from consensuscruncher_amd import native as N
from parity import GOLDEN

pytestmark = pytest.mark.gpu

CC_E_INVALID = -1
UPLOAD = "unpack_stream_upload"
# the column list of test_gpu_unpack.assert_same_tables
BASE = (("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("tlen", np.int32),
        ("flag", np.uint16), ("mapq", np.uint8), ("cigar_id", np.int32), ("qlen", np.int32), ("lseq", np.int32),
        ("bc_id", np.int32), ("rg_id", np.int32), ("rflags", np.uint8), ("qn_off", np.uint64), ("qn_len", np.uint16),
        ("pay_off", np.uint64), ("rdig", np.uint64))
BLOBS = ("qn_blob", "payload")
DERIVED = (("rkey", np.uint64), ("meta", np.uint32), ("core", np.int32), ("qn_ol", np.uint64), ("qdig", np.uint64),
           ("rdeep", np.uint8), ("ext", np.int32))
OUTPUTS = ("sscs", "singleton", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction", "uncorrected",
           "dcs_sc", "all_unique")


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def switched(engine, inflate=True, decode=True, resident=True):
    was = engine.device_resident(resident), engine.device_decode(decode), engine.device_inflate(inflate)
    try:
        yield engine
    finally:
        engine.device_inflate(was[2])
        engine.device_decode(was[1])
        engine.device_resident(was[0])


def count(engine):
    return int(engine.lib.cc_resident_count(engine.h))


def fetch(engine, rid):
    total = int(engine.lib.cc_resident_fetch(engine.h, rid, None, 0))
    assert total >= 0, total
    buf = np.zeros(max(total, 1), np.uint8)
    assert int(engine.lib.cc_resident_fetch(engine.h, rid, N.ptr(buf), total)) == total
    return buf[:total].tobytes()


def host_table(engine, bam, it, mode=0, delim="|"):
    """Bam.decode without the decoder's layout, uploaded: the derived columns are k_derive's."""
    from consensuscruncher_amd.engine import Records
    qn, pay, ml = C.c_uint64(), C.c_uint64(), C.c_int32()
    N.io().ccio_bam_layout(bam.h, C.byref(qn), C.byref(pay), C.byref(ml), 0)
    rec = Records(bam.n, qn.value, pay.value, ml.value, nref=len(bam.refs), derived=False)
    assert N.io().ccio_bam_decode(bam.h, it.h, mode, delim.encode(), C.byref(rec.struct), 0) == 0
    return rec, engine.upload(rec)


def assert_same_tables(engine, dev, host, rec=None):
    from consensuscruncher_amd.engine import coord_sorted
    for name, dt in BASE:
        a, b = engine.table_column(dev, name, dt), engine.table_column(host, name, dt)
        assert a.shape == b.shape and np.array_equal(a, b), name
        if rec is not None:
            assert np.array_equal(b, getattr(rec, name)[:rec.n]), name
    for name in BLOBS:
        a, b = engine.table_column(dev, name, np.uint8), engine.table_column(host, name, np.uint8)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
        if rec is not None:
            assert a.tobytes() == getattr(rec, name).tobytes(), name
    for name, dt in DERIVED:
        if name == "ext" and rec is not None and not coord_sorted(rec):
            continue
        a, b = engine.table_column(dev, name, dt), engine.table_column(host, name, dt)
        assert a.shape == b.shape and np.array_equal(a, b), name
    a, b = engine.table_column(dev, "dlist", np.int32), engine.table_column(host, "dlist", np.int32)
    assert np.array_equal(np.sort(a), np.sort(b)), "dlist"


def uploads(engine):
    return engine.kernel_times().get(UPLOAD, (0.0, 0))[1]


def check_bam(engine, path, expect_resident=True):
    """path's table by the host decoder (every switch off) against Engine.unpack with all three on."""
    from consensuscruncher_amd.engine import Bam, Interner
    hb = Bam(path)
    assert hb.resident() is None and count(engine) == 0
    rec, host = host_table(engine, hb, Interner())
    with switched(engine):
        engine.set_profiling(True)
        try:
            bam = Bam(path)
            assert (bam.resident() is not None) == expect_resident
            assert count(engine) == (1 if expect_resident else 0)
            drec, dev = engine.unpack(bam, Interner(), 0)
            times = engine.kernel_times()
        finally:
            engine.set_profiling(False)
        assert count(engine) == 0 and bam.resident() is None, "unpack frees the stream"
    try:
        assert drec.n == rec.n and drec.max_len == rec.max_len
        assert times.get(UPLOAD, (0.0, 0))[1] == 0, "the record stream was uploaded"
        assert (rec.n == 0) or "k_unpack_copy" in times
        assert_same_tables(engine, dev, host, rec)
    finally:
        engine.free_table(host)
        engine.free_table(dev)
    return rec


# ---------------------------------------------------------------- byte identity
def test_shapes_unpack_from_the_resident_stream(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam, Interner
    path = UC.write_bam(str(tmp_path / "shapes.bam"), UC.shapes())
    rec = check_bam(engine, path)
    assert rec.n == len(UC.shapes())
    # resident off, the other two on: the parent's path, which uploads the stream
    with switched(engine, resident=False):
        engine.set_profiling(True)
        try:
            bam = Bam(path)
            assert bam.resident() is None and count(engine) == 0
            drec, dev = engine.unpack(bam, Interner(), 0)
            assert uploads(engine) >= 1
        finally:
            engine.set_profiling(False)
    engine.free_table(dev)


@pytest.mark.parametrize("n", [0, 1, 257, 4097])
def test_record_counts_unpack_from_the_resident_stream(engine, tmp_path, n):
    rec = check_bam(engine, UC.write_bam(str(tmp_path / "n.bam"), UC.many(n, 100 + n, deep_at=True)))
    assert rec.n == n


# ---------------------------------------------------------------- member geometry
def _layout(parts, gap):
    """Raw DEFLATE members of parts and their places in an output with gaps: comp, coff, clen, uoff, ulen, total."""
    comp, coff, clen, uoff, ulen = bytearray(), [], [], [], []
    at = 0
    for j, p in enumerate(parts):
        s = IC.raw_deflate(p, (1, 6)[j % 2])
        comp += b"\xee" * (j % 3)
        coff.append(len(comp))
        clen.append(len(s))
        comp += s
        uoff.append(at)
        ulen.append(len(p))
        at += len(p) + gap(j)
    return bytes(comp), coff, clen, uoff, ulen, at + 64


def keep(engine, comp, coff, clen, uoff, ulen, out, total):
    a = [np.asarray(v if len(v) else [0], t) for v, t in ((coff, np.uint64), (clen, np.uint32), (uoff, np.uint64),
                                                         (ulen, np.uint32))]
    ok = np.full(max(len(coff), 1), 7, np.uint8)
    comp = np.frombuffer(comp, np.uint8)
    rid = C.c_int64(-5)
    bad = engine.lib.cc_bgzf_inflate_keep(engine.h, N.ptr(comp), N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), N.ptr(a[3]),
                                          len(coff), N.ptr(out), N.ptr(ok), int(total), C.byref(rid))
    return int(bad), ok[:len(coff)], int(rid.value)


def _check_kept(engine, parts, gap):
    comp, coff, clen, uoff, ulen, total = _layout(parts, gap)
    out = np.full(total, 0xc3, np.uint8)
    bad, ok, rid = keep(engine, comp, coff, clen, uoff, ulen, out, total)
    assert bad == 0 and ok.tolist() == [1] * len(parts) and rid > 0
    try:
        res = fetch(engine, rid)
        assert len(res) == total
        covered = np.zeros(total, bool)
        for j, (p, o) in enumerate(zip(parts, uoff)):
            assert res[o:o + len(p)] == p, ("resident", j)
            assert out[o:o + len(p)].tobytes() == p, ("out", j)
            covered[o:o + len(p)] = True
        assert (out[~covered] == 0xc3).all(), "bytes outside the members' ranges of out were written"
    finally:
        assert engine.lib.cc_resident_free(engine.h, rid) == 0
    assert count(engine) == 0
    return uoff


def _cut(data, sizes):
    parts, at, j = [], 0, 0
    while at < len(data):
        parts.append(data[at:at + sizes[j % len(sizes)]])
        at += len(parts[-1])
        j += 1
    return parts


@pytest.fixture(scope="module")
def source():
    src = IC.bam_stream()
    return (src * (1100 * 4096 // len(src) + 1))[:1100 * 4096]


def test_members_of_ff00_bytes(engine, source):
    _check_kept(engine, _cut(source[:5 * 0xff00 + 777], [0xff00]), lambda j: 0)


def test_members_of_odd_sizes_and_offsets(engine, source):
    parts = _cut(source[:400000], [1, 17, 65279, 65280])
    uoff = _check_kept(engine, parts, lambda j: (5, 0, 37)[j % 3])
    assert len({o % 16 for o in uoff}) >= 4 and len(parts) >= 10


def test_more_members_than_one_round(engine, source):
    parts = _cut(source, [4096])
    assert len(parts) == 1100
    _check_kept(engine, parts, lambda j: j % 2)


def test_far_and_out_of_order_members_close_a_round(engine):
    """A member more than a round's output span (64 MiB) above the round's base, and one below it."""
    parts = [IC.text(3000, 71), IC.text(500, 72), IC.random_bytes(4000, 73), IC.text(100, 74)]
    far = (70 << 20) + 3
    uoff = [200, far, 7000, 5]
    comp, coff, clen, ulen = bytearray(), [], [], []
    for p in parts:
        s = IC.raw_deflate(p, 6)
        coff.append(len(comp))
        clen.append(len(s))
        comp += s
        ulen.append(len(p))
    total = far + 1000
    out = np.full(total, 0xc3, np.uint8)
    bad, ok, rid = keep(engine, bytes(comp), coff, clen, uoff, ulen, out, total)
    assert bad == 0 and ok.tolist() == [1, 1, 1, 1] and rid > 0
    res = fetch(engine, rid)
    assert engine.lib.cc_resident_free(engine.h, rid) == 0
    covered = np.zeros(total, bool)
    for p, o in zip(parts, uoff):
        assert res[o:o + len(p)] == p and out[o:o + len(p)].tobytes() == p, o
        covered[o:o + len(p)] = True
    assert (out[~covered] == 0xc3).all()


def test_records_straddling_odd_members_unpack_in_place(engine):
    """A record stream behind a 3-byte 'header', cut into odd members, kept, and unpacked from base 3."""
    recs = UC.shapes()
    stream, off = UC.stream_of(recs)
    whole = b"hdr" + stream
    parts = _cut(whole, [1, 17, 4093, 1500])
    comp, coff, clen, uoff, ulen, _ = _layout(parts, lambda j: 0)
    out = np.zeros(len(whole), np.uint8)
    bad, ok, rid = keep(engine, comp, coff, clen, uoff, ulen, out, len(whole))
    assert bad == 0 and rid > 0 and out.tobytes() == whole
    z = np.zeros(len(off), np.int32)
    rf = np.array([r.fields["rflags"] for r in recs], np.uint8)
    try:
        dev, ml = engine.unpack_resident(rid, 3, len(stream), off, z, z, z, rf)
        assert count(engine) == 1, "the call does not free the stream"
    finally:
        assert engine.lib.cc_resident_free(engine.h, rid) == 0
    host, ml2 = engine.unpack_raw(np.frombuffer(stream, np.uint8), off, z, z, z, rf)
    try:
        assert ml == ml2 == max(r.fields["lseq"] for r in recs)
        assert_same_tables(engine, dev, host)
        assert engine.table_column(dev, "rdig", np.uint64).tolist() == [r.rdig for r in recs]
    finally:
        engine.free_table(dev)
        engine.free_table(host)


# ---------------------------------------------------------------- refused members
@pytest.mark.parametrize("which", [0, 3])
def test_a_refused_member_is_patched(engine, which):
    name, bad_stream, bad_len = IC.handmade_corrupt()[which]
    good = [IC.text(3000, 61), IC.bam_stream()[:20000], IC.random_bytes(777, 62), IC.text(50000, 63)]
    plan = [(IC.raw_deflate(g, 6), len(g), g) for g in good]
    plan.insert(2, (bad_stream, bad_len, None))
    comp, coff, clen, uoff, ulen = bytearray(), [], [], [], []
    at = 0
    for s, n, _ in plan:
        coff.append(len(comp))
        clen.append(len(s))
        comp += s
        uoff.append(at)
        ulen.append(n)
        at += n
    out = np.full(at, 0x5a, np.uint8)
    bad, ok, rid = keep(engine, bytes(comp), coff, clen, uoff, ulen, out, at)
    assert bad == 1 and ok.tolist() == [1, 1, 0, 1, 1], name
    try:
        res = fetch(engine, rid)
        for (s, n, want), o in zip(plan, uoff):
            if want is not None:
                assert res[o:o + n] == want and out[o:o + n].tobytes() == want
        assert (out[uoff[2]:uoff[2] + bad_len] == 0x5a).all(), "a refused member's bytes are not copied to out"
        fill = np.arange(bad_len, dtype=np.uint8) + 1
        assert engine.lib.cc_resident_patch(engine.h, rid, uoff[2], N.ptr(fill), bad_len) == 0
        res = fetch(engine, rid)
        assert res[uoff[2]:uoff[2] + bad_len] == fill.tobytes()
        assert res[:uoff[2]] == good[0] + good[1] and res[uoff[3]:] == good[2] + good[3], "the patch wrote only its range"
    finally:
        assert engine.lib.cc_resident_free(engine.h, rid) == 0


def test_a_member_with_another_crc_is_patched_through_libccio(engine, tmp_path):
    """The CRC32 field of one member flipped: the host path does not check it, the hooked open does,
    inflates the member with the host codec and patches the resident stream."""
    from consensuscruncher_amd.engine import Bam, Interner
    good = UC.write_bam(str(tmp_path / "good.bam"), UC.many(900, 31))
    raw = bytearray(open(good, "rb").read())
    sizes, off = [], 0
    while off < len(raw):
        sizes.append(struct.unpack_from("<H", raw, off + 16)[0] + 1)
        off += sizes[-1]
    assert len(sizes) >= 4, "several members"
    at = sizes[0] + sizes[1]          # the second member's end
    raw[at - 8] ^= 0xff               # its CRC32 field
    inflated_before = sum(struct.unpack_from("<I", raw, o - 4)[0] for o in (sizes[0],))
    path = str(tmp_path / "crc.bam")
    open(path, "wb").write(bytes(raw))
    hb = Bam(path)                    # the open succeeds on the host path
    want = hb.pack(np.arange(hb.n)).tobytes()
    rec, host = host_table(engine, hb, Interner())
    with switched(engine):
        bam = Bam(path)
        _, rid, base = bam.resident()
        res = fetch(engine, rid)
        assert res[base:] == want, "the resident records are the host's, the patched member's included"
        n1 = struct.unpack_from("<I", raw, at - 4)[0]
        member = zlib.decompress(bytes(raw[sizes[0] + 18:at - 8]), -15)
        assert len(member) == n1 and res[inflated_before:inflated_before + n1] == member
        drec, dev = engine.unpack(bam, Interner(), 0)
    try:
        assert_same_tables(engine, dev, host, rec)
    finally:
        engine.free_table(dev)
        engine.free_table(host)
    assert count(engine) == 0


# ---------------------------------------------------------------- argument refusals
def _small(engine):
    """A good keep call: (rid, stream, off, rflags) of 40 records kept behind no header."""
    recs = UC.many(40, 9)
    stream, off = UC.stream_of(recs)
    s = IC.raw_deflate(stream, 6)
    out = np.zeros(len(stream), np.uint8)
    bad, ok, rid = keep(engine, s, [0], [len(s)], [0], [len(stream)], out, len(stream))
    assert bad == 0 and rid > 0 and out.tobytes() == stream
    return rid, stream, off


def _unpack(engine, rid, base, nbytes, off, lib=None, h=None):
    z = np.zeros(max(len(off), 1), np.int32)
    ml, tid = C.c_int32(), C.c_int32(-1)
    rc = (lib or engine.lib).cc_table_unpack_resident(h or engine.h, rid, base, nbytes, N.ptr(off), len(off), N.ptr(z),
                                                      N.ptr(z), N.ptr(z), N.ptr(np.zeros(max(len(off), 1), np.uint8)),
                                                      C.byref(ml), C.byref(tid))
    return rc, tid.value


def _good_call(engine):
    rid, stream, off = _small(engine)
    rc, t = _unpack(engine, rid, 0, len(stream), off)
    assert rc == 0
    engine.lib.cc_table_free(engine.h, t)
    assert engine.lib.cc_resident_free(engine.h, rid) == 0


def test_bad_arguments_are_refused_without_a_fault(engine):
    from consensuscruncher_amd.engine import Engine
    a, b = IC.text(3000, 81), IC.text(2000, 82)
    sa, sb = IC.raw_deflate(a, 6), IC.raw_deflate(b, 6)
    comp, coff, clen = sa + sb, [0, len(sa)], [len(sa), len(sb)]
    out = np.full(6000, 0xc3, np.uint8)
    before = count(engine)
    for name, uoff, total in (("member overruns total", [0, 3000], 4999), ("member starts past total", [0, 5001], 5000),
                              ("members overlap", [0, 2999], 6000), ("members overlap, out of order", [1999, 0], 6000)):
        bad, ok, rid = keep(engine, comp, coff, clen, uoff, [3000, 2000], out, total)
        assert bad == CC_E_INVALID and rid == 0, name
        assert (out == 0xc3).all() and count(engine) == before, name
        _good_call(engine)
    rid, stream, off = _small(engine)
    for base, nbytes in ((0, len(stream) + 1), (1, len(stream)), (len(stream) + 1, 0), ((1 << 64) - 1, 2)):
        rc, _ = _unpack(engine, rid, base, nbytes, off)
        assert rc == CC_E_INVALID, (base, nbytes)
        _good_call(engine)
    fill = np.zeros(16, np.uint8)
    assert engine.lib.cc_resident_patch(engine.h, rid, len(stream) - 15, N.ptr(fill), 16) == CC_E_INVALID
    assert fetch(engine, rid) == stream
    # another context's id
    other = Engine(0)
    try:
        assert other.lib.cc_resident_free(other.h, rid) == CC_E_INVALID
        assert _unpack(engine, rid, 0, len(stream), off, h=other.h)[0] == CC_E_INVALID
        assert other.lib.cc_resident_patch(other.h, rid, 0, N.ptr(fill), 16) == CC_E_INVALID
        assert int(other.lib.cc_resident_fetch(other.h, rid, None, 0)) == CC_E_INVALID
        assert count(other) == 0
    finally:
        other.close()
    assert fetch(engine, rid) == stream, "the owner's stream is untouched"
    # freed twice, used after the free
    assert engine.lib.cc_resident_free(engine.h, rid) == 0
    assert engine.lib.cc_resident_free(engine.h, rid) == CC_E_INVALID
    assert _unpack(engine, rid, 0, len(stream), off)[0] == CC_E_INVALID
    assert engine.lib.cc_resident_patch(engine.h, rid, 0, N.ptr(fill), 16) == CC_E_INVALID
    assert int(engine.lib.cc_resident_fetch(engine.h, rid, None, 0)) == CC_E_INVALID
    assert engine.lib.cc_resident_free(engine.h, 0) == CC_E_INVALID
    _good_call(engine)
    assert count(engine) == before


def test_unpack_falls_back_when_the_id_is_unknown(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam, Interner
    path = UC.write_bam(str(tmp_path / "f.bam"), UC.many(130, 77))
    rec, host = host_table(engine, Bam(path), Interner())
    with switched(engine):
        bam = Bam(path)
        _, rid, _ = bam.resident()
        assert engine.lib.cc_resident_free(engine.h, rid) == 0   # behind the wrapper's back
        engine.set_profiling(True)
        try:
            drec, dev = engine.unpack(bam, Interner(), 0)
            assert uploads(engine) >= 1, "the host stream was uploaded instead"
        finally:
            engine.set_profiling(False)
    try:
        assert_same_tables(engine, dev, host, rec)
    finally:
        engine.free_table(dev)
        engine.free_table(host)


# ---------------------------------------------------------------- fallbacks
def test_regions_and_combined_handles_take_the_upload(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam, Interner
    p = str(tmp_path / "input.bam")
    Bam(os.path.join(GOLDEN, "basic", "input.bam")).write(p, level=6, index=True)

    def tables(make):
        b = make()
        rec, host = host_table(engine, b, Interner())
        return b, rec, host

    for make in (lambda: Bam.open_regions(p, [0, 0], [20000, 100000], [60000, 150000]),
                 lambda: Bam.combine([Bam(p), Bam(p)])):
        _, rec, host = tables(make)
        assert rec.n > 0
        with switched(engine):
            b = make()
            assert b.resident() is None
            drec, dev = engine.unpack(b, Interner(), 0)
            del b
        try:
            assert_same_tables(engine, dev, host, rec)
        finally:
            engine.free_table(dev)
            engine.free_table(host)
        import gc
        gc.collect()   # (the combined parts' wrappers close, and free what their opens kept)
        assert count(engine) == 0


def test_switch_needs_the_inflater_and_the_decoder(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam, Interner
    path = UC.write_bam(str(tmp_path / "s.bam"), UC.many(257, 5))
    rec, host = host_table(engine, Bam(path), Interner())
    for inflate, decode in ((False, True), (True, False), (False, False)):
        with switched(engine, inflate=inflate, decode=decode):
            bam = Bam(path)
            assert bam.resident() is None and count(engine) == 0, (inflate, decode)
            drec, dev = engine.unpack(bam, Interner(), 0)
        try:
            assert_same_tables(engine, dev, host, rec)
        finally:
            engine.free_table(dev)
    engine.free_table(host)
    assert not engine.resident_device and not engine.inflate_device and not engine.decode_device


def test_an_unconsumed_handle_frees_its_stream_on_close(engine, tmp_path, monkeypatch):
    from consensuscruncher_amd.engine import Bam, Engine
    path = UC.write_bam(str(tmp_path / "c.bam"), UC.many(64, 3))
    with switched(engine):
        a, b = Bam(path), Bam(path)
        assert count(engine) == 2 and a.resident()[1] != b.resident()[1]
        a.close()
        assert count(engine) == 1
        b.close()
        assert count(engine) == 0
        b.close()
    # the environment switch, and an engine that closes before the handle: cc_destroy frees the stream
    for k in ("CC_RESIDENT_DEVICE", "CC_INFLATE_DEVICE", "CC_DECODE_DEVICE"):
        monkeypatch.setenv(k, "1")
    other = Engine(0)
    for k in ("CC_RESIDENT_DEVICE", "CC_INFLATE_DEVICE", "CC_DECODE_DEVICE"):
        monkeypatch.delenv(k)
    try:
        assert other.resident_device and other.inflate_device and other.decode_device
        c = Bam(path)
        assert c.resident()[0] is other and count(other) == 1 and count(engine) == 0
    finally:
        other.close()
    assert c.resident() is None
    c.close()
    assert Bam(path).resident() is None, "the closed engine's hooks are unset"


# ---------------------------------------------------------------- pipeline
def _pipeline(engine, tmp, case, **opts):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, case)
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    if kw.get("bedfile", "False") != "False":
        kw["bedfile"] = os.path.join(d, kw["bedfile"])
    os.makedirs(tmp)
    shutil.copy(os.path.join(d, "input.bam"), os.path.join(tmp, "sample.bam"))
    kw["level"] = 1
    kw.update(opts)
    return consensus_pipeline(os.path.join(tmp, "sample.bam"), tmp, engine=engine, **kw)


@pytest.mark.parametrize("case", ["basic", "hg19_bed"])
def test_pipeline_outputs_are_byte_identical(engine, tmp_path, case):
    import gc
    engine.set_profiling(True)
    dev = _pipeline(engine, str(tmp_path / "device"), case, inflate="device", decode="device", resident="device")
    times = engine.kernel_times()
    engine.set_profiling(False)
    assert not engine.resident_device and not engine.inflate_device and not engine.decode_device
    assert "k_unpack_copy" in times and "bgzf_inflate" in times
    assert times.get(UPLOAD, (0.0, 0))[1] < times["k_unpack_sizes"][1], "no table was unpacked from a resident stream"
    gc.collect()
    assert count(engine) == 0, "no stream outlives the run"
    host = _pipeline(engine, str(tmp_path / "host"), case)
    for k in OUTPUTS + ("stats", "read_families"):
        assert open(dev[k], "rb").read() == open(host[k], "rb").read(), k
    seen = 0
    hroot, droot = str(tmp_path / "host"), str(tmp_path / "device")
    for base, _, files in os.walk(hroot):
        for f in files:
            if f.endswith((".bam", ".bai", "stats.txt", "read_families.txt")):
                rel = os.path.relpath(os.path.join(base, f), hroot)
                assert open(os.path.join(droot, rel), "rb").read() == open(os.path.join(hroot, rel), "rb").read(), rel
                seen += 1
    assert seen >= 12
    with pytest.raises(ValueError):
        _pipeline(engine, str(tmp_path / "gpu"), case, resident="gpu")
