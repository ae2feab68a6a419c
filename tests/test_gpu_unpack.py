"""The device record unpacker (cc_table_unpack: k_unpack_sizes, the slot-size scans, k_unpack_copy,
k_derive) against the host decoder.  Engine.unpack of a BAM must give the table that Bam.decode +
Engine.upload (device-derived) give: every base column, both blobs whole (every padding byte and the
tails) and every derived column, byte for byte (dlist sorted: its order is free).

The shapes are tests/unpack_cases.py's: l_seq at every slot-size step, the odd nibble tail and past
one pass of the copy kernel's 16-lane group; l_read_name 1..255; record starts on every alignment mod
16; no cigar and every cigar op; qual[0] == 0xff; the aux forms; tid -1; an unsorted table; a deep
position group; n at the launch and scan-tile edges.  Bad inputs are bad data handed to the
unchanged kernels: each must be refused with CC_E_INVALID (l_seq = 65536: CC_E_UNSUPPORTED), leave no
table, and the next good unpack on the same engine must still match."""
import json
import os
import shutil
import struct

import numpy as np
import pytest

import unpack_cases as UC
import vote_cases as VC
from consensuscruncher_amd import native as N
from parity import GOLDEN

pytestmark = pytest.mark.gpu

CC_E_INVALID, CC_E_UNSUPPORTED = -1, -11
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


def host_table(engine, bam, it, mode=0, delim="|"):
    """Bam.decode without the decoder's layout, uploaded: the derived columns are k_derive's."""
    import ctypes as C
    from consensuscruncher_amd.engine import Records
    qn, pay, ml = C.c_uint64(), C.c_uint64(), C.c_int32()
    N.io().ccio_bam_layout(bam.h, C.byref(qn), C.byref(pay), C.byref(ml), 0)
    rec = Records(bam.n, qn.value, pay.value, ml.value, nref=len(bam.refs), derived=False)
    assert N.io().ccio_bam_decode(bam.h, it.h, mode, delim.encode(), C.byref(rec.struct), 0) == 0
    return rec, engine.upload(rec)


def assert_same_tables(engine, dev, host, rec):
    """table `dev` (unpacked) against table `host` (uploaded from rec), and against rec's own arrays"""
    n = rec.n
    for name, dt in BASE:
        a, b = engine.table_column(dev, name, dt), engine.table_column(host, name, dt)
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert np.array_equal(b, getattr(rec, name)[:n]), name
    for name in BLOBS:
        a, b = engine.table_column(dev, name, np.uint8), engine.table_column(host, name, np.uint8)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), name
        assert a.tobytes() == getattr(rec, name).tobytes(), name      # the whole buffer, its tail included
    from consensuscruncher_amd.engine import coord_sorted
    for name, dt in DERIVED:
        # (ext is each tid's position at the end of its run: on an unsorted table a tid has several runs
        # and k_derive's threads race for the word, in both tables alike; the engine reads it on sorted
        # tables only)
        if name == "ext" and not coord_sorted(rec):
            continue
        a, b = engine.table_column(dev, name, dt), engine.table_column(host, name, dt)
        assert a.shape == b.shape and np.array_equal(a, b), name
    a, b = engine.table_column(dev, "dlist", np.int32), engine.table_column(host, "dlist", np.int32)
    assert np.array_equal(np.sort(a), np.sort(b)), "dlist"
    return len(a)


def both(engine, path, mode=0, delim="|"):
    from consensuscruncher_amd.engine import Bam, Interner
    bam = Bam(path)
    it_h, it_d = Interner(), Interner()
    rec, host = host_table(engine, bam, it_h, mode, delim)
    drec, dev = engine.unpack(bam, it_d, mode, delim)
    assert drec.n == rec.n and drec.max_len == rec.max_len
    return bam, rec, host, drec, dev


def check_bam(engine, path, mode=0, delim="|"):
    bam, rec, host, drec, dev = both(engine, path, mode, delim)
    try:
        return assert_same_tables(engine, dev, host, rec), rec
    finally:
        engine.free_table(host)
        engine.free_table(dev)


def test_shapes_match_the_host_decoder(engine, tmp_path):
    recs = UC.shapes()
    _, off = UC.stream_of(recs)
    assert {int(o) % 16 for o in off} == set(range(16))
    assert {r.fields["lseq"] for r in recs} >= set(UC.LSEQS) and {r.fields["l_read_name"] for r in recs} >= set(UC.LQNS)
    _, rec = check_bam(engine, UC.write_bam(str(tmp_path / "shapes.bam"), recs))
    assert rec.rdig[:rec.n].tolist() == [r.rdig for r in recs]
    assert (rec.tid[:rec.n] == -1).any() and (rec.qlen[:rec.n] == -1).any() and (rec.rflags[:rec.n] & 2).any()
    check_bam(engine, str(tmp_path / "shapes.bam"), mode=1)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_record_counts_at_launch_and_scan_tile_edges(engine, tmp_path, n):
    deep, _ = check_bam(engine, UC.write_bam(str(tmp_path / "n.bam"), UC.many(n, 100 + n, deep_at=True)))
    assert (deep >= 1) == (n >= 255), "a run of 70 equal positions is a deep group"


def test_unsorted_table(engine, tmp_path):
    from consensuscruncher_amd.engine import coord_sorted
    _, rec = check_bam(engine, UC.write_bam(str(tmp_path / "u.bam"), UC.many(700, 5, sort=False)))
    assert not coord_sorted(rec)


def test_golden_inputs(engine):
    for case in ("basic", "c4_skew", "unsorted"):
        check_bam(engine, os.path.join(GOLDEN, case, "input.bam"))


def _good(engine, tmp_path):
    check_bam(engine, UC.write_bam(str(tmp_path / "good.bam"), UC.many(130, 77)))


def _raw(engine, stream, off, n=None):
    n = len(off) if n is None else n
    z = np.zeros(max(n, 1), np.int32)
    return engine.unpack_raw(np.frombuffer(stream, np.uint8), off, z, z, z, np.zeros(max(n, 1), np.uint8))


def test_handmade_bad_inputs_are_refused(engine, tmp_path):
    recs = UC.many(40, 9)
    stream, off = UC.stream_of(recs)
    t, ml = _raw(engine, stream, off)          # the good stream is accepted as it stands
    assert ml == max(r.fields["lseq"] for r in recs)
    engine.free_table(t)
    k = 17

    def patched(at, fmt, v):
        b = bytearray(stream)
        b[int(off[k]) + at:int(off[k]) + at + struct.calcsize(fmt)] = struct.pack(fmt, v)
        return bytes(b)

    past = off.copy()
    past[-1] = len(stream) + 5
    swapped = off.copy()
    swapped[[k, k + 1]] = swapped[[k + 1, k]]
    twice = off.copy()
    twice[k + 1] = twice[k]
    bad = {"offset_past_stream": (stream, past, 39), "offsets_out_of_order": (stream, swapped, k + 1),
           "offset_twice": (stream, twice, k + 1), "bs_below_32": (patched(0, "<i", 31), off, k),
           "bs_past_stream": (patched(0, "<i", len(stream)), off, k),
           "lseq_overruns_bs": (patched(4 + 16, "<i", 4000), off, k),
           "ncigar_overruns_bs": (patched(4 + 12, "<H", 0xffff), off, k),
           "lqn_overruns_bs": (patched(4 + 8, "<B", 255), off, k), "lseq_negative": (patched(4 + 16, "<i", -5), off, k),
           "cut_mid_record": (stream[:int(off[-1]) + 60], off, 39)}
    for name, (s, o, first) in bad.items():
        before = dict(engine.tables)
        with pytest.raises(N.CCError) as ei:
            _raw(engine, s, o)
        assert ei.value.code == CC_E_INVALID, name
        assert "record %d:" % first in str(ei.value), (name, str(ei.value))
        assert engine.tables == before, name
        _good(engine, tmp_path)
    # the host's QUAL_MISSING bit must agree with the record
    with pytest.raises(N.CCError) as ei:
        z = np.zeros(len(off), np.int32)
        rf = np.zeros(len(off), np.uint8)
        rf[3] = 2
        engine.unpack_raw(np.frombuffer(stream, np.uint8), off, z, z, z, rf)
    assert ei.value.code == CC_E_INVALID and "record 3:" in str(ei.value)
    _good(engine, tmp_path)


def test_a_read_of_65536_bases_is_unsupported(engine, tmp_path):
    rng = np.random.default_rng(3)
    recs = [UC.make(rng, 0, 150, 20), UC.make(rng, 1, 65536, 20), UC.make(rng, 2, 150, 20)]
    stream, off = UC.stream_of(recs)
    with pytest.raises(N.CCError) as ei:
        _raw(engine, stream, off)
    assert ei.value.code == CC_E_UNSUPPORTED
    _good(engine, tmp_path)
    recs[1] = UC.make(rng, 1, 65535, 20)       # the longest read the table holds
    check_bam(engine, UC.write_bam(str(tmp_path / "long.bam"), recs))


def test_a_vote_on_an_unpacked_table(engine, tmp_path):
    table, calls = VC.sscs_matrix(150, seed=41, sizes=(1, 2, 3, 7), rounds=1, min_calls=2)
    path = str(tmp_path / "vote.bam")
    table.write(path)
    bam, rec, host, drec, dev = both(engine, path)
    assert rec.n == len(table)
    for cutoff, fams in calls[:2]:
        off = np.concatenate([[0], np.cumsum([len(f) for f in fams])]).astype(np.int64)
        mi = np.concatenate(fams).astype(np.int32)
        a = engine.sscs_vote(host, mi, off, cutoff)
        b = engine.sscs_vote(dev, mi, off, cutoff)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    engine.free_table(host)
    engine.free_table(dev)


def _pipeline(engine, tmp, case, decode=None):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, case)
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    if kw.get("bedfile", "False") != "False":
        kw["bedfile"] = os.path.join(d, kw["bedfile"])
    os.makedirs(tmp)
    shutil.copy(os.path.join(d, "input.bam"), os.path.join(tmp, "sample.bam"))
    kw["level"] = 1
    if decode is not None:
        kw["decode"] = decode
    return consensus_pipeline(os.path.join(tmp, "sample.bam"), tmp, engine=engine, **kw)


def _same_files(hroot, droot):
    seen = 0
    for base, _, files in os.walk(hroot):
        for f in files:
            if f.endswith((".bam", ".bai", "stats.txt", "read_families.txt")):
                rel = os.path.relpath(os.path.join(base, f), hroot)
                assert open(os.path.join(droot, rel), "rb").read() == open(os.path.join(hroot, rel), "rb").read(), rel
                seen += 1
    return seen


@pytest.mark.parametrize("case", ["basic", "hg19_bed", "c4_skew"])
def test_pipeline_outputs_are_byte_identical(engine, tmp_path, case):
    engine.set_profiling(True)
    dev = _pipeline(engine, str(tmp_path / "device"), case, "device")
    times = engine.kernel_times()
    engine.set_profiling(False)
    assert not engine.decode_device, "the option is wired for the call only"
    assert "k_unpack_copy" in times and "k_unpack_sizes" in times, "the unpacker ran, timed under its scope names"
    host = _pipeline(engine, str(tmp_path / "host"), case, "host")
    for k in OUTPUTS + ("stats", "read_families"):
        assert open(dev[k], "rb").read() == open(host[k], "rb").read(), k
    assert _same_files(str(tmp_path / "host"), str(tmp_path / "device")) >= 12
    with pytest.raises(ValueError):
        _pipeline(engine, str(tmp_path / "gpu"), case, "gpu")


def test_option_toggles_and_the_off_path_is_unchanged(engine, tmp_path, monkeypatch):
    from consensuscruncher_amd.engine import Engine
    monkeypatch.setenv("CC_DECODE_DEVICE", "1")
    first = Engine(0)
    try:
        assert first.decode_device
        monkeypatch.delenv("CC_DECODE_DEVICE")
        assert first.device_decode(False) is True and not first.decode_device
    finally:
        first.close()
    assert not engine.decode_device
    assert engine.device_decode(True) is False and engine.decode_device
    engine.set_profiling(True)
    _pipeline(engine, str(tmp_path / "on"), "basic")
    assert "k_unpack_copy" in engine.kernel_times()
    assert engine.device_decode(False) is True
    engine.set_profiling(True)   # (clears the scopes timed so far)
    # off: the default call and the explicit decode="host" enqueue the same device work, none of it new
    lib = N.amd()
    c0 = lib.cc_launch_count()
    _pipeline(engine, str(tmp_path / "off_default"), "basic")
    c1 = lib.cc_launch_count()
    t_off = engine.kernel_times()
    _pipeline(engine, str(tmp_path / "off_host"), "basic", "host")
    c2 = lib.cc_launch_count()
    engine.set_profiling(False)
    assert c1 - c0 == c2 - c1 > 0
    assert not any(k.startswith(("k_unpack", "unpack_scan")) for k in t_off)


def test_sharded_pipeline_outputs_are_byte_identical(engine, tmp_path):
    """The multi-GPU driver (three ranks, one after another on this GPU; combined views, so the slim
    pass packs each rank's records) with decode="device" against the same run with the host decoder."""
    from consensuscruncher_amd.sharded import LocalComm, sharded_pipeline
    d = os.path.join(GOLDEN, "bed_multi")
    bed = os.path.join(d, json.load(open(os.path.join(d, "params.json")))["run"]["bedfile"])
    out = {}
    for decode in ("device", "host"):
        root = str(tmp_path / decode)
        os.makedirs(root)
        shutil.copy(os.path.join(d, "input.bam"), os.path.join(root, "sample.bam"))
        if decode == "device":
            engine.set_profiling(True)
        out[decode] = sharded_pipeline(os.path.join(root, "sample.bam"), root, bed, LocalComm(3), engine, level=1,
                                       decode=decode)
        if decode == "device":
            assert "k_unpack_copy" in engine.kernel_times()
            engine.set_profiling(False)
        assert not engine.decode_device
    for k in OUTPUTS + ("stats", "read_families"):
        assert open(out["device"][k], "rb").read() == open(out["host"][k], "rb").read(), k
    assert _same_files(str(tmp_path / "host"), str(tmp_path / "device")) >= 12
