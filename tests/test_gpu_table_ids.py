"""The device interner (cc_table_ids, cc_table_ids_resident; Engine.device_ids) against libccio's string
pass.  Engine.table_ids + ccio_intern_first must give ccio_bam_decode_ids' three id columns and rflags
exactly, for a fresh interner and a filled one, and Engine.unpack with device_ids on must build the
table the host decoder uploads (test_gpu_unpack.py's assert_same_tables contract, restated here).
The records are tests/ids_cases.py's: the smallest shapes at which the kernels can still go wrong."""
import json
import os
import shutil

import numpy as np
import pytest

import ids_cases as IC
import unpack_cases as UC
from consensuscruncher_amd import native as N
from parity import GOLDEN

pytestmark = pytest.mark.gpu

SCAN_TILE = 4096    # cc_engine.hip: SCAN_T * SCAN_I
RS_TILE = 4096      # cc_engine.hip: RS_T * RS_I, sort_pairs' tile
BASE = (("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("tlen", np.int32),
        ("flag", np.uint16), ("mapq", np.uint8), ("cigar_id", np.int32), ("qlen", np.int32), ("lseq", np.int32),
        ("bc_id", np.int32), ("rg_id", np.int32), ("rflags", np.uint8), ("qn_off", np.uint64), ("qn_len", np.uint16),
        ("pay_off", np.uint64), ("rdig", np.uint64))
DERIVED = (("rkey", np.uint64), ("meta", np.uint32), ("core", np.int32), ("qn_ol", np.uint64), ("qdig", np.uint64),
           ("rdeep", np.uint8))
OUTPUTS = ("sscs", "singleton", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction", "uncorrected",
           "dcs_sc", "all_unique")


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_tile_sizes_are_the_engines():
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "cc_engine.hip")).read()
    assert "SCAN_T = 256, SCAN_I = 16, SCAN_TILE = SCAN_T * SCAN_I" in src
    assert "RS_T = 256, RS_I = 16, RS_TILE = RS_T * RS_I" in src


def check_ids(engine, path, mode=0, delim="|", filled=None, resident=False):
    """table_ids + intern_first against decode_ids on the file at path; returns (records, first)."""
    from consensuscruncher_amd.engine import Bam, Interner
    it_h, it_d = Interner(), Interner()
    for it in (it_h, it_d):
        if filled:
            b = Bam(filled)
            b.decode_ids(it, mode, delim)
            b.close()
    bh, bd = Bam(path), Bam(path)
    want, _, _ = bh.decode_ids(it_h, mode, delim)
    cols, stream, off = bd.decode_cols()
    if resident:
        lead = np.zeros(resident, np.uint8)   # the records start at an odd base
        rid = engine.resident_put(np.concatenate([lead, stream]))
        try:
            local, rflags, first = engine.table_ids_resident(rid, resident, stream.size, off, mode, delim)
        finally:
            engine.lib.cc_resident_free(engine.h, rid)
    else:
        local, rflags, first = engine.table_ids(stream, off, mode, delim)
    n = want.n
    for k in range(3):
        assert local[k].shape == (n,) and (local[k] < len(first[k])).all()
        # local ids are ranks in order of first occurrence: the first records ascend, and each is its id's first
        assert (np.diff(first[k]) > 0).all(), k
        assert np.array_equal(local[k][first[k]], np.arange(len(first[k]))), k
    bc, cig, rg = bd.intern_first(it_d, mode, delim, local, first)
    assert np.array_equal(bc, want.bc_id[:n]), "bc_id"
    assert np.array_equal(cig, want.cigar_id[:n]), "cigar_id"
    assert np.array_equal(rg, want.rg_id[:n]), "rg_id"
    assert np.array_equal(rflags, want.rflags[:n]), "rflags"
    for k in range(3):
        assert it_d.blob(k)[0].tobytes() == it_h.blob(k)[0].tobytes() and it_d.size(k) == it_h.size(k)
    bh.close()
    bd.close()
    return want, first


def host_table(engine, bam, it, mode=0, delim="|"):
    import ctypes as C
    from consensuscruncher_amd.engine import Records
    qn, pay, ml = C.c_uint64(), C.c_uint64(), C.c_int32()
    N.io().ccio_bam_layout(bam.h, C.byref(qn), C.byref(pay), C.byref(ml), 0)
    rec = Records(bam.n, qn.value, pay.value, ml.value, nref=len(bam.refs), derived=False)
    assert N.io().ccio_bam_decode(bam.h, it.h, mode, delim.encode(), C.byref(rec.struct), 0) == 0
    return rec, engine.upload(rec)


def check_table(engine, path, mode=0, delim="|"):
    """Engine.unpack with device_ids on against the host decoder's uploaded table."""
    from consensuscruncher_amd.engine import Bam, Interner
    bam = Bam(path)
    it_h, it_d = Interner(), Interner()
    rec, host = host_table(engine, bam, it_h, mode, delim)
    was = engine.device_ids(True)
    try:
        drec, dev = engine.unpack(bam, it_d, mode, delim)
    finally:
        engine.device_ids(was)
    try:
        n = rec.n
        assert drec.n == n and drec.max_len == rec.max_len
        for name, dt in BASE:
            a, b = engine.table_column(dev, name, dt), engine.table_column(host, name, dt)
            assert a.shape == b.shape and np.array_equal(a, b), name
            assert np.array_equal(b, getattr(rec, name)[:n]), name
        for name in ("qn_blob", "payload"):
            a, b = engine.table_column(dev, name, np.uint8), engine.table_column(host, name, np.uint8)
            assert a.tobytes() == b.tobytes() == getattr(rec, name).tobytes(), name
        for name, dt in DERIVED:
            assert np.array_equal(engine.table_column(dev, name, dt), engine.table_column(host, name, dt)), name
        a, b = engine.table_column(dev, "dlist", np.int32), engine.table_column(host, "dlist", np.int32)
        assert np.array_equal(np.sort(a), np.sort(b)), "dlist"
        for name in ("cigar_id", "bc_id", "rg_id", "rflags"):
            assert np.array_equal(getattr(drec, name)[:n], getattr(rec, name)[:n]), name
    finally:
        engine.free_table(host)
        engine.free_table(dev)
        bam.close()
    return rec


def _ran_on_device(engine, fn):
    """fn() with profiling on: whether the interner's kernels ran in it"""
    engine.set_profiling(True)
    try:
        fn()
        return "ids_keys" in engine.kernel_times()
    finally:
        engine.set_profiling(False)


COUNTS = sorted({0, 1, 63, 64, 65, 255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, RS_TILE - 1, RS_TILE,
                 RS_TILE + 1, 2 * RS_TILE + 1})


@pytest.mark.parametrize("n", COUNTS)
def test_record_counts_at_launch_scan_and_sort_tile_edges(engine, tmp_path, n):
    recs = IC.keyed(n, lambda i: (i * 37) % 61 if i % 5 else i % 3)
    path = UC.write_bam(str(tmp_path / "n.bam"), recs)
    check_ids(engine, path)
    if n in (0, 1, 257, SCAN_TILE + 1):
        assert _ran_on_device(engine, lambda: check_table(engine, path)) == (n > 0)


PATTERNS = {
    "one_key": lambda n: (lambda i: 5),
    "all_distinct": lambda n: (lambda i: i),
    "first_occurrence_is_the_last_record": lambda n: (lambda i: 9999 if i == n - 1 else i % 7),
    "record_0_and_the_last_tile_only": lambda n: (lambda i: 0 if i in (0, n - 3) else 1 + i % 50),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_key_patterns(engine, tmp_path, pattern):
    n = 2 * RS_TILE + 77
    recs = IC.keyed(n, PATTERNS[pattern](n), pad=0)
    want, first = check_ids(engine, UC.write_bam(str(tmp_path / "p.bam"), recs))
    counts = {"one_key": 1, "all_distinct": n, "first_occurrence_is_the_last_record": 8,
              "record_0_and_the_last_tile_only": 51}
    assert [len(f) for f in first] == [counts[pattern]] * 3
    if pattern == "first_occurrence_is_the_last_record":
        assert first[0][-1] == n - 1 and want.bc_id[n - 1] == 7
    if pattern == "record_0_and_the_last_tile_only":
        assert want.bc_id[n - 3] == 0 and n - 3 >= 2 * RS_TILE


def test_a_filled_interner_keeps_its_ids(engine, tmp_path):
    a = UC.write_bam(str(tmp_path / "a.bam"), IC.keyed(300, lambda i: (i * 7) % 40))
    b = UC.write_bam(str(tmp_path / "b.bam"), IC.keyed(700, lambda i: 20 + (i * 11) % 40 if i % 3 else 0))
    want, _ = check_ids(engine, b, filled=a)
    assert want.bc_id[:want.n].max() >= 40 and (want.bc_id[:want.n] < 40).any()


def test_cigar_forms(engine, tmp_path):
    recs = IC.cigar_records() * 3
    path = UC.write_bam(str(tmp_path / "c.bam"), recs)
    want, first = check_ids(engine, path)
    ids = want.cigar_id[:want.n]
    at = {c: i for i, c in enumerate(IC.CIGARS)}
    assert len(first[1]) == len(IC.CIGARS), "every raw cigar is a key of its own"
    assert ids[at[((0, 10),)]] == ids[at[((10, 10),)]] == ids[at[((15, 10),)]], "op 10 and 15 print as M: one shared id"
    assert ids[at[((0, 10), (4, 2))]] == ids[at[((12, 10), (4, 2))]] != ids[at[((0, 10),)]]
    assert len(set(ids.tolist())) == len(IC.CIGARS) - 3
    check_table(engine, path)
    check_table(engine, path, mode=1)


@pytest.mark.parametrize("delim", ["|", "||", "#+#", IC.DELIM16.decode(), "abc"])
def test_barcode_mode_0(engine, tmp_path, delim):
    recs = [IC.rec(n, aux=b"RGZg\x00", i=i) for i, (n, _) in enumerate(IC.BARCODE_MODE0)] * 2
    path = UC.write_bam(str(tmp_path / "b0.bam"), recs)
    want, _ = check_ids(engine, path, 0, delim)
    exp, rf, _ = IC.expected_ids(recs, 0, delim.encode())
    assert np.array_equal(exp[0], want.bc_id[:want.n]) and np.array_equal(rf, want.rflags[:want.n])
    assert (want.rflags[:want.n] & 1).any() and (want.bc_id[:want.n] >= 0).any() or delim == "abc"
    assert _ran_on_device(engine, lambda: check_table(engine, path, 0, delim))


def test_a_17_byte_delimiter_is_unsupported_and_falls_back(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam
    d17 = "x" + IC.DELIM16.decode()
    recs = [IC.rec(b"r" + d17.encode() + b"AC.GT", i=0), IC.rec(b"r|AC.GT", i=1)] + IC.name_records(0)
    path = UC.write_bam(str(tmp_path / "d17.bam"), recs)
    bam = Bam(path)
    _, stream, off = bam.decode_cols()
    launches = N.amd().cc_launch_count()
    with pytest.raises(N.CCError) as ei:
        engine.table_ids(stream, off, 0, d17)
    assert ei.value.code == N.CC_E_UNSUPPORTED and N.amd().cc_launch_count() == launches, "before any launch"
    bam.close()
    assert not _ran_on_device(engine, lambda: check_table(engine, path, 0, d17))


def test_barcode_mode_1(engine, tmp_path):
    recs = IC.name_records(1) * 2
    assert {len(n) for n in IC.BARCODE_MODE1} >= {1, 254}
    path = UC.write_bam(str(tmp_path / "b1.bam"), recs)
    want, _ = check_ids(engine, path, 1)
    exp, _, _ = IC.expected_ids(recs, 1, b"|")
    assert np.array_equal(exp[0], want.bc_id[:want.n])
    check_table(engine, path, 1)


def test_rg_forms(engine, tmp_path):
    recs = IC.aux_records() * 2 + UC.shapes()
    path = UC.write_bam(str(tmp_path / "rg.bam"), recs)
    for mode in (0, 1):
        want, _ = check_ids(engine, path, mode)
        exp, rf, _ = IC.expected_ids(recs, mode, b"|")
        assert np.array_equal(exp[2], want.rg_id[:want.n]) and np.array_equal(rf, want.rflags[:want.n])
    names = list(IC.RG_FORMS)
    rg, fl = want.rg_id[:want.n], want.rflags[:want.n] & 4
    for name, has, flag in (("Z", 1, 0), ("A", 1, 0), ("H", 0, 4), ("i", 0, 4), ("B_then_Z", 0, 4), ("after_every_type", 1, 0),
                            ("Z_no_nul", 1, 0), ("none", 0, 0), ("unknown_before_rg", 0, 4)):
        i = names.index(name)
        assert (rg[i] >= 0) == bool(has) and fl[i] == flag, name
    assert rg[names.index("Z")] == rg[names.index("grp1_again")] == rg[names.index("second_rg_ignored")]
    assert _ran_on_device(engine, lambda: check_table(engine, path))


@pytest.mark.parametrize("form", sorted(IC.RG_MALFORMED))
def test_malformed_aux_is_refused_and_unpack_falls_back(engine, tmp_path, form):
    from consensuscruncher_amd.engine import Bam
    k = 70
    recs = IC.keyed(130, lambda i: i % 9)
    recs[k] = IC.rec(b"q|AC.GT", aux=IC.RG_MALFORMED[form], i=k)
    recs[k + 20] = IC.rec(b"q|AC.GT", aux=IC.RG_MALFORMED[form], i=k + 20)
    path = UC.write_bam(str(tmp_path / "bad.bam"), recs)
    bam = Bam(path)
    _, stream, off = bam.decode_cols()
    tables, res = dict(engine.tables), engine.lib.cc_resident_count(engine.h)
    with pytest.raises(N.CCError) as ei:
        engine.table_ids(stream, off, 0, "|")
    assert ei.value.code == N.CC_E_INVALID and "record %d:" % k in str(ei.value), str(ei.value)
    bam.close()
    # the host pass decides the file (its walk stays inside the file's buffer on these forms), and the
    # next good file on the same engine runs on the device again
    check_table(engine, path)
    assert engine.tables == tables and engine.lib.cc_resident_count(engine.h) == res
    good = UC.write_bam(str(tmp_path / "good.bam"), IC.keyed(130, lambda i: i % 9))
    assert _ran_on_device(engine, lambda: check_table(engine, good))


def test_record_starts_on_every_alignment_and_the_resident_form(engine, tmp_path):
    recs = IC.aux_records() + IC.name_records(0) + UC.shapes()
    _, off = UC.stream_of(recs)
    assert {int(o) % 16 for o in off} == set(range(16))
    path = UC.write_bam(str(tmp_path / "al.bam"), recs)
    check_ids(engine, path)
    before = engine.lib.cc_resident_count(engine.h)
    for base in (1, 7, 13):
        check_ids(engine, path, resident=base)
    check_ids(engine, path, mode=1, resident=3)
    assert engine.lib.cc_resident_count(engine.h) == before
    with pytest.raises(N.CCError) as ei:
        engine.table_ids_resident(1 << 40, 0, 10, off, 0, "|")
    assert ei.value.code == N.CC_E_INVALID


def test_collisions_fall_back_and_leak_nothing(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam
    recs = IC.keyed(200, lambda i: i % 40)
    path = UC.write_bam(str(tmp_path / "col.bam"), recs)
    tables, res = dict(engine.tables), engine.lib.cc_resident_count(engine.h)
    engine.debug_ids_hash_bits(4)
    try:
        bam = Bam(path)
        _, stream, off = bam.decode_cols()
        with pytest.raises(N.CCError) as ei:
            engine.table_ids(stream, off, 0, "|")
        assert ei.value.code == N.CC_E_COLLISION
        bam.close()
        engine.set_profiling(True)
        check_table(engine, path)           # the host pass decides the file: the same table
        times = engine.kernel_times()
        engine.set_profiling(False)
        assert "ids_keys" in times and "ids_assign" in times, "the device path ran and gave up"
    finally:
        engine.debug_ids_hash_bits(64)
    assert engine.tables == tables and engine.lib.cc_resident_count(engine.h) == res
    check_ids(engine, path)
    assert _ran_on_device(engine, lambda: check_table(engine, path))
    assert engine.tables == tables and engine.lib.cc_resident_count(engine.h) == res
    with pytest.raises(N.CCError):
        engine.debug_ids_hash_bits(0)


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


def test_switch_plumbing_and_identical_pipeline_outputs(engine, tmp_path, monkeypatch):
    from consensuscruncher_amd.engine import Engine
    monkeypatch.setenv("CC_IDS_DEVICE", "1")
    first = Engine(0)
    try:
        assert first.ids_device and not first.decode_device
        monkeypatch.delenv("CC_IDS_DEVICE")
        assert first.device_ids(False) is True and not first.ids_device
    finally:
        first.close()
    assert not engine.ids_device
    assert engine.device_ids(True) is False and engine.device_ids(False) is True
    host = _pipeline(engine, str(tmp_path / "host"), "basic", inflate="host", decode="host", resident="host", ids="host")
    # ids="device" without decode="device" changes nothing: no interner kernel runs
    engine.set_profiling(True)
    alone = _pipeline(engine, str(tmp_path / "alone"), "basic", ids="device")
    assert not any(k.startswith("ids_") for k in engine.kernel_times())
    engine.set_profiling(True)
    dev = _pipeline(engine, str(tmp_path / "device"), "basic", inflate="device", decode="device", resident="device",
                    ids="device")
    times = engine.kernel_times()
    engine.set_profiling(False)
    assert not engine.ids_device and not engine.decode_device, "the options are wired for the call only"
    assert "ids_keys" in times and "ids_sort" in times and "ids_download" in times
    for k in OUTPUTS + ("stats", "read_families"):
        assert open(dev[k], "rb").read() == open(host[k], "rb").read() == open(alone[k], "rb").read(), k
    with pytest.raises(ValueError):
        _pipeline(engine, str(tmp_path / "gpu"), "basic", ids="gpu")
