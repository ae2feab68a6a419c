"""The device formatter for the consensus read names (cc_format_csn_names / cc_format_dcs_names:
k_name_sizes_*, the offsets' scan, k_name_write_*) against libccio's ccio_format_csn_names /
ccio_format_dcs_names, byte for byte, blob and off: through Engine.csn_names / Engine.dcs_names, through
the C calls where a refusal's text or cc_names_read's contract is the point, and through the whole
pipeline with names="device".  The cases (tests/name_cases.py) are the smallest shapes at which the
kernels can go wrong.  The issue's output length 1 cannot be made: the shortest name either rule
produces is the dcs rule's four separators (length 4), which the cases hold instead."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

import name_cases as NC
import unpack_cases as UC
from parity import GOLDEN, assert_same_in_order
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import MODE_DUPLEX, Bam, Engine, Interner, csn_names, dcs_names

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


class Names(object):
    """A dcs case's BAM opened, decoded and uploaded as a record table."""

    def __init__(self, engine, qnames, d, tag="names"):
        self.engine = engine
        self.bam = Bam(NC.Dcs(tag, qnames, [], []).write(d))
        self.it = Interner()
        self.rec, self.table = engine.table(self.bam, self.it, MODE_DUPLEX)

    def close(self):
        self.engine.free_table(self.table)


@pytest.fixture(scope="module")
def loaded(engine, tmp_path_factory):
    ld = Names(engine, NC.QNAMES, tmp_path_factory.mktemp("names"))
    yield ld
    ld.close()


def _same(got, want, what):
    assert (got[1] == want[1]).all(), what + ": off differs"
    n = int(want[1][-1])
    assert got[0][:n].tobytes() == want[0][:n].tobytes(), what + ": the blob differs"


def _c_csn(engine, case, it=None):
    """cc_format_csn_names itself: (rc, off, total)."""
    it = it or case.interner()
    bc, bc_off = it.blob(0)
    cg, cg_off = it.blob(1)
    n = len(case.suf)
    off = np.full(n + 1, -7, np.int64)
    total = C.c_int64(-7)
    rc = engine.lib.cc_format_csn_names(engine.h, n, N.ptr(case.f9), N.ptr(case.suf), N.ptr(bc), N.ptr(bc_off),
                                        len(bc_off) - 1, N.ptr(cg), N.ptr(cg_off), len(cg_off) - 1, N.ptr(off),
                                        C.byref(total))
    return rc, off, int(total.value)


def _c_dcs(engine, table, case):
    n = len(case.rec_tag)
    off = np.full(n + 1, -7, np.int64)
    total = C.c_int64(-7)
    rc = engine.lib.cc_format_dcs_names(engine.h, int(table), n, N.ptr(case.rec_tag), N.ptr(case.rec_ds), N.ptr(off),
                                        C.byref(total))
    return rc, off, int(total.value)


def _read(engine, total, slack=64):
    """cc_names_read into a buffer with sentinel bytes behind total: (rc, the blob); the sentinels must stay."""
    buf = np.full(total + slack, SENTINEL, np.uint8)
    rc = engine.lib.cc_names_read(engine.h, N.ptr(buf), total)
    assert (buf[total:] == SENTINEL).all(), "cc_names_read wrote behind total"
    return rc, buf[:total]


def _err(engine):
    return engine.lib.cc_last_error(engine.h).decode()


@pytest.mark.parametrize("case", NC.csn_cases(), ids=[c.name for c in NC.csn_cases()])
def test_csn_names_equal_the_host_formatter(engine, case):
    it = case.interner()
    want = csn_names(it, case.f9, case.suf)
    before = engine.launch_count()
    _same(engine.csn_names(it, case.f9, case.suf), want, case.name)
    assert engine.launch_count() > before or len(case.suf) == 0, "the kernels did not run"
    # the C call's own outputs, and the blob read into a buffer with sentinels behind it
    rc, off, total = _c_csn(engine, case, it)
    assert rc == 0 and total == want[1][-1] and (off == want[1]).all()
    rc, blob = _read(engine, total)
    assert rc == 0 and blob.tobytes() == want[0][:total].tobytes()


def test_csn_offsets_take_every_residue(engine):
    case = [c for c in NC.csn_cases() if c.name == "residues"][0]
    blob, off = engine.csn_names(case.interner(), case.f9, case.suf)
    assert {int(o) % 16 for o in off[:-1]} == set(range(16)) and (np.diff(off) == 33).all()


@pytest.mark.parametrize("case", NC.dcs_cases(), ids=[c.name for c in NC.dcs_cases()])
def test_dcs_names_equal_the_host_formatter(engine, loaded, case):
    want = dcs_names(loaded.bam, case.rec_tag, case.rec_ds)
    before = engine.launch_count()
    _same(engine.dcs_names(loaded.bam, loaded.table, case.rec_tag, case.rec_ds), want, case.name)
    assert engine.launch_count() > before or len(case.rec_tag) == 0, "the kernels did not run"
    rc, off, total = _c_dcs(engine, loaded.table, case)
    assert rc == 0 and total == want[1][-1] and (off == want[1]).all()
    rc, blob = _read(engine, total)
    assert rc == 0 and blob.tobytes() == want[0][:total].tobytes()


def test_dcs_lengths_and_residues(engine, loaded):
    by = {c.name: c for c in NC.dcs_cases()}
    blob, off = engine.dcs_names(loaded.bam, loaded.table, by["lengths"].rec_tag, by["lengths"].rec_ds)
    assert tuple(np.diff(off)) == NC.LENGTHS
    blob, off = engine.dcs_names(loaded.bam, loaded.table, by["residues"].rec_tag, by["residues"].rec_ds)
    assert {int(o) % 16 for o in off[:-1]} == set(range(16)) and (np.diff(off) == 17).all()
    blob, off = engine.dcs_names(loaded.bam, loaded.table, by["all_pairs"].rec_tag, by["all_pairs"].rec_ds)
    assert {int(o) % 16 for o in off[:-1]} == set(range(16))


def test_dcs_table_from_the_device_unpacker(engine, tmp_path):
    """The table built by the record unpacker (its own qname slots) gives the same names."""
    case = [c for c in NC.dcs_cases() if c.name == "all_pairs"][0]
    was = engine.device_decode(True)
    try:
        ld = Names(engine, NC.QNAMES, tmp_path, "unpacked")
    finally:
        engine.device_decode(was)
    try:
        _same(engine.dcs_names(ld.bam, ld.table, case.rec_tag, case.rec_ds), dcs_names(ld.bam, case.rec_tag, case.rec_ds),
              "unpacked")
    finally:
        ld.close()


@pytest.mark.parametrize("label,case,bad", NC.csn_refusals(), ids=[r[0] for r in NC.csn_refusals()])
def test_csn_refusals_name_the_name(engine, label, case, bad):
    rc, off, total = _c_csn(engine, case)
    assert rc == N.CC_E_INVALID and ("name %d:" % bad) in _err(engine) and ("field %s" % label[1]) in _err(engine), _err(engine)
    assert engine.lib.cc_names_read(engine.h, N.ptr(np.zeros(64, np.uint8)), 64) == N.CC_E_INVALID, "no blob after a refusal"
    it = case.interner()
    with pytest.raises(RuntimeError, match="name field id out of range") as host:
        csn_names(it, case.f9, case.suf)
    with pytest.raises(RuntimeError, match="name field id out of range") as dev:
        engine.csn_names(it, case.f9, case.suf)
    assert type(dev.value) is type(host.value) and str(dev.value) == str(host.value)


@pytest.mark.parametrize("label,case,bad,host_ok", NC.dcs_refusals(), ids=[r[0] for r in NC.dcs_refusals()])
def test_dcs_refusals_name_the_name(engine, tmp_path, label, case, bad, host_ok):
    ld = Names(engine, case.qnames, tmp_path, "bad_" + label)
    try:
        rc, off, total = _c_dcs(engine, ld.table, case)
        word = {"t_no_us": "no '_' in the tag", "t_no_colon": "no ':' in the tag", "d_no_colon": "no ':' in the partner",
                "t_empty": "no '_' in the tag", "d_empty": "no ':' in the partner", "t_one": "no '_' in the tag"}.get(
                    label, "record index outside the table")
        assert rc == N.CC_E_INVALID and ("name %d:" % bad) in _err(engine) and word in _err(engine), _err(engine)
        assert engine.lib.cc_names_read(engine.h, N.ptr(np.zeros(64, np.uint8)), 64) == N.CC_E_INVALID
        if host_ok:   # (the host function does not survive an index outside its handle)
            with pytest.raises(RuntimeError, match="IndexError in dcs_consensus_tag") as host:
                dcs_names(ld.bam, case.rec_tag, case.rec_ds)
            with pytest.raises(RuntimeError, match="IndexError in dcs_consensus_tag") as dev:
                engine.dcs_names(ld.bam, ld.table, case.rec_tag, case.rec_ds)
            assert type(dev.value) is type(host.value) and str(dev.value) == str(host.value)
    finally:
        ld.close()


def test_names_read_contract(engine):
    case = [c for c in NC.csn_cases() if c.name == "n65"][0]
    want = csn_names(case.interner(), case.f9, case.suf)
    rc, off, total = _c_csn(engine, case)
    assert rc == 0 and total > 1
    buf = np.full(total + 64, SENTINEL, np.uint8)
    assert engine.lib.cc_names_read(engine.h, N.ptr(buf), total - 1) == N.CC_E_INVALID
    assert (buf == SENTINEL).all(), "a short cap copies nothing"
    rc, blob = _read(engine, total)
    assert rc == 0 and blob.tobytes() == want[0][:total].tobytes(), "a short cap keeps the buffer"
    assert engine.lib.cc_names_read(engine.h, N.ptr(buf), total) == N.CC_E_INVALID, "the read released it"
    # a blob nobody read is released by the next format call, which leaves its own
    assert _c_csn(engine, case)[0] == 0
    empty = [c for c in NC.csn_cases() if c.name == "n0"][0]
    rc, off, total = _c_csn(engine, empty)
    assert rc == 0 and total == 0 and off[0] == 0
    assert _read(engine, 0)[0] == 0


def test_names_with_a_nul_go_to_the_host(engine, tmp_path):
    """A record whose name holds a NUL before its terminator: the table keeps the name up to it, the host
    formatter reads l_read_name - 1 bytes, so ccio_dcs_names_plain says 0 and Engine.dcs_names gives the
    host's bytes."""
    good = UC.Rec(b"AC.GT_0_1_0_2_150M_150M_pos_9:3\x00", [1, 2], [30, 30], [(0, 2)])
    nul = UC.Rec(b"TT.AA_0_1_0_2_150M\x00150M_neg_9:4\x00", [1, 2], [30, 30], [(0, 2)])
    bam = Bam(UC.write_bam(str(tmp_path / "nul.bam"), [good, nul]))
    it = Interner()
    rec, table = engine.table(bam, it, MODE_DUPLEX)
    try:
        a, b = np.array([0, 0], np.int64), np.array([0, 1], np.int64)
        io = N.io()
        assert io.ccio_dcs_names_plain(bam.h, 1, N.ptr(a), N.ptr(b)) == 1
        assert io.ccio_dcs_names_plain(bam.h, 2, N.ptr(a), N.ptr(b)) == 0
        before = engine.launch_count()
        _same(engine.dcs_names(bam, table, a, b), dcs_names(bam, a, b), "nul")
        assert engine.launch_count() == before, "the fallback runs no kernel"
        _same(engine.dcs_names(bam, table, a[:1], b[:1]), dcs_names(bam, a[:1], b[:1]), "plain")
    finally:
        engine.free_table(table)


def test_profiling_scopes(engine, loaded):
    case = [c for c in NC.dcs_cases() if c.name == "n257"][0]
    engine.set_profiling(True)
    try:
        engine.kernel_times()
        engine.dcs_names(loaded.bam, loaded.table, case.rec_tag, case.rec_ds)
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert times["name_sizes"][1] == 1 and times["name_write"][1] == 1 and times["name_scan"][1] == 1, times


def test_switch_and_environment(engine, monkeypatch):
    assert engine.names_device is False
    assert engine.device_names(True) is False and engine.names_device is True
    assert engine.device_names(False) is True and engine.names_device is False
    monkeypatch.setenv("CC_NAMES_DEVICE", "1")
    e = Engine(0)
    try:
        assert e.names_device is True
    finally:
        e.close()


@pytest.mark.parametrize("all_on", [False, True])
def test_golden_basic_with_the_device_names(engine, tmp_path, all_on):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, "basic")
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    if kw.get("bedfile", "False") != "False":
        kw["bedfile"] = os.path.join(d, kw["bedfile"])
    if all_on:
        kw.update(bgzf="device", inflate="device", decode="device", resident="device", crc="device", assemble="device")
    shutil.copy(os.path.join(d, "input.bam"), str(tmp_path / "sample.bam"))
    engine.set_profiling(True)
    try:
        engine.kernel_times()
        out = consensus_pipeline(str(tmp_path / "sample.bam"), str(tmp_path), engine=engine, names="device", **kw)
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert not engine.names_device
    assert times.get("name_write", (0, 0))[1] >= 3, "the three emits must format on the device"
    exp = os.path.join(d, "expected")
    n = sum(assert_same_in_order(out[f[:-4]], os.path.join(exp, f), "basic/" + f)
            for f in sorted(os.listdir(exp)) if f.endswith(".bam"))
    assert n > 0
    assert open(out["stats"]).read() == open(os.path.join(exp, "stats.txt")).read()
