"""Name sets (cc_names_keep / _fetch / _free / _count), the SSCS names formatted from the group's own
buffers (cc_format_csn_names_group) and the assembler reading a set in place (cc_bam_assemble_names):
a kept blob against what cc_names_read and libccio's formatters give, the assembler on a set against
the assembler on host names (itself pinned to the host writer by tests/test_gpu_assemble.py), byte for
byte, and the whole pipeline with names_resident="device" against the same run without it and against
the fixtures.  The shapes are the smallest at which the new code can go wrong: a set whose last name
ends on the blob's zeroed tail, names at every residue mod 16, a prefix of a set, counts on both sides
of the kernels' block sizes (256 names a sizes block, 16 a write block)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

import assemble_cases as AC
import name_cases as NC
import unpack_cases as UC
from parity import GOLDEN, assert_same_in_order
from consensuscruncher_amd import native as N
from consensuscruncher_amd import synth
from consensuscruncher_amd.engine import (MODE_DUPLEX, MODE_SSCS, Bam, Engine, Interner, KeptNames, csn_names, dcs_names,
                                          make_specs, whole_file_stream, write_bam)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
BY_NAME = {c.name: c for c in NC.csn_cases()}


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    start = e.names_count(), e.resident_count()
    yield e
    assert (e.names_count(), e.resident_count()) == start, "a name set or a resident stream leaked"
    e.close()


@pytest.fixture(scope="module")
def loaded(engine, tmp_path_factory):
    """name_cases' dcs qnames as a BAM, opened, decoded and uploaded: (bam, table)."""
    bam = Bam(NC.Dcs("names", NC.QNAMES, [], []).write(tmp_path_factory.mktemp("names")))
    rec, table = engine.table(bam, Interner(), MODE_DUPLEX)
    yield bam, table
    engine.free_table(table)


def _err(engine):
    return engine.lib.cc_last_error(engine.h).decode()


def _format(engine, case):
    """cc_format_csn_names itself, the blob left pending: (off, total)."""
    it = case.interner()
    bc, bc_off = it.blob(0)
    cg, cg_off = it.blob(1)
    n = len(case.suf)
    off = np.zeros(n + 1, np.int64)
    total = C.c_int64(-7)
    assert engine.lib.cc_format_csn_names(engine.h, n, N.ptr(case.f9), N.ptr(case.suf), N.ptr(bc), N.ptr(bc_off),
                                          len(bc_off) - 1, N.ptr(cg), N.ptr(cg_off), len(cg_off) - 1, N.ptr(off),
                                          C.byref(total)) == 0
    return off, int(total.value)


def _keep(engine):
    nid = C.c_int64(-7)
    rc = engine.lib.cc_names_keep(engine.h, C.byref(nid))
    return rc, int(nid.value)


def _fetch(engine, nid, total, cap=None, slack=64):
    """cc_names_fetch into a buffer with sentinel bytes behind total: (result, the whole buffer)."""
    buf = np.full(total + slack, SENTINEL, np.uint8)
    got = int(engine.lib.cc_names_fetch(engine.h, nid, N.ptr(buf), total if cap is None else cap))
    assert (buf[total:] == SENTINEL).all(), "cc_names_fetch wrote behind total"
    return got, buf


# ---------------------------------------------------------------- the life cycle of a set
def test_set_life_cycle(engine):
    lib, h = engine.lib, engine.h
    case = BY_NAME["n65"]
    want = csn_names(case.interner(), case.f9, case.suf)
    start = engine.names_count()
    off, total = _format(engine, case)
    assert total == want[1][-1] > 1 and (off == want[1]).all()
    rc, nid = _keep(engine)
    assert rc == 0 and nid > 0 and engine.names_count() == start + 1
    # the pending blob is gone: no second set from it, nothing to read
    assert _keep(engine) == (N.CC_E_INVALID, 0) and "no formatted names" in _err(engine)
    assert lib.cc_names_read(h, N.ptr(np.zeros(total, np.uint8)), total) == N.CC_E_INVALID
    assert "no formatted names" in _err(engine)
    # a fetch does not consume: twice the same bytes, nothing behind total
    assert int(lib.cc_names_fetch(h, nid, None, 0)) == total, "blob NULL is a size query"
    for _ in range(2):
        got, buf = _fetch(engine, nid, total)
        assert got == total and buf[:total].tobytes() == want[0][:total].tobytes()
    got, buf = _fetch(engine, nid, total, cap=total - 1)
    assert got == N.CC_E_INVALID and (buf == SENTINEL).all(), "a short cap copies nothing"
    assert _fetch(engine, nid, total)[0] == total, "and leaves the set"
    # a format call in between leaves the set alone, and its own blob is read as always
    off2, total2 = _format(engine, BY_NAME["n1"])
    assert lib.cc_names_read(h, N.ptr(np.zeros(total2 + 1, np.uint8)), total2) == 0
    assert _fetch(engine, nid, total)[1][:total].tobytes() == want[0][:total].tobytes()
    # ids that name no set of this context
    for bad in (0, -1, nid + (1 << 40)):
        assert int(lib.cc_names_fetch(h, bad, None, 0)) == N.CC_E_INVALID
        assert lib.cc_names_free(h, bad) == N.CC_E_INVALID
    assert lib.cc_bam_assemble_names(h, -1) == N.CC_E_INVALID and lib.cc_bam_assemble_names(h, nid + (1 << 40)) == N.CC_E_INVALID
    assert lib.cc_names_free(h, nid) == 0 and engine.names_count() == start
    assert int(lib.cc_names_fetch(h, nid, None, 0)) == N.CC_E_INVALID, "use after free"
    assert lib.cc_names_free(h, nid) == N.CC_E_INVALID and lib.cc_bam_assemble_names(h, nid) == N.CC_E_INVALID


def test_ids_are_per_context_and_destroy_frees(engine):
    case = BY_NAME["n63"]
    start = engine.names_count()
    other = Engine(0)
    try:
        mine, _ = engine.csn_names(case.interner(), case.f9, case.suf, keep=True)
        theirs, _ = other.csn_names(case.interner(), case.f9, case.suf, keep=True)
        assert isinstance(mine, KeptNames) and isinstance(theirs, KeptNames) and mine != theirs and min(mine, theirs) > 0
        assert int(engine.lib.cc_names_fetch(engine.h, theirs, None, 0)) == N.CC_E_INVALID
        assert int(other.lib.cc_names_fetch(other.h, mine, None, 0)) == N.CC_E_INVALID
        assert engine.lib.cc_names_free(engine.h, theirs) == N.CC_E_INVALID
        assert engine.lib.cc_bam_assemble_names(engine.h, theirs) == N.CC_E_INVALID
        assert other.names_count() == 1
        engine.names_free(mine)
    finally:
        other.close()   # with its set live: cc_destroy frees it
    assert engine.names_count() == start


def test_empty_sets(engine, loaded):
    start = engine.names_count()
    empty = BY_NAME["n0"]
    nid, off = engine.csn_names(empty.interner(), empty.f9, empty.suf, keep=True)
    did, doff = engine.dcs_names(loaded[0], loaded[1], np.zeros(0, np.int64), np.zeros(0, np.int64), keep=True)
    assert isinstance(nid, KeptNames) and isinstance(did, KeptNames) and nid != did
    assert len(off) == 1 and off[0] == 0 and len(doff) == 1 and doff[0] == 0
    assert engine.names_count() == start + 2
    for s in (nid, did):
        assert int(engine.lib.cc_names_fetch(engine.h, s, None, 0)) == 0
        assert _fetch(engine, s, 0)[0] == 0
        assert engine.lib.cc_bam_assemble_names(engine.h, s) == 0 and engine.lib.cc_bam_assemble_names(engine.h, 0) == 0
        engine.names_free(s)
    assert engine.names_count() == start
    assert _keep(engine)[0] == N.CC_E_INVALID


# ---------------------------------------------------------------- kept equals read
@pytest.mark.parametrize("case", NC.csn_cases(), ids=[c.name for c in NC.csn_cases()])
def test_kept_csn_names_equal_the_host_formatter(engine, case):
    it = case.interner()
    want = csn_names(it, case.f9, case.suf)
    nid, off = engine.csn_names(it, case.f9, case.suf, keep=True)
    try:
        assert isinstance(nid, KeptNames) and (off == want[1]).all()
        n = int(want[1][-1])
        assert engine.names_fetch(nid)[:n].tobytes() == want[0][:n].tobytes()
    finally:
        engine.names_free(nid)


@pytest.mark.parametrize("case", NC.dcs_cases(), ids=[c.name for c in NC.dcs_cases()])
def test_kept_dcs_names_equal_the_host_formatter(engine, loaded, case):
    want = dcs_names(loaded[0], case.rec_tag, case.rec_ds)
    nid, off = engine.dcs_names(loaded[0], loaded[1], case.rec_tag, case.rec_ds, keep=True)
    try:
        assert isinstance(nid, KeptNames) and (off == want[1]).all()
        n = int(want[1][-1])
        assert engine.names_fetch(nid)[:n].tobytes() == want[0][:n].tobytes()
    finally:
        engine.names_free(nid)


def test_a_refused_format_falls_back_to_the_host_shape(engine):
    label, case, bad = NC.csn_refusals()[0]
    with pytest.raises(RuntimeError, match="name field id out of range"):
        engine.csn_names(case.interner(), case.f9, case.suf, keep=True)
    assert _keep(engine)[0] == N.CC_E_INVALID, "no blob after a refusal"


# ---------------------------------------------------------------- the assembler on a set
def _lengths_case(lengths):
    """A csn case whose names have these lengths (18 or more): a barcode of length - 18, empty cigars,
    zero fields, suffix 1 ("<barcode>_0_0_0_0___pos_0:1")."""
    bcs = sorted({b"A" * (ln - 18) for ln in lengths}, key=len)
    f9 = np.zeros((len(lengths), 9), np.int32)
    f9[:, 0] = [bcs.index(b"A" * (ln - 18)) for ln in lengths]
    return NC.Csn("lengths", f9, np.ones(len(lengths), np.int64), bcs=bcs, cgs=[b""])


def _row(kind, rec, name_id, k=0, src=0):
    return dict(kind=kind, src_file=src, src_rec=rec, name_id=name_id, flag=(99, 147)[k % 2], mapq=k % 61, tlen=k, rg_id=(k % 4) - 1,
                cons_off=14 * k, cons_len=AC.LS[k % len(AC.LS)] % 200)


NSRC0 = len(AC.sources()[0])


def _shape(label):
    """(csn case, spec rows, names the call says it has: None for all of the set's)"""
    RAW, REN, NEW = N.OUT_RAW, N.OUT_RENAME, N.OUT_NEW
    if label == "single":
        return _lengths_case([19]), [_row(REN, 3, 0)], None
    if label == "residues":
        return BY_NAME["residues"], [_row(REN, i % NSRC0, i, i) for i in range(64)], None
    if label == "last254":
        return _lengths_case([19, 30, 254]), [_row(NEW, 1, 2, 1), _row(REN, 2, 0, 2), _row(REN, 4, 2, 3), _row(NEW, 5, 1, 4)], None
    if label == "descending":
        return _lengths_case(list(range(20, 36))), [_row((REN, NEW)[i % 2], i, 15 - i, i) for i in range(16)], None
    if label == "shared":
        return _lengths_case([21, 40]), [_row(REN, 0, 1, 0), _row(NEW, 1, 1, 1), _row(REN, 2, 0, 2)], None
    if label == "mixed":
        rows = [_row((RAW, REN, NEW)[i % 3], i % NSRC0, -1 if i % 3 == 0 else (5 * i) % 8, i, src=0) for i in range(60)]
        rows += [_row((NEW, REN, RAW)[i % 3], i, -1 if i % 3 == 2 else i, i, src=1) for i in range(6)]
        return _lengths_case([18, 19, 25, 31, 32, 33, 100, 200]), rows, None
    assert label == "prefix"
    return _lengths_case(list(range(18, 28))), [_row((REN, NEW)[i % 2], i, 3 - i % 4, i) for i in range(12)], 4


SHAPES = ("single", "residues", "last254", "descending", "shared", "mixed", "prefix")
HEADER = AC.header_bytes(AC.header_pad(1))
CONS = AC._cons(np.random.default_rng(17), 4096)


def _assemble(engine, rows, name_off, sort, **names):
    srcs = [UC.stream_of(recs) for recs in AC.sources()]
    return engine.assemble(HEADER, srcs, AC._specs(rows), name_off=name_off, cons_seq=CONS[0], cons_qual=CONS[1],
                           rg_values=AC.RG_VALUES, sort=sort, **names)


@pytest.mark.parametrize("sort", [False, True], ids=["spec_order", "sorted"])
@pytest.mark.parametrize("label", SHAPES)
def test_assembler_on_a_set_equals_the_assembler_on_host_names(engine, label, sort):
    case, rows, used = _shape(label)
    it = case.interner()
    blob, off = csn_names(it, case.f9, case.suf)
    if label == "residues":
        assert {int(o) % 16 for o in off[:-1]} == set(range(16))
    if label == "last254":
        assert off[-1] - off[-2] == 254 and off[-1] % 16 != 0, "the last name ends inside the blob's last line"
    if label in ("descending", "prefix", "mixed", "shared", "single", "last254"):
        assert list(np.diff(off)) == [len(b) + 18 for b in (case.bcs[i] for i in case.f9[:, 0])]
    name_off = off if used is None else off[:used + 1]
    assert used is None or used < len(case.suf)
    want, at = _assemble(engine, rows, name_off, sort, names=blob[:int(name_off[-1])])
    nid, koff = engine.csn_names(it, case.f9, case.suf, keep=True)
    residents = engine.resident_count()
    try:
        assert isinstance(nid, KeptNames) and (koff == off).all()
        got, gat = _assemble(engine, rows, name_off, sort, names_id=nid)
        assert got == want and (gat == at).all(), "%s: the stream or at[] differs" % label
        kat, token = _assemble(engine, rows, name_off, sort, names_id=nid, keep=True)
        try:
            assert token > 0 and (kat == at).all() and engine.resident_fetch(token) == want
        finally:
            engine.resident_free(token)
        # the set is still whole
        assert engine.names_fetch(nid)[:int(off[-1])].tobytes() == blob[:int(off[-1])].tobytes()
    finally:
        engine.names_free(nid)
    assert engine.resident_count() == residents
    assert len(want) > len(HEADER)


@pytest.mark.parametrize("label", ["long_name", "name_id"])
def test_refusals_read_as_with_host_names(engine, label):
    case = _lengths_case([19, 255])
    it = case.interner()
    blob, off = csn_names(it, case.f9, case.suf)
    assert off[-1] - off[-2] == 255
    bad = _row(N.OUT_NEW, 2, 1, 2) if label == "long_name" else _row(N.OUT_RENAME, 2, 2, 2)   # (name_id == n_names)
    rows = [_row(N.OUT_RENAME, 0, 0, 0), _row(N.OUT_RAW, 1, -1, 1), bad]
    with pytest.raises(N.CCError) as host:
        _assemble(engine, rows, off, False, names=blob[:int(off[-1])])
    nid, _ = engine.csn_names(it, case.f9, case.suf, keep=True)
    residents = engine.resident_count()
    try:
        for keep in (False, True):
            with pytest.raises(N.CCError) as dev:
                _assemble(engine, rows, off, False, names_id=nid, keep=keep)
            assert str(dev.value) == str(host.value)
    finally:
        engine.names_free(nid)
    assert "spec 2:" in str(host.value) and ("254" if label == "long_name" else "name_id") in str(host.value)
    assert str(host.value).startswith("CC_E_INVALID") and engine.resident_count() == residents


def test_selection_rules(engine):
    case, rows, _ = _shape("descending")
    it = case.interner()
    blob, off = csn_names(it, case.f9, case.suf)
    want, at = _assemble(engine, rows, off, False, names=blob[:int(off[-1])])
    srcs = [UC.stream_of(recs) for recs in AC.sources()]

    def null_names(name_off):   # names NULL, names_bytes = name_off[-1] > 0: whatever set is selected
        return engine._assemble(HEADER, srcs, AC._specs(rows), None, name_off, CONS[0], CONS[1], None, AC.RG_VALUES, False,
                                False, True)
    with pytest.raises(N.CCError, match="CC_E_INVALID"):
        null_names(off)   # no set selected
    nid, _ = engine.csn_names(it, case.f9, case.suf, keep=True)
    try:
        assert engine.lib.cc_bam_assemble_names(engine.h, nid) == 0
        for _ in range(2):   # a call does not consume the selection
            got, gat = null_names(off)
            assert got == want and (gat == at).all()
        # more names or bytes than the set has: refused before any launch
        before = engine.launch_count()
        with pytest.raises(N.CCError, match="larger than the name set"):
            null_names(np.append(off, off[-1]))
        longer = off.copy()
        longer[-1] += 1
        with pytest.raises(N.CCError, match="larger than the name set"):
            null_names(longer)
        assert engine.launch_count() == before
        assert null_names(off)[0] == want, "a refusal leaves the selection"
        assert engine.lib.cc_bam_assemble_names(engine.h, 0) == 0
        with pytest.raises(N.CCError, match="CC_E_INVALID"):
            null_names(off)
        # freeing the selected set clears the selection as well
        assert engine.lib.cc_bam_assemble_names(engine.h, nid) == 0
    finally:
        engine.names_free(nid)
    with pytest.raises(N.CCError, match="CC_E_INVALID"):
        null_names(off)


def test_a_set_is_not_uploaded(engine):
    case, rows, _ = _shape("mixed")
    it = case.interner()
    blob, off = csn_names(it, case.f9, case.suf)
    nid, _ = engine.csn_names(it, case.f9, case.suf, keep=True)
    try:
        engine.set_profiling(True)
        want = _assemble(engine, rows, off, False, names=blob[:int(off[-1])])[0]
        host = engine.kernel_times()
        engine.set_profiling(False)
        engine.set_profiling(True)   # (clears the times)
        got = _assemble(engine, rows, off, False, names_id=nid)[0]
        dev = engine.kernel_times()
    finally:
        engine.set_profiling(False)
        engine.names_free(nid)
    assert got == want
    assert host["asm_names_upload"][1] >= 1 and host["k_asm_copy"][1] >= 1, host
    assert "asm_names_upload" not in dev and dev["k_asm_copy"][1] >= 1, dev


# ---------------------------------------------------------------- the group form
class Voted(object):
    """A synthetic input through read_bam and (vote=True) cc_consensus_maker."""

    def __init__(self, engine, d, n_pairs, seed, vote=True, **kw):
        batch = synth.generate(n_pairs, seed=synth.SEED_BASE + seed, contigs=(("chr1", 100_000),), **kw)
        path = os.path.join(str(d), "g%d.bam" % seed)
        synth.write_bam_native(batch, path, level=1)
        self.engine, self.it, self.bam = engine, Interner(), Bam(path)
        rec = self.bam.decode(self.it, MODE_SSCS, "|")
        self.table = engine.upload(rec)
        self.g = engine.read_bam(self.table, whole_file_stream(rec), delim_filter=1, badread_file=1, scope_by_run=0)
        if vote:
            engine.consensus_maker(self.g, 0.7)

    def close(self):
        self.engine.free_group(self.g)
        self.engine.free_table(self.table)

    def host_names(self):
        e = self.engine
        ckey = np.repeat(e.fetch(self.g, "emit_ckey", np.int32).reshape(-1, 9), 2, axis=0).reshape(-1)
        return csn_names(self.it, ckey, e.fetch(self.g, "emit_n", np.int32))

    def c_call(self):
        bc, bc_off = self.it.blob(0)
        cg, cg_off = self.it.blob(1)
        off = np.zeros(1 << 12, np.int64)
        total = C.c_int64(-7)
        return self.engine.lib.cc_format_csn_names_group(self.engine.h, self.g, N.ptr(bc), N.ptr(bc_off), len(bc_off) - 1,
                                                         N.ptr(cg), N.ptr(cg_off), len(cg_off) - 1, N.ptr(off), C.byref(total))


# (pairs, seed, generator options, the names it must give): fewer than 16; more than 256 and no multiple
# of 16, so past one sizes block and into a part-filled write block; none at all (every spacer bad)
GROUPS = [("few", 3, 9001, {}, lambda n: 0 < n < 16),
          ("blocks", 600, 9004, {}, lambda n: n > 256 and n % 16 != 0),
          ("none", 4, 9006, dict(spacer_bad_frac=1.0), lambda n: n == 0)]


@pytest.mark.parametrize("label,pairs,seed,kw,counts", GROUPS, ids=[g[0] for g in GROUPS])
def test_group_names_equal_the_uploaded_form(engine, tmp_path, label, pairs, seed, kw, counts):
    v = Voted(engine, tmp_path, pairs, seed, **kw)
    try:
        want = v.host_names()
        n = len(want[1]) - 1
        assert counts(n), "%s: %d names: the input no longer covers its case" % (label, n)
        before = engine.launch_count()
        blob, off = engine.csn_names_group(v.g, v.it)
        assert engine.launch_count() > before or n == 0, "the kernels did not run"
        total = int(want[1][-1])
        assert (off == want[1]).all() and blob[:total].tobytes() == want[0][:total].tobytes()
        # the uploaded form on the same fields, and the kept form
        up = engine.csn_names(v.it, np.repeat(engine.fetch(v.g, "emit_ckey", np.int32).reshape(-1, 9), 2, axis=0),
                              engine.fetch(v.g, "emit_n", np.int32))
        assert (up[1] == off).all() and up[0][:total].tobytes() == blob[:total].tobytes()
        nid, koff = engine.csn_names_group(v.g, v.it, keep=True)
        try:
            assert isinstance(nid, KeptNames) and (koff == off).all()
            assert engine.names_fetch(nid)[:total].tobytes() == blob[:total].tobytes()
        finally:
            engine.names_free(nid)
    finally:
        v.close()


def test_group_that_has_not_voted_is_refused(engine, tmp_path):
    v = Voted(engine, tmp_path, 3, 9001, vote=False)
    try:
        before = engine.launch_count()
        assert v.c_call() == N.CC_E_INVALID and "cc_consensus_maker" in _err(engine)
        assert engine.launch_count() == before
        assert _keep(engine)[0] == N.CC_E_INVALID, "no blob after a refusal"
        g, v.g = v.g, v.g + 1000
        assert v.c_call() == N.CC_E_INVALID and "unknown group" in _err(engine)
        v.g = g
        engine.consensus_maker(v.g, 0.7)
        assert v.c_call() == 0 and engine.lib.cc_names_read(engine.h, N.ptr(np.zeros(1 << 16, np.uint8)), 1 << 16) == 0
    finally:
        v.close()


# ---------------------------------------------------------------- write_bam and the fallback
def test_write_bam_reads_the_set_and_falls_back_once(engine, tmp_path):
    source = Bam(os.path.join(GOLDEN, "basic", "input.bam"))
    case = BY_NAME["residues"]   # (64 names of 33 bytes: none the assembler refuses)
    it = case.interner()
    blob, off = csn_names(it, case.f9, case.suf)
    sp = make_specs(64)
    sp["kind"] = N.OUT_RENAME
    sp["src_rec"] = np.arange(64)
    sp["name_id"] = np.arange(64)[::-1]
    host = str(tmp_path / "host.bam")
    write_bam(host, source, Interner(), sp, [source], blob, off, level=1)
    nid, _ = engine.csn_names(it, case.f9, case.suf, keep=True)
    was = engine.device_assemble(True)
    try:
        engine.set_profiling(True)
        p = str(tmp_path / "set.bam")
        write_bam(p, source, Interner(), sp, [source], None, off, level=1, names_dev=(engine, nid))
        t = engine.kernel_times()
        assert open(p, "rb").read() == open(host, "rb").read()
        assert t["k_asm_copy"][1] >= 1 and "asm_names_upload" not in t and "name_download" not in t, t
        # a view never reaches a hook: the set is fetched, once, and the host writes the file
        engine.set_profiling(False)
        engine.set_profiling(True)
        p = str(tmp_path / "view.bam")
        write_bam(p, source, Interner(), sp, [Bam.combine([source], key=2)], None, off, level=1, names_dev=(engine, nid))
        t = engine.kernel_times()
        assert open(p, "rb").read() == open(host, "rb").read()
        assert t["name_download"][1] == 1 and "k_asm_copy" not in t, t
        # the selection was cleared either way
        assert engine.names_count() >= 1
        with pytest.raises(N.CCError, match="CC_E_INVALID"):
            engine._assemble(HEADER, [], make_specs(1), None, off, None, None, None, (), False, False, True)
    finally:
        engine.set_profiling(False)
        engine.device_assemble(was)
        engine.names_free(nid)


# ---------------------------------------------------------------- the pipelines
def test_switch_and_environment(engine, monkeypatch):
    assert engine.names_resident_device is False
    assert engine.device_names_resident(True) is False
    try:
        assert engine.names_resident_device is False, "without names_device and assemble_device it has no effect"
        engine.device_names(True)
        assert engine.names_resident_device is False
        engine.device_assemble(True)
        assert engine.names_resident_device is True
        engine.device_names(False)
        assert engine.names_resident_device is False
    finally:
        engine.device_assemble(False)
        engine.device_names(False)
        assert engine.device_names_resident(False) is True
    monkeypatch.setenv("CC_NAMES_RESIDENT_DEVICE", "1")
    e = Engine(0)
    try:
        assert e._names_resident_want is True and e.names_resident_device is False
    finally:
        e.close()
    from consensuscruncher_amd.pipeline import consensus_pipeline
    from consensuscruncher_amd.sharded import sharded_pipeline
    with pytest.raises(ValueError, match="names_resident"):
        consensus_pipeline("missing.bam", "out", names_resident="bogus")
    with pytest.raises(ValueError, match="names_resident"):
        sharded_pipeline("missing.bam", "out", "False", None, None, names_resident="bogus")


def _files(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".bam") or f.endswith(".bai"):
                out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


class Spy(object):
    """Engine.csn_names_group counted: its calls, whether each ran kernels and kept its blob."""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = Engine.csn_names_group

        def wrapped(eng, group, interner, keep=False):
            before = eng.launch_count()
            r = inner(eng, group, interner, keep)
            self.calls.append((eng.launch_count() - before, isinstance(r[0], KeptNames)))
            return r
        monkeypatch.setattr(Engine, "csn_names_group", wrapped)


def _run_twice(engine, tmp_path, run, min_uploads=3):
    """run(root, names_resident) without and with the option, profiled: (outputs of the run with it, the two
    runs' kernel times)."""
    times = {}
    outs = {}
    for mode in ("host", "device"):
        root = str(tmp_path / mode)
        os.makedirs(root)
        engine.set_profiling(True)
        try:
            outs[mode] = run(root, mode)
            times[mode] = engine.kernel_times()
        finally:
            engine.set_profiling(False)
        assert engine.names_count() == 0 and not engine.names_resident_device and not engine.names_device
    off, on = _files(str(tmp_path / "host")), _files(str(tmp_path / "device"))
    assert sorted(on) == sorted(off) and len(on) >= 12
    for f in on:
        assert on[f] == off[f], f
    # without the option every named write the assembler takes uploads its names
    assert times["host"].get("asm_names_upload", (0, 0))[1] >= min_uploads, times["host"]
    assert "asm_names_upload" not in times["device"], times["device"].get("asm_names_upload")
    assert times["device"]["name_write"][1] >= 3
    return outs["device"], times


def _fixtures(out, d, label):
    exp = os.path.join(d, "expected")
    n = sum(assert_same_in_order(out[f[:-4]], os.path.join(exp, f), label + "/" + f)
            for f in sorted(os.listdir(exp)) if f.endswith(".bam"))
    assert n > 0


@pytest.mark.parametrize("resident_out", [False, True], ids=["assemble", "out_resident"])
@pytest.mark.parametrize("case", ["basic", "bed_multi"])
def test_pipeline_files_are_the_same_with_resident_names(engine, tmp_path, monkeypatch, case, resident_out):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, case)
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    if kw.get("bedfile", "False") != "False":
        kw["bedfile"] = os.path.join(d, kw["bedfile"])
    kw.update(names="device", assemble="device")
    if resident_out:
        kw.update(bgzf="device", out_resident="device")
    spy = Spy(monkeypatch)

    def run(root, mode):
        shutil.copy(os.path.join(d, "input.bam"), os.path.join(root, "sample.bam"))
        residents = engine.resident_count()
        out = consensus_pipeline(os.path.join(root, "sample.bam"), root, engine=engine, names_resident=mode, **kw)
        assert engine.resident_count() == residents
        return out
    out, times = _run_twice(engine, tmp_path, run)
    # only the run with the option formats from the group, on the device, and keeps the blob there
    assert len(spy.calls) == 1 and spy.calls[0][0] >= 3 and spy.calls[0][1], spy.calls
    _fixtures(out, d, case)
    assert open(out["stats"]).read() == open(os.path.join(d, "expected", "stats.txt")).read()


def test_sharded_pipeline_files_are_the_same_with_resident_names(engine, tmp_path, monkeypatch):
    from consensuscruncher_amd.sharded import LocalComm, sharded_pipeline
    d = os.path.join(GOLDEN, "bed_multi")
    bed = os.path.join(d, json.load(open(os.path.join(d, "params.json")))["run"]["bedfile"])
    spy = Spy(monkeypatch)

    def run(root, mode):
        shutil.copy(os.path.join(d, "input.bam"), os.path.join(root, "sample.bam"))
        return sharded_pipeline(os.path.join(root, "sample.bam"), root, bed, LocalComm(3), engine, level=1, names="device",
                                assemble="device", names_resident=mode)
    # (a rank's combined and routed views never reach the assembler: their writes take the fetched blob)
    out, times = _run_twice(engine, tmp_path, run, min_uploads=0)
    assert len(spy.calls) == 3 and all(c[1] for c in spy.calls), spy.calls   # a rank each
    _fixtures(out, d, "bed_multi x3")
