"""The device merge of sorted record sets (cc_bam_merge: k_merge_keys, k_merge_rank, k_merge_sizes,
k_merge_copy) against numpy: np.argsort(keys of the concatenation, kind="stable") and the records'
bytes gathered in that order.  merge_kept with the option off is the second witness for the writer
and the pipeline; the device path is never its own reference.  The sizes, windows and slices sit at
the edges csrc/merge_core.h names (MRG_TILE, MRG_WIN), read from that file."""
import json
import os
import re
import shutil
import struct

import numpy as np
import pytest

from parity import GOLDEN
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam, Engine, Interner, Sink, flush_writes, make_specs, merge_kept, write_bam

pytestmark = pytest.mark.gpu

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
CORE = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "consensuscruncher_amd", "csrc",
                         "merge_core.h")).read()
MAX_SRC, TILE, WIN = (int(re.search(r"constexpr int %s = (\d+);" % k, CORE).group(1))
                      for k in ("MRG_MAX_SRC", "MRG_TILE", "MRG_WIN"))
HEADER = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", 0) + b"x"   # 13 bytes: the records start unaligned


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


def rec(tid, pos, flag=0, nl=4, ncig=0, fill=b"q"):
    """One raw record: a name of nl bytes (NUL included, 1..7 reach every alignment), ncig cigar ops."""
    name = fill * (nl - 1) + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, nl, 0, 4680, ncig, flag, 0, -1, -1, 0) + name
    body += b"".join(struct.pack("<I", (1 + k % 9) << 4) for k in range(ncig))
    return struct.pack("<i", len(body)) + body


def key_of(tid, pos, flag):
    return ((tid & 0xffffffff) << 32) | (((pos + 1) & 0xffffffff) << 1) | ((flag >> 4) & 1)


def source(items):
    """(stream, rec_off, keys, records) of a list of (tid, pos, flag, nl, ncig) already in key order."""
    recs = [rec(*it, fill=bytes([97 + i % 26])) for i, it in enumerate(items)]
    off = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64) if recs else np.zeros(0, np.uint64)
    keys = np.array([key_of(*it[:3]) for it in items], np.uint64)
    assert (keys[1:] >= keys[:-1]).all()
    return b"".join(recs), off, keys, recs


def expect(srcs):
    keys = np.concatenate([s[2] for s in srcs]) if srcs else np.zeros(0, np.uint64)
    recs = [r for s in srcs for r in s[3]]
    org = np.argsort(keys, kind="stable")
    at = np.cumsum([len(HEADER)] + [len(recs[g]) for g in org]).astype(np.uint64)
    return HEADER + b"".join(recs[g] for g in org), at, org.astype(np.uint32)


def check(engine, srcs, args=None):
    stream, at, org = engine.merge(HEADER, args if args is not None else [(s[0], s[1]) for s in srcs])
    want, wat, worg = expect(srcs)
    assert (org == worg).all()
    assert (at == wat).all()
    assert stream == want


SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def items(pattern, s, n, nsrc):
    """n records of source s in key order."""
    out = []
    for i in range(n):
        nl, ncig = 1 + (i + s) % 7, 0
        if pattern == "equal":
            tid, pos, flag = 2, 77, 16
        elif pattern == "interleaved":
            tid, pos, flag = 0, i * nsrc + s, 0
        elif pattern == "before":      # source 0 wholly before the others, the last wholly after
            tid, pos, flag = (0, i, 0) if s == 0 else ((5, i, 0) if s == nsrc - 1 and nsrc > 2 else (1, i // 3, 0))
        else:                          # "mixed": pos -1, both reverse bits, tid -1 last, a 300-op cigar
            q = 4 * i // max(n, 1)
            tid, pos, flag = [(0, -1, 16 * (i & 1)), (0, i, 0), (3, 2 ** 31 - 2, 16 * (i & 1)), (-1, -1, 0)][q]
            ncig = 300 if (s == 0 and i == n // 2) else 0
        out.append((tid, pos, flag, nl, ncig))
    out.sort(key=lambda it: key_of(*it[:3]))
    return out


@pytest.mark.parametrize("nsrc", [1, 2, 3, MAX_SRC])
@pytest.mark.parametrize("pattern", ["equal", "interleaved", "before", "mixed"])
def test_merge_equals_the_stable_argsort(engine, pattern, nsrc):
    rot = {"equal": 0, "interleaved": 1, "before": 2, "mixed": 3}[pattern] + nsrc
    srcs = [source(items(pattern, s, SIZES[(s + rot) % len(SIZES)], nsrc)) for s in range(nsrc)]
    check(engine, srcs)


def test_every_size_meets_every_size(engine):
    """two sources, all keys equal (stability), at each pair of the edge sizes"""
    made = {n: source(items("equal", 0, n, 2)) for n in SIZES}
    for a in SIZES:
        for b in SIZES:
            check(engine, [made[a], made[b]])


@pytest.mark.parametrize("w", [0, 1, WIN, WIN + 1])
def test_window_of_one_tile(engine, w):
    """one tile of source 0 whose window in source 1 holds w keys: up to MRG_WIN staged in LDS, one more
    bisected in global memory; ties inside the window go to source 0"""
    a = [(0, 1000 + i, 0, 1 + i % 7, 0) for i in range(TILE)]
    b = [(0, 10, 0, 3, 0)] * 5 + [(0, 1000 + (i * TILE) // max(w, 1), 0, 2 + i % 5, 0) for i in range(w)] + \
        [(0, 5000, 16, 4, 0)] * 5
    srcs = [source(a), source(b)]
    lo, hi = np.searchsorted(srcs[1][2], srcs[0][2][0], "left"), np.searchsorted(srcs[1][2], srcs[0][2][-1], "right")
    assert hi - lo == w
    check(engine, srcs)
    check(engine, srcs[::-1])   # the same window seen from the later source (ties go the other way)


def test_resident_sources_and_keep(engine):
    srcs = [source(items("mixed", s, SIZES[(s + 2) % len(SIZES)], 3)) for s in range(3)]
    before = engine.resident_count()
    pad = b"\xee" * 21   # the records at an odd base inside the resident stream
    rids = [engine.resident_put(pad + s[0]) for s in srcs]
    try:
        args = [(None, s[1], rid, len(pad), len(s[0])) for s, rid in zip(srcs, rids)]
        check(engine, srcs, args)
        check(engine, srcs, [args[0], (srcs[1][0], srcs[1][1]), args[2]])   # resident and host sources together
        want, wat, worg = expect(srcs)
        at, org, token = engine.merge(HEADER, args, keep=True)
        try:
            assert token > 0 and engine.resident_count() == before + 4
            assert (at == wat).all() and (org == worg).all()
            assert engine.resident_fetch(token) == want
            f = engine.index_fields(token, at)
            assert (f["block_size"].astype(np.uint64) + 4 == np.diff(at)).all()
        finally:
            engine.resident_free(token)
    finally:
        for rid in rids:
            engine.resident_free(rid)
    assert engine.resident_count() == before


def test_three_slices_give_the_same_stream(engine, monkeypatch):
    srcs = [source(items("mixed", s, TILE + 1 + s, 3)) for s in range(3)]
    n = sum(len(s[1]) for s in srcs)
    largest = max(len(r) for s in srcs for r in s[3])
    monkeypatch.setenv("CC_ASM_SLICE_BYTES", str(largest * ((n + 2) // 3)))
    engine.set_profiling(True)
    try:
        engine.kernel_times()
        check(engine, srcs)
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert times["k_merge_copy"][1] == 3 and times["k_merge_rank"][1] == 1


def test_empty_merges(engine):
    check(engine, [])
    check(engine, [source([])])
    check(engine, [source([]), source([(0, 1, 0, 2, 0)]), source([])])


def test_refusals_leave_nothing_resident(engine):
    good = source(items("interleaved", 0, TILE + 3, 2))
    other = source(items("interleaved", 1, 5, 2))
    before = engine.resident_count()

    def refused(srcs, code, *words):
        for keep in (False, True):
            with pytest.raises(N.CCError) as ei:
                engine.merge(HEADER, srcs, keep=keep)
            assert ei.value.code == code, str(ei.value)
            for w in words:
                assert w in str(ei.value), str(ei.value)
            assert engine.resident_count() == before
    # an offset past the source (record 2 of source 1)
    off = other[1].copy()
    off[2] = len(other[0]) + 40
    refused([(good[0], good[1]), (other[0], off)], N.CC_E_INVALID, "source 1 record 2", "outside")
    # block_size 31 (record TILE + 1 of source 0: past the first block)
    st = bytearray(good[0])
    a = int(good[1][TILE + 1])
    st[a:a + 4] = struct.pack("<i", 31)
    refused([(bytes(st), good[1]), (other[0], other[1])], N.CC_E_INVALID, "source 0 record %d" % (TILE + 1), "block_size < 32")
    # the last record runs past the end of its source
    refused([(good[0], good[1]), (other[0][:-1], other[1])], N.CC_E_INVALID, "source 1 record 4", "past")
    # an out-of-order pair: records TILE - 1 and TILE of source 0 exchanged (the pair straddles two blocks)
    it = items("interleaved", 0, TILE + 3, 2)
    it[TILE - 1], it[TILE] = it[TILE], it[TILE - 1]
    recs = [rec(*x) for x in it]
    ooo = (b"".join(recs), np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64))
    refused([ooo, (other[0], other[1])], N.CC_E_INVALID, "source 0 record %d" % TILE, "key order")
    refused([(other[0], other[1]), ooo], N.CC_E_INVALID, "source 1 record %d" % TILE, "key order")
    # nine sources
    refused([(other[0], other[1])] * (MAX_SRC + 1), N.CC_E_UNSUPPORTED)
    check(engine, [good, other])   # and the engine merges on


# ---------------------------------------------------------------- the writer and the pipeline
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Three sorted kept handles over overlapping slices of the golden input (ties across the inputs)."""
    src = Bam(INPUT)
    hs = []
    for k, (a, b) in enumerate([(0, 700), (500, 1300), (250, 600)]):
        b = min(b, src.n)
        sp = make_specs(b - a)
        sp["kind"] = N.OUT_RAW
        sp["src_rec"] = np.arange(a, b)
        p = str(tmp_path_factory.mktemp("in%d" % k) / "in.bam")
        sink = Sink(fused=[p], keep=[p])
        out = write_bam(p, src, Interner(), sp, [src], level=1, sink=sink)
        hs.append(sink.take(out))
    yield hs
    for h in hs:
        h.close()


@pytest.mark.parametrize("asy", [False, True])
@pytest.mark.parametrize("resident", [False, True])
def test_merge_kept_files_are_the_same_with_the_device_merge(engine, inputs, tmp_path, resident, asy):
    was = (engine.device_assemble(True), engine.device_bgzf(True), engine.device_out_resident(True)) if resident else None
    before = engine.resident_count()
    try:
        assert engine.out_resident_device == resident
        got = {}
        for tag in ("off", "on"):
            was_m = engine.device_merge(tag == "on")
            engine.set_profiling(True)
            try:
                engine.kernel_times()
                p = str(tmp_path / (tag + ".sorted.bam"))
                h = merge_kept(p, inputs, level=1, async_writes=asy)
                flush_writes()
                times = engine.kernel_times()
            finally:
                engine.set_profiling(False)
                engine.device_merge(was_m)
            assert times.get("k_merge_rank", (0, 0))[1] == (1 if tag == "on" else 0)
            got[tag] = (open(p, "rb").read(), open(p + ".bai", "rb").read(), h.pack(np.arange(h.n, dtype=np.int64)).tobytes())
            h.close()
            assert engine.resident_count() == before
        assert got["on"][2] == got["off"][2]
        assert got["on"][1] == got["off"][1]
        assert got["on"][0] == got["off"][0]
    finally:
        if was:
            engine.device_out_resident(was[2])
            engine.device_bgzf(was[1])
            engine.device_assemble(was[0])


@pytest.mark.parametrize("others", [False, True])
def test_golden_basic_pipeline_is_the_same_with_the_device_merge(engine, tmp_path, others):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, "basic")
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    if kw.get("bedfile", "False") != "False":
        kw["bedfile"] = os.path.join(d, kw["bedfile"])
    kw["all_unique_sscs"] = True
    if others:
        kw.update(assemble="device", bgzf="device", out_resident="device")

    def run(tag, **more):
        (tmp_path / tag).mkdir()
        shutil.copy(os.path.join(d, "input.bam"), str(tmp_path / tag / "sample.bam"))
        before = engine.resident_count()
        engine.set_profiling(True)
        try:
            engine.kernel_times()
            consensus_pipeline(str(tmp_path / tag / "sample.bam"), str(tmp_path / tag), engine=engine, **dict(kw, **more))
            times = engine.kernel_times()
        finally:
            engine.set_profiling(False)
        assert engine.resident_count() == before and not engine.merge_device
        out = {}
        for root, _, files in os.walk(str(tmp_path / tag)):
            for f in files:
                if f.endswith(".bam") or f.endswith(".bai"):
                    out[os.path.relpath(os.path.join(root, f), str(tmp_path / tag))] = open(os.path.join(root, f), "rb").read()
        return out, times
    off, t_off = run("off")
    on, t_on = run("on", merge="device")
    assert t_off.get("k_merge_rank", (0, 0))[1] == 0 and t_on["k_merge_rank"][1] == 3   # sscs.sc, all.unique.dcs, all.unique.sscs
    assert sorted(on) == sorted(off) and any("all.unique" in f for f in on)
    for f in on:
        assert on[f] == off[f], f
