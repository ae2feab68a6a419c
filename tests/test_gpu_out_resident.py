"""The output stream kept on the device: cc_bam_assemble_keep against cc_bam_assemble, cc_index_fields
(k_index_fields) against a numpy restatement over the fetched bytes, cc_bgzf_deflate_resident against
cc_bgzf_deflate byte for byte, and the writer, Engine.pin_source and the pipeline with
device_out_resident on against the same run with it off (same files, same .bai, same kept records)."""
import json
import os
import shutil
import struct

import numpy as np
import pytest

import assemble_cases as AC
from parity import GOLDEN
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import (Bam, Engine, Interner, MemorySink, Sink, flush_writes, make_specs,
                                          write_bam)

pytestmark = pytest.mark.gpu

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
PIECE = 0xff00


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- cc_bam_assemble_keep
def _assemble_args(case, sort):
    import unpack_cases as UC
    srcs = [UC.stream_of(recs) for recs in case.sources]
    return (AC.header_bytes(case.pad), srcs, case.specs), dict(
        names=case.names_blob[:-1], name_off=case.name_off, cons_seq=case.cons_seq, cons_qual=case.cons_qual,
        rg_values=case.rgs, sort=sort)


KEEP_CASES = [("main%d" % r, lambda r=r: AC.main_case(AC.header_pad(r))) for r in (0, 1, 15)]
KEEP_CASES += [("empty", lambda: AC.empty_case(AC.header_pad(15)))] + [("one%d" % k, lambda k=k: AC.one_case(k)) for k in (0, 1, 2)]


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("label,make", KEEP_CASES, ids=[c[0] for c in KEEP_CASES])
def test_assemble_keep_equals_assemble(engine, label, make, sort):
    a, kw = _assemble_args(make(), sort)
    before = engine.resident_count()
    stream, at = engine.assemble(*a, **kw)
    at2, token = engine.assemble(*a, keep=True, **kw)
    try:
        assert token > 0 and engine.resident_count() == before + 1
        assert (at2 == at).all()
        assert engine.resident_fetch(token) == stream
    finally:
        engine.resident_free(token)
    assert engine.resident_count() == before


def test_assemble_keep_refusal_leaves_no_stream(engine):
    _, case, bad, word = AC.refusals()[0]
    a, kw = _assemble_args(case, False)
    before = engine.resident_count()
    with pytest.raises(N.CCError) as ei:
        engine.assemble(*a, keep=True, **kw)
    assert ei.value.code == N.CC_E_INVALID and ("spec %d:" % bad) in str(ei.value)
    assert engine.resident_count() == before


# ---------------------------------------------------------------- cc_index_fields
def _rec(tid, pos, flag, name, cigar, block_size=None, n_cigar=None):
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 30, 4680, len(cigar) if n_cigar is None else n_cigar,
                       flag, 5, -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cigar) + bytes(range(8))
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def _records(n):
    """n records at every byte alignment: one-op cigars, one 300-op cigar, an unmapped record with a
    cigar and one without a reference."""
    out = []
    for i in range(n):
        name = b"r" * (1 + i % 7)
        if i == n // 2:
            out.append(_rec(1, 10 + i, 0, name, [((k % 5 + 1) << 4) | (k % 10) for k in range(300)]))
        elif i == n // 2 + 1:
            out.append(_rec(1, 10 + i, 4, name, [(20 << 4) | 0, (7 << 4) | 2]))
        elif i == n - 1 and n > 2:
            out.append(_rec(-1, -1, 4, name, []))
        else:
            out.append(_rec(i % 3, 10 + i if i else -1, 16 * (i & 1), name, [((30 + i % 50) << 4) | (0, 7, 8)[i % 3]]))
    return out


def _put(engine, recs, lead=b"\xee\xee\xee"):
    stream = lead + b"".join(recs)
    at = np.cumsum([len(lead)] + [len(r) for r in recs]).astype(np.uint64)
    return engine.resident_put(stream), stream, at


def _fields(stream, at):
    out = np.zeros(len(at) - 1, N.INDEX_FIELD_DTYPE)
    for i, a in enumerate(at[:-1]):
        bs, tid, pos, lqn, _, _, ncig, flag = struct.unpack_from("<iiiBBHHH", stream, int(a))
        c = np.frombuffer(stream, "<u4", ncig, int(a) + 36 + lqn) if not flag & 4 else np.zeros(0, np.uint32)
        rl = int((c >> 4)[np.isin(c & 15, (0, 2, 3, 7, 8))].sum())
        out[i] = (tid, pos, bs, min(rl, 0x7fffffff) | (0x80000000 if flag & 4 else 0))
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_index_fields_equal_the_restatement(engine, n):
    before = engine.resident_count()
    token, stream, at = _put(engine, _records(n))
    try:
        assert int(at[-1]) == len(stream)   # the last record ends at the stream's last byte
        fetched = engine.resident_fetch(token)
        assert fetched == stream
        got = engine.index_fields(token, at)
        want = _fields(fetched, at)
        assert got.tobytes() == want.tobytes()
        if n > 2:
            assert (got["rl"][n // 2 + 1], got["tid"][n - 1], got["rl"][n - 1]) == (0x80000000, -1, 0x80000000)
    finally:
        engine.resident_free(token)
    assert engine.resident_count() == before


def test_index_fields_saturates(engine):
    token, stream, at = _put(engine, [_rec(0, 5, 0, b"big", [(0x0fffffff << 4) | (0, 3)[k % 2] for k in range(9)])])
    try:
        assert int(engine.index_fields(token, at)["rl"][0]) == 0x7fffffff
    finally:
        engine.resident_free(token)


def test_index_fields_refusals_name_their_record(engine):
    recs = _records(70)
    cases = []
    short = list(recs)
    short[66] = _rec(0, 1, 0, b"", [], block_size=31)[:35] + b"\0"
    cases.append((short, None, 66, "block_size under 32"))
    long_cigar = list(recs)
    long_cigar[65] = _rec(0, 1, 0, b"x", [16, 32, 48], n_cigar=65535)
    cases.append((long_cigar, None, 65, "n_cigar_op"))
    cases.append((recs, 40, 39, "at[i + 1]"))   # at[40] moved: record 39's span is the first that is wrong
    for rs, moved, bad, word in cases:
        token, stream, at = _put(engine, rs)
        try:
            if moved is not None:
                at[moved] += 1
            with pytest.raises(N.CCError) as ei:
                engine.index_fields(token, at)
            assert ei.value.code == N.CC_E_INVALID and ("record %d:" % bad) in str(ei.value) and word in str(ei.value)
        finally:
            engine.resident_free(token)
    token, stream, at = _put(engine, recs)
    try:
        at[-1] += 1
        with pytest.raises(N.CCError) as ei:
            engine.index_fields(token, at)
        assert ei.value.code == N.CC_E_INVALID and "past the stream" in str(ei.value)
    finally:
        engine.resident_free(token)
    with pytest.raises(N.CCError):
        engine.index_fields(token, at)   # freed: an unknown id


# ---------------------------------------------------------------- cc_bgzf_deflate_resident
@pytest.fixture(scope="module")
def text():
    """257 pieces and a byte of compressible bytes (it crosses BG_CHUNK), and the stream holding them."""
    rng = np.random.default_rng(11)
    words = rng.integers(0, 256, (4096, 12), dtype=np.uint8)
    pick = rng.integers(0, 4096, (257 * PIECE + PIECE + 1) // 12 + 1)
    return words[pick].reshape(-1)[:257 * PIECE + PIECE + 1].tobytes()


@pytest.fixture(scope="module")
def text_token(engine, text):
    token = engine.resident_put(text)
    yield token
    engine.resident_free(token)


@pytest.mark.parametrize("effort", [1, 2])
@pytest.mark.parametrize("off,n", [(0, 1), (0, PIECE - 1), (0, PIECE), (0, PIECE + 1), (0, 257 * PIECE), (PIECE, 1),
                                   (PIECE, PIECE + 1), (PIECE, 257 * PIECE)])
def test_deflate_resident_equals_deflate(engine, text, text_token, off, n, effort):
    want = engine.bgzf_deflate(text[off:off + n], effort=effort)
    got = engine.bgzf_deflate_resident(text_token, off, n, effort=effort)
    assert len(got) == (n + PIECE - 1) // PIECE and got == want


def test_deflate_resident_refusals_and_profile(engine, text, text_token):
    for off, n in ((4, 16), (0, len(text) + 1), (256 * ((len(text) + 255) // 256), 1)):
        with pytest.raises(N.CCError) as ei:
            engine.bgzf_deflate_resident(text_token, off, n)
        assert ei.value.code == N.CC_E_INVALID
    with pytest.raises(N.CCError) as ei:
        engine.bgzf_deflate_resident(1 << 40, 0, 16)
    assert ei.value.code == N.CC_E_INVALID and "unknown id" in str(ei.value)
    engine.set_profiling(True)
    try:
        engine.kernel_times()
        engine.bgzf_deflate_resident(text_token, 0, 3 * PIECE)
        times = engine.kernel_times()
    finally:
        engine.set_profiling(False)
    assert times["bgzf_deflate"][1] == 1 and times.get("bgzf_upload", (0, 0))[1] == 0


# ---------------------------------------------------------------- the writer
@pytest.fixture(scope="module")
def source():
    return Bam(INPUT)


def _raw_specs(n, step=1):
    sp = make_specs(len(range(0, n, step)))
    sp["kind"] = N.OUT_RAW
    sp["src_rec"] = np.arange(0, n, step)
    return sp


def _files(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}


def _wired(engine, resident):
    was = (engine.device_assemble(True), engine.device_bgzf(True), engine.device_out_resident(resident))
    assert engine.out_resident_device == bool(resident)
    return was


def _unwire(engine, was):
    engine.device_out_resident(was[2])
    engine.device_bgzf(was[1])
    engine.device_assemble(was[0])


def _write_all(engine, source, d, resident):
    """The fused write without and with a kept handle, the asynchronous one, and the MemorySink's."""
    d.mkdir()
    sp = _raw_specs(source.n)
    kept = {}
    was = _wired(engine, resident)
    try:
        before = engine.resident_count()
        for tag, keep, asy in (("plain", False, False), ("keep", True, False), ("async", False, True)):
            p = str(d / (tag + ".bam"))
            sink = Sink(fused=[p], keep=[p] if keep else [], async_writes=asy)
            engine.set_profiling(True)
            engine.kernel_times()
            out = write_bam(p, source, Interner(), sp, [source], level=1, sink=sink)
            flush_writes()
            times = engine.kernel_times()
            engine.set_profiling(False)
            if keep:
                b = sink.take(out)
                kept[tag] = b.pack(np.arange(b.n, dtype=np.int64)).tobytes()
                b.close()
            elif resident:
                assert "asm_download" not in times and times.get("bgzf_upload", (0, 0))[1] == 0, times
                assert times["index_fields"][1] == 1 and times["bgzf_deflate"][1] >= 1
            else:
                assert "asm_download" in times and times["bgzf_upload"][1] >= 1
            assert engine.resident_count() == before
        p = str(d / "memory.bam")
        sink = MemorySink(fused=[p])
        out = write_bam(p, source, Interner(), sp, [source], level=1, sink=sink)
        b = sink.take(out)
        kept["memory"] = b.pack(np.arange(b.n, dtype=np.int64)).tobytes()
        b.close()
        assert engine.resident_count() == before
    finally:
        engine.set_profiling(False)
        _unwire(engine, was)
    return _files(d), kept


def test_writer_files_are_the_same_with_the_stream_resident(engine, source, tmp_path):
    off = _write_all(engine, source, tmp_path / "off", False)
    on = _write_all(engine, source, tmp_path / "on", True)
    assert sorted(on[0]) == sorted(off[0]) and len(on[0]) == 6   # three files and their indexes
    for f in on[0]:
        assert on[0][f] == off[0][f], f
    assert on[1] == off[1] and sorted(on[1]) == ["keep", "memory"]
    assert not engine.out_resident_device


def test_option_without_its_two_hooks_wires_nothing(engine):
    was = engine.device_out_resident(True)
    try:
        assert not engine.out_resident_device
        engine.device_assemble(True)
        assert not engine.out_resident_device
        engine.device_bgzf(True)
        assert engine.out_resident_device
        engine.device_assemble(False)
        assert not engine.out_resident_device
    finally:
        engine.device_bgzf(False)
        engine.device_assemble(False)
        engine.device_out_resident(was)


def test_pin_source_uploads_once(engine, source, tmp_path):
    def three(d, pin, fail=False):
        d.mkdir()
        engine.set_profiling(True)
        engine.kernel_times()
        with (engine.pin_source(source) if pin else _Null()):
            for k in range(3):
                p = str(d / ("w%d.bam" % k))
                write_bam(p, source, Interner(), _raw_specs(source.n, k + 2), [source], level=1, sink=Sink(fused=[p]))
            if fail:
                raise RuntimeError("a write raised")
        times = engine.kernel_times()
        engine.set_profiling(False)
        return _files(d), times
    was = _wired(engine, True)
    try:
        before = engine.resident_count()
        plain, t0 = three(tmp_path / "plain", False)
        pinned, t1 = three(tmp_path / "pinned", True)
        assert t0["asm_stream_upload"][1] == 3 and "resident_put" not in t0
        assert "asm_stream_upload" not in t1 and t1["resident_put"][1] == 1
        assert pinned == plain and len(plain) == 6
        assert engine.resident_count() == before
        with pytest.raises(RuntimeError):
            three(tmp_path / "raised", True, fail=True)
        assert engine.resident_count() == before
        tok, base = N.C.c_int64(0), N.C.c_uint64(0)
        assert N.io().ccio_bam_resident(source.h, N.C.byref(tok), N.C.byref(base)) == 0
    finally:
        engine.set_profiling(False)
        _unwire(engine, was)


class _Null(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def test_golden_basic_pipeline_is_the_same_with_the_stream_resident(engine, tmp_path):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, "basic")
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    if kw.get("bedfile", "False") != "False":
        kw["bedfile"] = os.path.join(d, kw["bedfile"])
    kw.update(assemble="device", bgzf="device", names="device")

    def run(tag, **more):
        (tmp_path / tag).mkdir()
        shutil.copy(os.path.join(d, "input.bam"), str(tmp_path / tag / "sample.bam"))
        before = engine.resident_count()
        consensus_pipeline(str(tmp_path / tag / "sample.bam"), str(tmp_path / tag), engine=engine, **dict(kw, **more))
        assert engine.resident_count() == before and not engine.out_resident_device
        out = {}
        for root, _, files in os.walk(str(tmp_path / tag)):
            for f in files:
                if f.endswith(".bam") or f.endswith(".bai"):
                    out[os.path.relpath(os.path.join(root, f), str(tmp_path / tag))] = open(os.path.join(root, f), "rb").read()
        return out
    off = run("off")
    on = run("on", out_resident="device")
    assert sorted(on) == sorted(off) and any(f.endswith(".bai") for f in on)
    for f in on:
        assert on[f] == off[f], f
