"""The device interner's host side without a GPU.  ccio_intern_keys runs the shared key finders
(csrc/intern_core.h: what k_ids_keys compiles) over files of tests/ids_cases.py's records: the key
bytes they point at must print the strings ccio_bam_decode_ids interned (ccio_interner_blob), with its
flags, in modes 0 and 1.  ccio_intern_first, fed local ids computed here with numpy, must reproduce
decode_ids' three id columns for a fresh interner and for one another file has filled."""
import os

import numpy as np
import pytest

import ids_cases as IC
import unpack_cases as UC
from consensuscruncher_amd.engine import Bam, Interner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "consensuscruncher_amd", "csrc")


def _strings(it, kind):
    blob, off = it.blob(kind)
    b = blob.tobytes()
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _all_records(mode):
    return IC.aux_records() + IC.cigar_records() + IC.name_records(mode) + UC.shapes()


def _cigar_text(key):
    vals = np.frombuffer(key, "<u4")
    return ("".join("%d%s" % (v >> 4, IC.CIG_OPS[v & 15] if (v & 15) < 10 else "M") for v in vals) or "None").encode()


@pytest.mark.parametrize("mode,delim", [(0, "|"), (1, "|"), (0, "||"), (0, IC.DELIM16.decode())])
def test_keys_are_the_strings_decode_ids_interned(tmp_path, mode, delim):
    recs = _all_records(mode)
    if delim != "|":
        recs = [IC.rec(n, aux=b"RGAx", i=i) for i, (n, _) in enumerate(IC.BARCODE_MODE0)] + recs[:20]
    bam = Bam(UC.write_bam(str(tmp_path / "k.bam"), recs))
    it = Interner()
    rec, stream, rec_off = bam.decode_ids(it, mode, delim)
    stream = stream.tobytes()
    off, ln, none, flags, refuse = bam.intern_keys(mode, delim)
    assert not refuse.any()
    assert np.array_equal(flags, rec.rflags[:rec.n] & 5)
    tables = [_strings(it, k) for k in range(3)]
    for t, ids in enumerate((rec.bc_id, rec.cigar_id, rec.rg_id)):
        for r in range(rec.n):
            if none[t, r]:
                assert ids[r] == -1, (t, r)
                continue
            at = int(rec_off[r]) + int(off[t, r])
            key = stream[at:at + int(ln[t, r])]
            assert int(off[t, r]) + int(ln[t, r]) <= 4 + recs[r].fields["bs"]
            assert tables[t][ids[r]] == (_cigar_text(key) if t == 1 else key), (t, r)
    # and the restatement agrees with both
    cols, rf, seen = IC.expected_ids(recs, mode, delim.encode())
    assert [np.array_equal(c, x[:rec.n]) for c, x in zip(cols, (rec.bc_id, rec.cigar_id, rec.rg_id))] == [True] * 3
    assert np.array_equal(rf, rec.rflags[:rec.n]) and seen == tables
    bam.close()


def test_malformed_aux_is_refused_and_a_long_delimiter_is_an_error(tmp_path):
    recs = IC.aux_records(IC.RG_MALFORMED)
    bam = Bam(UC.write_bam(str(tmp_path / "bad.bam"), recs + IC.aux_records()))
    *_, refuse = bam.intern_keys(0, "|")
    assert refuse.tolist() == [1] * len(recs) + [0] * len(IC.RG_FORMS)
    with pytest.raises(IOError):
        bam.intern_keys(0, "x" * 17)
    bam.close()


def _locals(recs, mode, delim):
    """Per table: local ids in order of first occurrence and the first records, from np.unique over
    the restated keys (the cigar by its raw bytes, as the device keys it)."""
    local, first = [], []
    for t in range(3):
        keys = []
        for r in recs:
            k = IC.keys_of(r.raw, mode, delim)
            s = k.span[t]
            keys.append(None if s is None else r.raw[s[0]:s[0] + s[1]])
        have = np.array([k is not None for k in keys])
        names = sorted({k for k in keys if k is not None})
        code = np.array([names.index(k) if k is not None else -1 for k in keys], np.int64)
        loc = np.full(len(recs), -1, np.int32)
        if have.any():
            _, idx = np.unique(code[have], return_index=True)
            at = np.flatnonzero(have)[idx]          # each distinct key's first record
            order = np.argsort(at)
            rank = np.empty(len(order), np.int32)
            rank[order] = np.arange(len(order), dtype=np.int32)
            loc[have] = rank[code[have]]
            first.append(np.sort(at).astype(np.int32))
        else:
            first.append(np.zeros(0, np.int32))
        local.append(loc)
    return local, first


@pytest.mark.parametrize("nthreads", [1, 16])
@pytest.mark.parametrize("mode", [0, 1])
def test_intern_first_reproduces_decode_ids(tmp_path, mode, nthreads):
    other = IC.keyed(300, lambda i: (i * 7) % 40) + IC.cigar_records()[:5] + IC.aux_records()[:8]
    recs = IC.keyed(700, lambda i: 20 + (i * 11) % 40 if i % 3 else 0) + _all_records(mode)
    pa, pb = UC.write_bam(str(tmp_path / "a.bam"), other), UC.write_bam(str(tmp_path / "b.bam"), recs)
    for filled in (False, True):
        it_h, it_d = Interner(), Interner()
        if filled:   # half of b's keyed strings are in a
            for it in (it_h, it_d):
                a = Bam(pa)
                a.decode_ids(it, mode, "|", nthreads)
                a.close()
        bh, bd = Bam(pb), Bam(pb)
        want, _, _ = bh.decode_ids(it_h, mode, "|", nthreads)
        local, first = _locals(recs, mode, b"|")
        bc, cig, rg = bd.intern_first(it_d, mode, "|", local, first, nthreads)
        n = want.n
        assert np.array_equal(bc, want.bc_id[:n]) and np.array_equal(cig, want.cigar_id[:n])
        assert np.array_equal(rg, want.rg_id[:n])
        assert [_strings(it_d, k) for k in range(3)] == [_strings(it_h, k) for k in range(3)]
        if filled:
            assert 0 < len(set(bc.tolist()) & set(range(40))) and bc.max() >= 40, "old and new strings both"
        # decode_cols: decode_ids' columns, stream and offsets without the ids
        cols, stream, off = bd.decode_cols(nthreads)
        w2, s2, o2 = bh.decode_ids(it_h, mode, "|", nthreads)
        for name in ("tid", "pos", "mtid", "mpos", "tlen", "flag", "mapq", "lseq", "qlen", "qn_len"):
            assert np.array_equal(getattr(cols, name), getattr(w2, name)), name
        assert np.array_equal(cols.rflags, w2.rflags & 2) and cols.max_len == w2.max_len
        assert stream.tobytes() == s2.tobytes() and np.array_equal(off, o2)
        bh.close()
        bd.close()


def test_intern_first_errors(tmp_path):
    recs = IC.aux_records()
    bam = Bam(UC.write_bam(str(tmp_path / "e.bam"), recs))
    local, first = _locals(recs, 0, b"|")
    it = Interner()
    no_rg = [i for i, r in enumerate(recs) if IC.keys_of(r.raw, 0, b"|").rg is None][0]
    bad_first = [first[0], first[1], np.concatenate([first[2], [no_rg]]).astype(np.int32)]
    with pytest.raises(IOError, match="no RG"):
        bam.intern_first(it, 0, "|", local, bad_first)
    outside = [np.array([len(recs)], np.int32)] + first[1:]
    with pytest.raises(IOError, match="outside the handle"):
        bam.intern_first(it, 0, "|", local, outside)
    big = [local[0].copy(), local[1], local[2]]
    big[0][3] = len(first[0])
    with pytest.raises(IOError, match="local barcode id"):
        bam.intern_first(it, 0, "|", big, first)
    bam.close()


def test_core_is_what_the_kernel_includes():
    inc = open(os.path.join(CSRC, "table_ids.hip.inc")).read()
    assert '#include "intern_core.h"' in inc and os.path.exists(os.path.join(CSRC, "intern_core.h"))
    for fn in ("barcode_key", "cigar_key", "rg_key", "hash_bytes", "Delim", "Key"):
        assert "itn::" + fn in inc, fn
    assert "upk::parse" in inc
    engine = open(os.path.join(CSRC, "cc_engine.hip")).read()
    assert '#include "table_ids.hip.inc"' in engine
    ccio = open(os.path.join(CSRC, "ccio.cpp")).read()
    assert '#include "intern_core.h"' in ccio
    for fn in ("barcode_key", "cigar_key", "rg_key"):
        assert "itn::" + fn in ccio, fn
