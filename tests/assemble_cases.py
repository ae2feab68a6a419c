"""Inputs for the output-record assembler's tests (tests/test_assemble_core_host.py on the host,
tests/test_gpu_assemble.py on the device): source records, cc_out_spec arrays, names, consensus
arrays and RG values at the smallest shapes where assemble_core.h's layout, the copy kernel's
head / line / tail split, the sort's digit range and the offset slices can go wrong.  Every expected
byte comes from libccio's host writer (ccio_write_bam_ex with no hook set); nothing is restated here."""
import os
import struct

import numpy as np

import unpack_cases as UC
from consensuscruncher_amd import native as N

LS = (0, 1, 2, 15, 16, 17, 150, 151, 1025)
NAME_LENS = (1, 7, 8, 9, 254)          # and name_id = -1: length 0
RG_VALUES = (b"", b"g", b"seventeen_bytes_rg")
# headers whose encoded size is 0, 1 and 15 mod 16 (see header_bytes; asserted by the tests)
REFS = [("chr1", 600000000), ("chr2", 1000000), ("chr3", 1000000)]


def header_text(pad):
    return "@HD\tVN:1.6\tSO:unsorted\n@CO\t" + "x" * pad + "\n"


def header_bytes(pad):
    t = header_text(pad).encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(REFS))
    for name, ln in REFS:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def header_pad(residue):
    """The @CO padding that gives an encoded header of size `residue` mod 16."""
    return (residue - len(header_bytes(0))) % 16


class Case(object):
    def __init__(self, name, sources, specs, names=(), cons_seq=None, cons_qual=None, rgs=RG_VALUES, pad=0):
        self.name, self.sources, self.specs, self.pad = name, sources, specs, pad
        self.names = list(names)
        self.name_off = np.cumsum([0] + [len(x) for x in self.names]).astype(np.int64)
        self.names_blob = np.frombuffer(b"".join(self.names) + b"\0", np.uint8)
        self.cons_seq = np.zeros(1, np.uint8) if cons_seq is None else cons_seq
        self.cons_qual = np.zeros(1, np.uint8) if cons_qual is None else cons_qual
        self.rgs = list(rgs)

    def write_sources(self, d):
        """The sources as BAM files under d (header of this case's padding); their paths."""
        import pysam
        paths = []
        for f, recs in enumerate(self.sources):
            p = os.path.join(str(d), "%s_src%d.bam" % (self.name, f))
            pysam.write_bam_file(p, pysam.AlignmentHeader(header_text(self.pad), REFS), [r.raw for r in recs], level=1)
            paths.append(p)
        return paths


def _rec(rng, i, L, lqn, cig, aux=b"", **kw):
    codes = rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), L)
    quals = rng.integers(0, 94, L).astype(np.uint8)
    return UC.Rec(UC.qname(lqn, i), codes, quals, cig, aux=aux, **kw)


def _aux(k):
    return b"" if k == 0 else b"XXZ" + b"a" * (k - 1) + b"\0"


def sources(seed=3):
    """Two sources.  The first: every L with n_cigar 0, 1, 5 and the name lengths, aux tails that put
    the record starts on every alignment mod 16, then the reg2bin edges and the sort's ties."""
    rng = np.random.default_rng(seed)
    a = []
    cigs = ([], [(0, 10)], [(4, 2), (0, 5), (2, 3), (1, 1), (0, 4)])
    lqns = (1, 2, 8, 9, 10, 255)
    for k, L in enumerate(LS):
        a.append(_rec(rng, len(a), L, lqns[k % len(lqns)], cigs[k % 3], aux=_aux(k), pos=3000 + 40 * k, flag=(99, 147)[k % 2]))
    for k in range(16):   # sizes 0..15 mod 16 in a row: the starts that follow fall on every alignment
        a.append(_rec(rng, len(a), 20, 12, cigs[1], aux=_aux(k), pos=5000 + k))
    # reg2bin: pos -1, rlen 0 (no cigar; only query ops), spans ending at and one past each level's edge
    a.append(_rec(rng, len(a), 8, 9, cigs[1], tid=-1, pos=-1, mtid=-1, mpos=-1, flag=77))
    a.append(_rec(rng, len(a), 8, 9, [(4, 3), (1, 5)], pos=7000))
    a.append(_rec(rng, len(a), 8, 9, [], pos=(1 << 14) - 1))
    for sh in (14, 17, 20, 23, 26):
        for over in (0, 1):
            a.append(_rec(rng, len(a), 8, 9, [(0, 100 + over)], pos=(1 << sh) - 100))
    a.append(_rec(rng, len(a), 8, 9, [(0, 50)], pos=(1 << 29) - 50))
    # forward and reverse at one position, twice (ties in spec order)
    for fl in (99, 147, 163, 83):
        a.append(_rec(rng, len(a), 30, 14, cigs[1], pos=9000, flag=fl))
    # the smallest records there are: 37 bytes (empty name, no cigar, no bases), three lines for four of them
    for k in range(4):
        a.append(_rec(rng, len(a), 0, 1, [], pos=9500))
    b = [_rec(rng, 100 + k, (30, 17, 0)[k % 3], 14 - k, cigs[(k + 1) % 3], pos=9000 if k < 3 else 5003, tid=0 if k < 5 else 2,
              flag=(99, 147)[k % 2], aux=_aux(3 * k)) for k in range(6)]
    return [a, b]


def _cons(rng, nbytes):
    return rng.integers(0, 256, nbytes // 2 + 8).astype(np.uint8), rng.integers(0, 94, nbytes + 8).astype(np.uint8)


def main_case(pad=0, seed=11):
    """Every kind over every template of both sources, names of every length, every L, every RG."""
    rng = np.random.default_rng(seed)
    src = sources()
    names = [bytes(rng.integers(65, 91, ln).astype(np.uint8)) for ln in NAME_LENS]
    cs, cq = _cons(rng, 4096)
    rows = []
    k = 0
    for f, recs in enumerate(src):
        for r in range(len(recs)):
            for kind in (N.OUT_RAW, N.OUT_RENAME, N.OUT_NEW):
                L = LS[k % len(LS)]
                rows.append(dict(kind=kind, src_file=f, src_rec=r, name_id=(k % (len(names) + 1)) - 1, flag=(0, 16)[k % 2] | 1,
                                 mapq=k % 61, tlen=(-1) ** k * k, rg_id=(k % (len(RG_VALUES) + 1)) - 1,
                                 cons_off=(2 * k * 7) % (4096 - 1025) + (1 if k % 29 == 5 else 0), cons_len=L))
                k += 1
    for j in range(16):   # new records 3 bytes apart: every size mod 16, whatever the rows above give
        rows.append(dict(kind=N.OUT_NEW, src_file=0, src_rec=9, name_id=-1, flag=99, mapq=3, tlen=0, rg_id=-1, cons_off=32 * j,
                         cons_len=2 * j))
    return Case("main%d" % pad, src, _specs(rows), names, cs, cq, pad=pad)


def _specs(rows):
    sp = np.zeros(len(rows), N.OUT_SPEC_DTYPE)
    for i, r in enumerate(rows):
        for key, v in r.items():
            sp[key][i] = v
    return sp


def empty_case(pad=0):
    return Case("empty%d" % pad, sources(), _specs([]), pad=pad)


def one_case(kind):
    rng = np.random.default_rng(5)
    cs, cq = _cons(rng, 64)
    return Case("one%d" % kind, sources(), _specs([dict(kind=kind, src_file=0, src_rec=3, name_id=0, flag=83, mapq=9, tlen=-4,
                                                        rg_id=2, cons_off=6, cons_len=17)]), [b"n"], cs, cq, pad=header_pad(15))


def lowdigit_case():
    """Keys that use only the sort's lowest digit (tid 0, pos < 127), in descending order."""
    rng = np.random.default_rng(6)
    recs = [_rec(rng, k, 5, 9, [(0, 5)], pos=120 - 3 * (k // 2), flag=(99, 147)[k % 2]) for k in range(40)]
    return Case("lowdigit", [recs], _specs([dict(kind=N.OUT_RAW, src_file=0, src_rec=k, name_id=-1, rg_id=-1) for k in range(40)]))


def toptid_case():
    """Keys that use the top tid bits (no index can be built over such a file: sorted, not indexed)."""
    rng = np.random.default_rng(7)
    tids = (0x40000000, 3, -1, 0x7fffff00, 0, 0x40000000)
    recs = [_rec(rng, k, 5, 9, [(0, 5)], tid=t, pos=10 + k) for k, t in enumerate(tids)]
    return Case("toptid", [recs], _specs([dict(kind=k % 2, src_file=0, src_rec=k, name_id=-1, rg_id=-1) for k in range(6)]))


SLICE_REC = 4 + 32 + 10 + 4 + 5 + 10   # the slice case's record size


def slice_case():
    """40 equal records (SLICE_REC bytes), shuffled positions: CC_ASM_SLICE_BYTES = 14 * SLICE_REC ends
    slices exactly on a record's last byte, 14 * SLICE_REC - 1 one byte short of it."""
    rng = np.random.default_rng(8)
    recs = [_rec(rng, k, 10, 10, [(0, 10)], pos=int(p)) for k, p in enumerate(rng.permutation(40) * 17)]
    assert all(len(r.raw) == SLICE_REC for r in recs)
    return Case("slices", [recs], _specs([dict(kind=N.OUT_RAW, src_file=0, src_rec=k, name_id=-1, rg_id=-1) for k in range(40)]))


def refusals():
    """(label, case, index of the refused spec, word of the error message): each of assemble_core.h's refusals,
    the bad spec behind good ones."""
    rng = np.random.default_rng(9)
    src = sources()
    cs, cq = _cons(rng, 64)
    good = dict(kind=N.OUT_NEW, src_file=0, src_rec=1, name_id=0, flag=99, mapq=1, tlen=1, rg_id=0, cons_off=0, cons_len=20)
    out = []
    for label, patch, word in (("src_file", dict(src_file=2), "src_file"), ("src_file_neg", dict(src_file=-1), "src_file"),
                               ("src_rec", dict(src_rec=len(src[0])), "src_rec"), ("src_rec_neg", dict(src_rec=-1), "src_rec"),
                               ("name_id", dict(name_id=2), "name_id"), ("cons_range", dict(cons_off=60, cons_len=20), "cons_off"),
                               ("cons_nibbles", dict(cons_off=6, cons_len=20), "cons_off"),
                               ("cons_neg", dict(cons_len=-1), "cons_off"), ("rg_id", dict(rg_id=len(RG_VALUES)), "rg_id"),
                               ("long_name", dict(name_id=1), "254")):
        rows = [dict(good), dict(good, kind=N.OUT_RAW), dict(good, **patch)]
        # (cons_nibbles: 12 nibble bytes hold the good rows' 10 but not bytes 3..13, while the qualities fit)
        out.append((label, Case("bad_" + label, src, _specs(rows), [b"ok", b"L" * 255],
                                cs[:12] if label == "cons_nibbles" else cs, cq), 2, word))
    # a template whose lengths do not fit its block_size: n_cigar raised in the raw record
    bad = list(src[0])
    r = bad[1]
    raw = bytearray(r.raw)
    raw[4 + 12:4 + 14] = struct.pack("<H", 0x4000)
    r2 = UC.Rec.__new__(UC.Rec)
    r2.raw = bytes(raw)
    bad[1] = r2
    out.append(("template", Case("bad_template", [bad, src[1]], _specs([dict(good, src_rec=0), dict(good)]), [b"ok"], cs, cq), 1,
                "block_size"))
    return out
