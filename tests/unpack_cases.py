"""Hand-built BAM record streams for the record unpacker (csrc/unpack_core.h, ccio_bam_decode_ids,
cc_table_unpack), with what each record must parse to, computed here from the values the record was
built from (struct, numpy), never by the code under test.

The shapes are the smallest at which the unpacker can still go wrong: l_seq at every payload slot
step, the odd nibble tail and beyond one pass of the copy kernel's 16-lane group; l_read_name from
the empty name to 255; record starts on every alignment mod 16; no cigar and every cigar op;
qual[0] == 0xff; no aux, RG:Z, RG:A, an integer RG, and other aux in front of RG."""
import struct

import numpy as np

LSEQS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 150, 255, 256, 257, 1024, 1025)
LQNS = (1, 2, 8, 9, 16, 17, 255)
M64 = (1 << 64) - 1
QUERY_OPS = (0, 1, 4, 7, 8)   # M I S = X consume the query (infer_query_length)
AUXES = (b"", b"RGZgrp1\x00", b"RGAx", b"RGi" + struct.pack("<i", 7), b"NMC\x03XSZabc\x00RGZgrp2\x00",
         b"XBBS" + struct.pack("<iHH", 2, 5, 6) + b"RGZgrp1\x00")


def qname(lqn, i, spacer=True):
    """A read name of l_read_name lqn (NUL included), with the barcode spacer when it fits."""
    if lqn <= 1:
        return b"\x00"
    tail = b"|AC.GT" if spacer and lqn - 1 >= 8 else b""
    head = ("r%d" % i).encode()
    body = (head + b"x" * 255)[:lqn - 1 - len(tail)] + tail
    assert len(body) == lqn - 1
    return body + b"\x00"


class Rec(object):
    """One record and what it must parse to."""

    def __init__(self, qn, codes, quals, cigar, tid=0, pos=1000, flag=99, mapq=60, mtid=0, mpos=1200, tlen=350, aux=b"",
                 bin_=4681):
        codes = np.asarray(codes, np.uint8)
        quals = np.asarray(quals, np.uint8)
        n = len(codes)
        assert len(quals) == n and qn.endswith(b"\x00") and len(qn) <= 255
        nib = np.zeros(2 * ((n + 1) // 2), np.uint8)
        nib[:n] = codes
        packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
        cig = b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar)
        body = struct.pack("<iiBBHHHiiii", tid, pos, len(qn), mapq, bin_, len(cigar), flag, n, mtid, mpos, tlen)
        body += qn + cig + packed + quals.tobytes() + aux
        self.raw = struct.pack("<i", len(body)) + body
        self.fields = dict(bs=len(body), tid=tid, pos=pos, l_read_name=len(qn), mapq=mapq, n_cigar=len(cigar), flag=flag,
                           lseq=n, mtid=mtid, mpos=mpos, tlen=tlen, qn_len=qn.index(b"\x00"),
                           qlen=sum(ln for op, ln in cigar if op in QUERY_OPS) if cigar else -1,
                           cig_off=36 + len(qn), seq_off=36 + len(qn) + len(cig),
                           qual_off=36 + len(qn) + len(cig) + len(packed),
                           aux_off=36 + len(qn) + len(cig) + len(packed) + n,
                           rflags=2 if n == 0 or quals[0] == 0xff else 0)
        # the slots: [qual | zeros to 16][nibbles | zeros to the 128-B multiple], [name | zeros to 8]
        qa, na = (n + 15) & ~15, (len(packed) + 15) & ~15
        pay = np.zeros((qa + na + 127) & ~127, np.uint8)
        pay[:n] = quals
        pay[qa:qa + len(packed)] = np.frombuffer(packed, np.uint8)
        self.pay = pay.tobytes()
        name = qn[:qn.index(b"\x00")]
        self.qn = name + b"\x00" * (((len(qn) + 7) & ~7) - len(name))
        self.rdig = rec_digest(body)


def _mix(x):
    x ^= x >> 31
    x = (x * 0x7fb5d329728ea185) & M64
    x ^= x >> 27
    x = (x * 0x81dadef4bc2dd44d) & M64
    return x ^ (x >> 33)


def rec_digest(body):
    """The record digest restated: 8-byte words of the record core, bin zeroed, the tail word tagged
    with its length."""
    bs = len(body)
    h = 0x9E3779B97F4A7C15 ^ bs
    i = 0
    while i + 8 <= bs:
        w = int.from_bytes(body[i:i + 8], "little")
        if i == 8:
            w &= ~(0xffff << 16) & M64
        h = (_mix(h ^ w) + 0x632BE59BD9B4E019) & M64
        i += 8
    w = int.from_bytes(body[i:], "little")
    if i == 8:
        w &= ~(0xffff << 16) & M64
    return _mix(h ^ w ^ ((bs - i) << 56))


def make(rng, i, lseq, lqn, cigar="M", aux=b"", qual_ff=False, **kw):
    codes = rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), lseq)
    quals = rng.integers(0, 94, lseq).astype(np.uint8)
    if qual_ff and lseq:
        quals[0] = 0xff
    if cigar == "M":
        cig = [(0, lseq)] if lseq else [(0, 1)]
    elif cigar == "none":
        cig = []
    else:   # every op, the query ops adding up to anything (the parser only sums them)
        cig = [(op, 1 + (i + op) % 5) for op in range(9)]
    return Rec(qname(lqn, i), codes, quals, cig, aux=aux, **kw)


def shapes(seed=7):
    """Every l_seq with every l_read_name once (126 records), then the cigar, quality, aux and
    position cases."""
    rng = np.random.default_rng(seed)
    out = []
    for a, lseq in enumerate(LSEQS):
        for b, lqn in enumerate(LQNS):
            k = len(out)
            out.append(make(rng, k, lseq, lqn, cigar=("M", "none", "all")[(a + b) % 3], aux=AUXES[k % len(AUXES)],
                            qual_ff=(k % 11 == 3), pos=1000 + 3 * k))
    for aux in AUXES:
        out.append(make(rng, len(out), 150, 20, aux=aux, pos=2000))
    out.append(make(rng, len(out), 40, 12, tid=-1, pos=-1, mtid=-1, mpos=-1, flag=77))
    out.append(make(rng, len(out), 40, 12, tid=2, pos=5, flag=147))
    return out


def many(n, seed, deep_at=None, sort=True):
    """n records of L around 150 with mixed name lengths; deep_at: a position 70 of them share (a deep
    position group); sort: in (tid, pos) order, else shuffled."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, 50 * max(n, 1) + 1, n))
    if deep_at is not None and n >= 70:
        pos[n // 3:n // 3 + 70] = pos[n // 3]
    if not sort:
        pos = rng.permutation(pos)
    lq = (9, 14, 17, 23, 30, 33)
    return [make(rng, i, int(rng.choice((149, 150, 151, 75))), lq[i % len(lq)] + (i * 7) % 5, aux=AUXES[i % 3],
                 tid=int(i * 3 // max(n, 1)) if sort else int(rng.integers(0, 3)), pos=int(pos[i])) for i in range(n)]


def stream_of(recs):
    """(stream bytes, record offsets)"""
    off = np.cumsum([0] + [len(r.raw) for r in recs])[:-1].astype(np.uint64) if recs else np.zeros(0, np.uint64)
    return b"".join(r.raw for r in recs), off


HEADER_TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:1000000\n@SQ\tSN:chr3\tLN:1000000\n"


def write_bam(path, recs):
    import pysam
    refs = [("chr1", 1000000), ("chr2", 1000000), ("chr3", 1000000)]
    pysam.write_bam_file(path, pysam.AlignmentHeader(HEADER_TEXT, refs), [r.raw for r in recs], level=1)
    return path
