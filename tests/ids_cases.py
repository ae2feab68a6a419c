"""Hand-built BAM records for the device interner (csrc/intern_core.h, ccio_intern_keys,
ccio_intern_first, cc_table_ids), and an independent restatement of its three rules: what a record's
barcode, cigar string and RG value are, which record flags it sets, and which records are refused.
Everything here is computed from the record's bytes with struct and bytes methods, never by the code
under test.  The records are built with tests/unpack_cases.py's Rec."""
import struct

import numpy as np

import unpack_cases as UC

RF_BAD_SPACER, RF_QUAL_MISSING, RF_RG_UNSUPPORTED = 1, 2, 4
CIG_OPS = "MIDNSHP=XB"
FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


class Keys(object):
    """What one record gives: refuse, or per table the key's (offset in the record, length) or None,
    the interned strings (bc, cigar, rg; None: id -1) and the string-derived flags."""

    def __init__(self):
        self.refuse = False
        self.span = [None, None, None]   # barcode, cigar, RG
        self.bc = self.rg = None
        self.cigar = "None"
        self.flags = 0
        self.qual_missing = 0


def keys_of(raw, mode, delim):
    """raw: one record, block_size first, exactly its bytes (a cut record is refused)."""
    k = Keys()
    k.refuse = True
    if len(raw) < 4:
        return k
    bs, = struct.unpack_from("<i", raw, 0)
    if bs < 32 or 4 + bs > len(raw):
        return k
    lqn, ncig, lseq = raw[12], struct.unpack_from("<H", raw, 16)[0], struct.unpack_from("<i", raw, 20)[0]
    if lseq < 0 or 32 + lqn + 4 * ncig + (lseq + 1) // 2 + lseq > bs:
        return k
    k.refuse = False
    end = 4 + bs
    cig_off = 36 + lqn
    qual_off = cig_off + 4 * ncig + (lseq + 1) // 2
    aux_off = qual_off + lseq
    k.qual_missing = RF_QUAL_MISSING if lseq == 0 or raw[qual_off] == 0xff else 0
    name = raw[36:36 + lqn].split(b"\x00")[0]
    # cigar: the key is the raw bytes, the string prints op codes of 10 and more as M
    k.span[1] = (cig_off, 4 * ncig)
    if ncig:
        vals = struct.unpack_from("<%dI" % ncig, raw, cig_off)
        k.cigar = "".join("%d%s" % (v >> 4, CIG_OPS[v & 15] if (v & 15) < 10 else "M") for v in vals)
    # barcode
    if mode == 0:
        d0 = name.find(delim) if delim else -1
        if d0 < 0:
            k.flags |= RF_BAD_SPACER
        else:
            st = d0 + len(delim)
            d1 = name.find(delim, st)
            k.bc = name[st:len(name) if d1 < 0 else d1]
            k.span[0] = (36 + st, len(k.bc))
    else:
        k.bc = name.split(b"_")[0]
        k.span[0] = (36, len(k.bc))
    # RG: every aux value must lie whole inside the record, else the record is refused
    p, bad = aux_off, False
    while p + 3 <= end:
        tag, ty = raw[p:p + 2], raw[p + 2:p + 3]
        p += 3
        if ty in FIXED:
            if p + FIXED[ty] > end:
                k.refuse = True
                return k
            if tag == b"RG":
                if ty == b"A" and not bad:
                    k.rg, k.span[2] = raw[p:p + 1], (p, 1)
                else:
                    k.flags |= RF_RG_UNSUPPORTED
                return k
            p += FIXED[ty]
        elif ty in (b"Z", b"H"):
            q = raw.find(b"\x00", p, end)
            q = end if q < 0 else q
            if tag == b"RG":
                if ty == b"Z" and not bad:
                    k.rg, k.span[2] = raw[p:q], (p, q - p)
                else:
                    k.flags |= RF_RG_UNSUPPORTED
                return k
            p = q + 1
        elif ty == b"B":
            if p + 5 > end:
                k.refuse = True
                return k
            sub, cnt = raw[p:p + 1], struct.unpack_from("<i", raw, p + 1)[0]
            es = 1 if sub in (b"c", b"C") else 2 if sub in (b"s", b"S") else 4
            if cnt < 0 or p + 5 + es * cnt > end:
                k.refuse = True
                return k
            if tag == b"RG":
                bad = True
            p += 5 + es * cnt
        else:
            bad = True
            break
    if bad:
        k.flags |= RF_RG_UNSUPPORTED
    return k


def rec(name, cigar=((0, 10),), aux=b"", lseq=10, i=0, **kw):
    """A record with the given read name (bytes, without the NUL), cigar [(op, len)] and aux bytes."""
    rng = np.random.default_rng(1000 + i)
    codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), lseq)
    quals = rng.integers(0, 60, lseq).astype(np.uint8)
    kw.setdefault("pos", 1000 + i)
    return UC.Rec(name + b"\x00", codes, quals, list(cigar), aux=aux, **kw)


I32 = lambda v: struct.pack("<i", v)
# every aux type in front of RG
EVERY_TYPE = (b"XAAq" + b"Xcc\xff" + b"XCC\x07" + b"Xss\x01\x02" + b"XSS\x01\x02" + b"Xii" + I32(-5) + b"XII" + I32(5) +
              b"Xff" + struct.pack("<f", 1.5) + b"XZZtext\x00" + b"XHH1AE3\x00" + b"XBBc" + I32(3) + b"\x01\x02\x03" +
              b"XbBS" + I32(2) + b"\x01\x00\x02\x00" + b"XdBf" + I32(1) + struct.pack("<f", 2.0) + b"XeBi" + I32(0))
# name -> aux: the forms the walk accepts (a key, or id -1 with or without the flag)
RG_FORMS = {
    "none": b"",
    "Z": b"RGZgrp1\x00",
    "Z_empty": b"RGZ\x00",
    "A": b"RGAx",
    "H": b"RGH1AE3\x00",
    "i": b"RGi" + I32(7),
    "c": b"RGc\x01",
    "S": b"RGS\x01\x02",
    "f": b"RGf" + struct.pack("<f", 1.0),
    "B_then_Z": b"RGBc" + I32(2) + b"\x01\x02" + b"RGZgrp1\x00",
    "B_only": b"RGBS" + I32(1) + b"\x01\x02",
    "after_every_type": EVERY_TYPE + b"RGZgrp2\x00",
    "every_type_no_rg": EVERY_TYPE,
    "Z_no_nul": b"NMC\x03RGZgrp3",
    "Z_no_nul_empty": b"RGZ",
    "other_Z_no_nul": b"XSZabc",
    "unknown_before_rg": b"XQ?abRGZgrp1\x00",
    "unknown_after_rg_b": b"RGBc" + I32(0) + b"XQ?",
    "second_rg_ignored": b"RGZgrp1\x00RGZgrp9\x00",
    "two_bytes_left": b"NMC\x03RG",
    "grp1_again": b"XSZabc\x00RGZgrp1\x00",
}
# the forms that are refused: the host's walk would read past the record's end
RG_MALFORMED = {
    "B_header_cut": b"NMC\x03XBBc" + b"\x01\x00",
    "B_header_cut_at_sub": b"XBB",
    "B_negative": b"XBBc" + I32(-1) + b"RGZgrp1\x00",
    "B_overrun": b"XBBS" + I32(1000) + b"\x01\x00",
    "B_overrun_by_one": b"XBBi" + I32(1) + b"\x01\x02\x03",
    "fixed_at_last_byte": b"NMC\x03XIi\x01",
    "fixed_no_value": b"NMC",
    "rg_A_no_value": b"RGA",
    "rg_B_cut": b"RGBc" + I32(5) + b"\x01",
}

DELIM16 = b"<=16-byte-delim>"
assert len(DELIM16) == 16
# (read name, delimiter): mode 0
BARCODE_MODE0 = [
    (b"read1|AC.GT", b"|"), (b"read1", b"|"), (b"|ACGT", b"|"), (b"read1|", b"|"), (b"r||x", b"|"),
    (b"r|AC|GT|x", b"|"), (b"a|||b", b"||"), (b"a||b||c", b"||"), (b"|", b"|"), (b"", b"|"), (b"ab", b"abc"),
    (b"x" + DELIM16 + b"AC.GT", DELIM16), (b"x" + DELIM16[:15], DELIM16), (b"r#+#AC#+#x", b"#+#"),
    (b"r" * 200 + b"|" + b"A" * 53, b"|"), (b"q|AC.GT", b"|"),
]
# read names: mode 1
BARCODE_MODE1 = [b"AC.GT_chr1_100", b"ACGT", b"_x", b"x_", b"a", b"_", b"b" * 254, b"c" * 100 + b"_" + b"d" * 153,
                 b"AC.GT_other"]
# cigars: none, one op, every op code 0..15, and pairs of raw cigars that print one string
CIGARS = [(), ((0, 10),), tuple((op, 1 + op) for op in range(16)), ((10, 10),), ((15, 10),), ((0, 10), (4, 2)),
          ((12, 10), (4, 2)), ((0, 11),), ((0, 0),)]


def aux_records(forms=None):
    forms = RG_FORMS if forms is None else forms
    return [rec(b"q%d|AC.GT" % i, aux=a, i=i) for i, a in enumerate(forms.values())]


def cigar_records():
    return [rec(b"q|AC.GT", cigar=c, i=i) for i, c in enumerate(CIGARS)]


def name_records(mode):
    names = [n for n, _ in BARCODE_MODE0] if mode == 0 else BARCODE_MODE1
    return [rec(n, aux=b"RGZg\x00", i=i) for i, n in enumerate(names)]


def keyed(n, key_of, pad=None):
    """n records whose barcode, cigar length and RG all follow key_of(i) (an int): equal ints, equal keys."""
    out = []
    for i in range(n):
        k = int(key_of(i))
        out.append(rec(b"r%d|B%dx" % (i, k), cigar=((0, 1 + k),), aux=b"RGZg%d\x00" % k, lseq=4 + (i % 13 if pad is None else pad),
                       i=i))
    return out


def expected_ids(recs, mode, delim, seen=None):
    """The three shared-id columns, rflags and the interner's tables after a decode of recs in order:
    a new string takes the next id at its first occurrence.  seen: the tables so far ([bc, cigar, rg]
    lists), extended in place."""
    seen = seen if seen is not None else [[], [], []]
    cols = [np.zeros(len(recs), np.int32) for _ in range(3)]
    rf = np.zeros(len(recs), np.uint8)
    for i, r in enumerate(recs):
        k = keys_of(r.raw, mode, delim)
        assert not k.refuse
        for t, s in enumerate((k.bc, k.cigar.encode(), k.rg)):
            if s is None:
                cols[t][i] = -1
                continue
            if s not in seen[t]:
                seen[t].append(s)
            cols[t][i] = seen[t].index(s)
        rf[i] = k.flags | k.qual_missing
    return cols, rf, seen
