"""Inputs for the consensus read-name formatter's tests (tests/test_name_core_host.py on the host,
tests/test_gpu_names.py on the device): packed csn fields with their barcode and cigar strings, and
SSCS-style qnames with (tag, partner) record pairs, at the smallest shapes where name_core.h's rules,
the SWAR scans, the write kernels' head / line / tail split and the offsets' scan can go wrong.
Every expected byte comes from libccio's ccio_format_csn_names / ccio_format_dcs_names; nothing is
restated here."""
import numpy as np

import unpack_cases as UC

# the name counts: around a wave, a block of the sizes kernel (256), and the scan's 4,096-element tile
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _width_edges(top):
    """0, then 9, 10, 99, 100, ... up to top: both sides of every decimal width."""
    out, p = [0], 10
    while p <= top:
        out += [p - 1, p]
        p *= 10
    return out + [top]


E32 = _width_edges(I32_MAX) + [-1, -9, -10, -99, -100, -999999999, -1000000000, I32_MIN]
EU32 = _width_edges(0xffffffff) + [0x7fffffff, 0x80000000]
E64 = [1, I64_MAX, -1, I64_MIN, -9, -10, -10 ** 18] + _width_edges(I64_MAX)
F7 = [0, 1, 2, 3, 4, 5, 6, 7, 0x7ffffffc, 0x7ffffffd, 0x7ffffffe, 0x7fffffff, -1, -2, -3, -4]
BARCODES = [b"", b"A", b"AC.GTAC", b"ACG.TACG", b"ACGT.ACGT", b"ACGTACG.TACGTAC", b"ACGTACGT.ACGTACG", b"ACGTACGT.ACGTACGT",
            b"ACGTACGTACGTACGT.ACGTACGTACGTACG"]
CIGARS = [b"150M", b"", b"5S145M", b"1M1I" * 75, b"None"]
assert [len(b) for b in BARCODES] == [0, 1, 7, 8, 9, 15, 16, 17, 32] and len(CIGARS[3]) == 300


class Csn(object):
    def __init__(self, name, f9, suf, refused=-1, bcs=BARCODES, cgs=CIGARS):
        self.name, self.refused, self.bcs, self.cgs = name, refused, list(bcs), list(cgs)
        self.f9 = np.ascontiguousarray(f9, np.int32).reshape(-1, 9)
        self.suf = np.ascontiguousarray(suf, np.int64)

    def interner(self):
        from consensuscruncher_amd.engine import Interner
        it = Interner()
        for kind, strs in ((0, self.bcs), (1, self.cgs)):
            for i, s in enumerate(strs):
                assert it.intern(kind, s.decode()) == i
        return it


def csn_rows(n, nbc=len(BARCODES), ncg=len(CIGARS)):
    """n names that walk every edge list at its own stride (from max(len) names on, every value of
    every list has been used)."""
    i = np.arange(n, dtype=np.int64)
    e32, eu, f7 = (np.array(x, dtype=np.int64) for x in (E32, EU32, F7))
    f9 = np.zeros((n, 9), np.int64)
    f9[:, 0] = i % nbc
    for k in range(4):
        f9[:, 1 + k] = e32[(i * (2 * k + 1) + k) % len(E32)]
    f9[:, 5] = i % ncg
    f9[:, 6] = (i // ncg) % ncg
    f9[:, 7] = f7[i % len(F7)]
    f9[:, 8] = eu[i % len(EU32)]
    suf = np.array([E64[int(k) % len(E64)] for k in i], dtype=np.int64) if n else np.zeros(0, np.int64)
    return (f9 & 0xffffffff).astype(np.uint32).view(np.int32).reshape(n, 9), suf


def csn_cases():
    out = [Csn("n%d" % n, *csn_rows(n)) for n in COUNTS]
    # 64 equal names of 33 bytes: the offsets take every residue mod 16 (33 is odd), four times over
    f9 = np.zeros((64, 9), np.int32)
    f9[:, 0] = 5                     # 15 + "_0_0_0_0_" + "" + "_" + "" + "_pos_0:1"
    f9[:, 5] = f9[:, 6] = 1
    out.append(Csn("residues", f9, np.ones(64, np.int64)))
    # every name longer than 254 bytes
    f9 = csn_rows(40)[0].copy()
    f9[:, 5] = 3
    out.append(Csn("long", f9, csn_rows(40)[1]))
    return out


def csn_refusals():
    """(label, case, the index the refusal must name)"""
    out = []
    for col, size in ((0, len(BARCODES)), (5, len(CIGARS)), (6, len(CIGARS))):
        for label, v in (("below", -1), ("size", size)):
            f9, suf = csn_rows(300)
            f9 = f9.copy()
            f9[261, col] = v
            f9[290, col] = v        # a later one: the first is the one named
            out.append(("f%d_%s" % (col, label), Csn("bad_f%d_%s" % (col, label), f9, suf, refused=261), 261))
    return out


# ---- dcs --------------------------------------------------------------------------------------------
def _pad(head, tail, n):
    """head + filler + tail, n bytes"""
    assert len(head) + len(tail) <= n
    return head + b"x" * (n - len(head) - len(tail)) + tail


# names the rule accepts as the tag and as the partner
TAGS = [
    b"_:",                                         # the shortest tag
    b"__:",                                        # empty coordinates
    _pad(b"A_1:", b"", 7), _pad(b"A_1:", b"", 8), _pad(b"A_1:", b"", 9),
    _pad(b"AC.GT_0_1234_0_5678_150M_150M_pos_300:", b"7", 254),
    _pad(b"AC.GT_0_1234_0_5678_150M_150M_neg_300:", b"_9", 254),
    b"pos_1_2:3",                                  # "pos" at the start ...
    b"AC_1_2:3pos",                                # ... at the very end ...
    _pad(b"_:", b"", 5) + b"pos", _pad(b"_:", b"", 6) + b"pos", _pad(b"_:", b"", 7) + b"pos",    # ... from byte 5, 6, 7 of a word
    _pad(b"_:", b"", 13) + b"pos:z", _pad(b"_:", b"", 14) + b"pos_z", _pad(b"_:", b"", 15) + b"posz",
    b"ApoposC_1_2:3",                              # inside the barcode
    b"AC_1_2:3po", b"AC_1_2:po", _pad(b"A_1:", b"po", 16), _pad(b"A_1:", b"p", 16), _pad(b"A_1:", b"pos", 8),
    b"AC_1_2:3p_os", b"po_s:1", b"AC_1_2:3_pso",   # near misses
    b"AC.GT_1_2_x:33",                             # no second ':'
    b"AC.GT_1_2::5", b"AC.GT_1_2:", b"AC.GT_1_2::",   # empty fields
    b"AC_12:3",                                    # a rest without '_'
    b"AC.GT_0_100_0_200_150M_150M_neg_350:12:x:y",  # more than two ':'
    b":_", b":a_b:c",                              # ':' before the first '_'
    _pad(b"", b"_:", 8), _pad(b"", b"_:", 9), _pad(b"", b"_:", 16), _pad(b"", b":_", 17),   # found in a word's last bytes
]
PARTNERS = [b":", b"AC:7", b"_:", b"TT.GG_0_1_0_2_150M_150M_neg_1:4", _pad(b"G:", b"", 8), _pad(b"G_:", b":", 9),
            _pad(b"TG.CA_5:", b"", 254), b"x:pos"]
# the output lengths 4, 15, 16, 17, 31, 32, 33 (4 is the shortest name the rule can make: its four separators)
LENGTH_TAGS = [b"B" * k + b"__:" for k in (0, 11, 12, 13, 27, 28, 29)]
LENGTHS = (4, 15, 16, 17, 31, 32, 33)
# refused as the tag / as the partner
BAD = dict(no_us=b"AC:1", no_colon=b"AC_1", empty=b"", one=b"A")


class Dcs(object):
    def __init__(self, name, qnames, rec_tag, rec_ds, refused=-1):
        self.name, self.qnames, self.refused = name, list(qnames), refused
        self.rec_tag = np.ascontiguousarray(rec_tag, np.int64)
        self.rec_ds = np.ascontiguousarray(rec_ds, np.int64)

    def write(self, d):
        """The names as the records of a BAM file under d; its path."""
        recs = [UC.Rec(q + b"\x00", [1, 2, 4, 8], [30, 31, 32, 33], [(0, 4)], pos=1000 + i)
                for i, q in enumerate(self.qnames)]
        return UC.write_bam("%s/%s.bam" % (str(d), self.name), recs)


QNAMES = TAGS + PARTNERS + LENGTH_TAGS
N_TAGS = len(TAGS)


# the records that can be the tag (the partners without '_' cannot), and any record as the partner
TAG_IDX = np.array(list(range(N_TAGS)) + list(range(N_TAGS + len(PARTNERS), len(QNAMES))), np.int64)


def dcs_pairs(n):
    i = np.arange(n, dtype=np.int64)
    return TAG_IDX[i % len(TAG_IDX)], (i * 7 + 3) % len(QNAMES)


def dcs_cases():
    nq = len(QNAMES)
    t, d = np.meshgrid(TAG_IDX, np.arange(nq), indexing="ij")   # every tag with every name, itself included
    out = [Dcs("all_pairs", QNAMES, t.reshape(-1), d.reshape(-1))]
    lt = np.arange(nq - len(LENGTH_TAGS), nq)
    out.append(Dcs("lengths", QNAMES, lt, np.full(len(lt), N_TAGS + 2)))        # the partner "_:"
    out.append(Dcs("residues", QNAMES, np.full(64, lt[3]), np.full(64, N_TAGS + 2)))   # 64 names of 17 bytes
    out += [Dcs("n%d" % n, QNAMES, *dcs_pairs(n)) for n in COUNTS]
    return out


def dcs_refusals():
    """(label, case, the index the refusal must name, host: the host function can be asked)"""
    names = QNAMES + [BAD["no_us"], BAD["no_colon"], BAD["empty"], BAD["one"]]
    nq = len(QNAMES)
    out = []
    for label, tag, ds in (("t_no_us", nq, 0), ("t_no_colon", nq + 1, 0), ("d_no_colon", 0, nq + 1), ("t_empty", nq + 2, 0),
                           ("d_empty", 0, nq + 2), ("t_one", nq + 3, 0), ("rec_size", len(names), 0), ("ds_size", 0, len(names)),
                           ("rec_below", -1, 0)):
        t, d = (x.copy() for x in dcs_pairs(300))
        for bad in (261, 290):
            t[bad], d[bad] = tag, ds
        out.append((label, Dcs("bad_" + label, names, t, d, refused=261), 261, "size" not in label and "below" not in label))
    return out
