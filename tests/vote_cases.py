"""The cases of tests/test_gpu_vote_edges.py (the kernels against tests/vote_refs.py) and, in a reduced
draw, of tests/test_vote_refs.py (vote_refs against the Python oracle): tables of reads built on
arrays, the families and pairs voted over them, and the launch-geometry edges they are laid on.

The kernel constants are mirrored here (test_vote_refs.py checks them against csrc/cc_engine.hip);
every edge list is derived from them."""
import math
import struct

import numpy as np

import vote_refs as R

# ---- mirrored from csrc/cc_engine.hip -----------------------------------------------------------
VOTE_BIGN = 63      # members the SWAR vote takes (byte counters)
BIG_CH = 63         # members per item of a larger family
BIG_STAGE = 6       # items per wave up to which k_big_swar stages member records in LDS
SV_POS = 16         # positions per lane
MODE_K = 4          # distinct values table_mode holds before serial_mode takes over
MODE_SLOTS = 256    # distinct values lds_mode holds before wave_mode takes over
WAVE = 64           # lanes per wave (gfx950)


def chunks_of(max_len):
    return (max_len + SV_POS - 1) // SV_POS


def fams_per_wave(max_len):
    """fpw of vote_families / duplex_vote: families (items, pairs) side by side in a wave."""
    return WAVE // min(WAVE, max(1, chunks_of(max_len)))


# the table's longest read: fpw 64, 64, 32, BIG_STAGE + 1 (unstaged, one idle lane), BIG_STAGE
# (staged), 1 with 31 idle lanes, 1 with every lane used, all_slow
TABLE_LENS = (1, SV_POS, SV_POS + 1,
              SV_POS * (WAVE // (BIG_STAGE + 1)), SV_POS * (WAVE // (BIG_STAGE + 1)) + 1,
              SV_POS * (WAVE // 2) + SV_POS // 2, SV_POS * WAVE, SV_POS * WAVE + 1)
LONG_TABLES = TABLE_LENS[-3:]
SIZES = (1, 2, 3, VOTE_BIGN - 1, VOTE_BIGN, VOTE_BIGN + 1, VOTE_BIGN + 2, 2 * BIG_CH, 2 * BIG_CH + 1,
         3 * BIG_CH, 3 * BIG_CH + 1, 300)
LONG_SIZES = (1, 2, VOTE_BIGN, VOTE_BIGN + 1, 2 * BIG_CH + 1)
QUALS = (0, 2, 29, 30, 31, 59, 60, 61, 93, 127, 128, 157, 158, 254)
PASS_Q = tuple(q for q in QUALS if q >= R.PHRED_PASS)
FAIL_Q = tuple(q for q in QUALS if q < R.PHRED_PASS)
LONE_Q = (30, 60, 61, 254)
CUTOFFS = (0.7, math.nextafter(0.7, 1.0), 0.5, 2.0 / 3.0, 1.0 / 3.0, 1.0, math.nextafter(1.0, 2.0), 0.0)
DISTINCT = (1, MODE_K, MODE_K + 1, MODE_SLOTS, MODE_SLOTS + 1)
NT16 = "=ACMGRSVTWYHKDBN"
IUPAC = tuple(c for c in range(1, 15) if c not in R.ACGT)      # M R S V W Y H K D B
ACGTN = R.ACGT + (R.N,)


def family_lengths(max_len):
    """Member 0's lengths under a table of longest read max_len: that read's, one that is no multiple
    of SV_POS, one less, and 1."""
    odd = (max_len * 5 // 8) | 1
    out = []
    for v in (max_len, odd, max_len - 1, 1):
        if 1 <= v <= max_len and v not in out:
            out.append(v)
    return out


def min_count(passed, cutoff):
    """The smallest count with count / passed >= cutoff (passed + 1 when none), in Python floats."""
    for c in range(passed + 1):
        if c / passed >= cutoff:
            return c
    return passed + 1


# ---- tables ---------------------------------------------------------------------------------------
class Table(object):
    """Reads as arrays: base codes and qualities per read (the cigar is one M of the read's length),
    flag, mapq, tlen and the RG string (None: no RG tag)."""

    def __init__(self):
        self.codes, self.quals, self.flag, self.mapq, self.tlen, self.rg = [], [], [], [], [], []

    def add(self, codes, quals, flag=99, mapq=60, tlen=350, rg="1"):
        codes = np.asarray(codes, np.uint8)
        quals = np.asarray(quals, np.uint8)
        assert len(codes) == len(quals) > 0 and quals[0] != 255 and codes.min() >= 1
        self.codes.append(codes)
        self.quals.append(quals)
        self.flag.append(int(flag))
        self.mapq.append(int(mapq))
        self.tlen.append(int(tlen))
        self.rg.append(rg)
        return len(self.codes) - 1

    def __len__(self):
        return len(self.codes)

    @property
    def max_len(self):
        return max(len(c) for c in self.codes)

    def raw(self, i):
        """Read i as a BAM record (block_size first)."""
        import pysam
        codes = self.codes[i]
        n = len(codes)
        nib = np.zeros(2 * ((n + 1) // 2), np.uint8)
        nib[:n] = codes
        packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
        qn = ("r%d|AC.GT" % i).encode() + b"\x00"
        body = struct.pack("<iiBBHHHiiii", 0, 1000, len(qn), self.mapq[i], pysam.reg2bin(1000, 1000 + n), 1,
                           self.flag[i], n, 0, 1200, self.tlen[i])
        body += qn + struct.pack("<I", (n << 4) | 0) + packed + self.quals[i].tobytes()
        if self.rg[i] is not None:
            body += b"RGZ" + self.rg[i].encode() + b"\x00"
        return struct.pack("<i", len(body)) + body

    def header(self):
        import pysam
        return pysam.AlignmentHeader("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n", [("chr1", 1000000)])

    def write(self, path):
        import pysam
        pysam.write_bam_file(path, self.header(), [self.raw(i) for i in range(len(self))], level=1)

    def segment(self, i):
        """Read i as the oracle's record type."""
        import pysam
        r = pysam.AlignedSegment(self.header())
        r.query_name = "r%d|AC.GT" % i
        r.flag = self.flag[i]
        r.reference_id = 0
        r.reference_start = 1000
        r.mapping_quality = self.mapq[i]
        r.cigartuples = [(0, len(self.codes[i]))]
        r.next_reference_id = 0
        r.next_reference_start = 1200
        r.template_length = self.tlen[i]
        r.query_sequence = "".join(NT16[c] for c in self.codes[i])
        r.query_qualities = [int(q) for q in self.quals[i]]
        if self.rg[i] is not None:
            r.set_tag("RG", self.rg[i])
        return r


def expect_family(table, members, cutoff):
    """What the vote of family `members` (record indices, member 0 first) must return: (codes, quals,
    [L, mapq, tlen, flag], RG string or None); VoteError as consensus_maker raises."""
    L = len(table.codes[members[0]])
    codes, quals = R.sscs_vote([table.codes[j] for j in members], [table.quals[j] for j in members], cutoff, L)
    meta = [L, R.most_common_first([table.mapq[j] for j in members]),
            R.most_common_first([table.tlen[j] for j in members]), R.pick_flag([table.flag[j] for j in members])]
    return codes, quals, meta, R.family_rg([table.rg[j] for j in members])


# ---- per-position patterns of one family ----------------------------------------------------------
UNANIMOUS, THRESHOLD, TIE2, TIE3, TIE4, LONE, NO_PASS, ONE_PASS, FAILED_N = range(9)
KINDS = (UNANIMOUS, THRESHOLD, TIE2, THRESHOLD, LONE, TIE3, THRESHOLD, NO_PASS, TIE4, ONE_PASS, THRESHOLD, FAILED_N)


def column(rng, n, kind):
    """Base codes and qualities of n members at one position, laid out for `kind`."""
    b = rng.choice(R.ACGT, n)
    q = rng.choice(FAIL_Q, n)
    order = rng.permutation(n)
    bases = rng.permutation(R.ACGT)
    at = [0]

    def put(count, base, quals=None):
        idx = order[at[0]:at[0] + count]
        at[0] += count
        b[idx] = base
        q[idx] = rng.choice(PASS_Q, len(idx)) if quals is None else quals

    if kind in (TIE2, TIE3, TIE4) and n < kind - TIE2 + 2:
        kind = UNANIMOUS
    if kind == LONE and n < 2:
        kind = ONE_PASS
    if kind == UNANIMOUS:
        put(n if rng.random() < 0.5 else int(rng.integers(1, n + 1)), bases[0])
    elif kind in (THRESHOLD, FAILED_N):
        # the best count exactly at, or one below, the smallest count that passes one of the cutoffs,
        # at a pass count where count / pass can equal it exactly (multiples of 10, 3 and 2)
        p = int(rng.integers(1, n + 1)) if kind == THRESHOLD else max(1, n - int(rng.integers(1, 4)))
        d = int(rng.choice((1, 10, 3, 2)))
        if p >= d:
            p -= p % d
        t = min_count(p, CUTOFFS[int(rng.integers(len(CUTOFFS)))])
        best = min(p, max(1, t - int(rng.integers(0, 2))))
        put(best, bases[0])
        rest = p - best
        for k in (1, 2, 3):                     # the others share the rest, below the best where it fits
            c = min(rest, best - 1) if k < 3 else rest
            put(c, bases[k])
            rest -= c
        if kind == FAILED_N:
            b[order[at[0]:]] = R.N              # every failing member an N below Q30
    elif kind in (TIE2, TIE3, TIE4):
        k = kind - TIE2 + 2
        m = int(rng.integers(1, n // k + 1))
        for j in range(k):
            put(m, bases[j])
    elif kind == LONE:
        # count[best] == 1 below the pass count: the consensus quality is that one member's
        p = min(n, int(rng.integers(2, 5)))
        first = min(bases[:p])                  # the first maximum in A, C, G, T order
        for j in range(p):
            put(1, bases[j], int(rng.choice(LONE_Q)) if bases[j] == first else None)
    elif kind == ONE_PASS:
        put(1, bases[0], int(rng.choice(PASS_Q)))
    # failing members: any base, N included
    fail = order[at[0]:]
    if kind != FAILED_N and len(fail):
        b[fail] = rng.choice(ACGTN, len(fail))
    return b, q


def add_family(table, rng, n, length, max_len, meta_pool=3):
    """n reads voting as one family of consensus length `length` (member 0's), the others that long or
    longer, up to max_len; positions from `length` on hold IUPAC bases, N at Q >= 30 and other bases,
    which no vote may look at.  Returns the reads' indices, member 0 first."""
    b = np.zeros((n, length), np.uint8)
    q = np.zeros((n, length), np.uint8)
    off = int(rng.integers(len(KINDS)))
    for i in range(length):
        b[:, i], q[:, i] = column(rng, n, KINDS[(i + off) % len(KINDS)])
    flags = rng.choice((99, 83, 147, 163, 97, 145, 1024, 0), meta_pool, replace=False)
    mapqs = rng.choice(256, meta_pool, replace=False)
    tlens = rng.choice(np.arange(-400, 400), meta_pool, replace=False)
    rgs = ("1", "2", "1") if rng.random() < 0.3 else ("1",)
    idx = []
    for j in range(n):
        ln = length
        if j > 0 and length < max_len and (j == n - 1 or rng.random() < 0.5):
            ln = max_len if j == n - 1 else int(rng.integers(length + 1, max_len + 1))
        cb, cq = b[j], q[j]
        if ln > length:
            tb = rng.integers(1, 16, ln - length).astype(np.uint8)
            tq = rng.choice(QUALS, ln - length).astype(np.uint8)
            tb[0], tq[0] = ((IUPAC[j % len(IUPAC)], 60), (R.N, 30), (R.ACGT[j % 4], 254))[j % 3]
            cb, cq = np.concatenate([cb, tb]), np.concatenate([cq, tq])
        idx.append(table.add(cb, cq, flag=rng.choice(flags), mapq=rng.choice(mapqs), tlen=rng.choice(tlens),
                             rg=None if (n > 1 and rng.random() < 0.01) else rgs[j % len(rgs)]))
    return idx


def sscs_matrix(max_len, seed, sizes=None, rounds=None, min_calls=8):
    """The table of longest read max_len and the calls voted over it: (Table, [(cutoff, [family, ..])]),
    a family the list of its reads.  Every size meets `rounds` of the family lengths; small families fill
    up to the largest call; the calls hold fpw - 1, fpw, fpw + 1 and 4 fpw + 1 families (none of 0
    families: nothing to compare), walking the families round until each was voted, with the cutoffs
    in turn, so no two calls in a row share one."""
    rng = np.random.default_rng(seed)
    fpw = fams_per_wave(max_len)
    if sizes is None:
        sizes = LONG_SIZES if max_len in LONG_TABLES else SIZES
    lens = family_lengths(max_len)
    if rounds is None:
        rounds = 4 if max_len in LONG_TABLES else 2
    spec = [(n, lens[(i + r) % len(lens)]) for r in range(rounds) for i, n in enumerate(sizes)]
    k = 0
    while len(spec) < 4 * fpw + 1:
        spec.append(((1, 2, 3)[k % 3], lens[k % len(lens)]))
        k += 1
    order = rng.permutation(len(spec))           # small and big families mixed in every call
    table = Table()
    fams = [None] * len(spec)
    for s in order:
        fams[s] = add_family(table, rng, spec[s][0], spec[s][1], max_len, meta_pool=3 if s % 4 else 6)
    fams = [fams[s] for s in order]
    counts = [c for c in (fpw - 1, fpw, fpw + 1, 4 * fpw + 1) if c > 0]
    calls, start, used = [], 0, 0
    while len(calls) < min_calls or used < len(fams):
        c = counts[len(calls) % len(counts)]
        calls.append((CUTOFFS[len(calls) % len(CUTOFFS)], [fams[(start + j) % len(fams)] for j in range(c)]))
        start = (start + c) % len(fams)
        used += c
    assert table.max_len == max_len
    return table, calls


# ---- mode fields ----------------------------------------------------------------------------------
def plain_read(rng, length):
    return rng.choice(R.ACGT, length), rng.choice(PASS_Q[:4], length)


def mode_family(table, rng, n, length, field, values):
    """n plain reads whose `field` holds values[j]; the other fields are member 0's."""
    idx = []
    for j in range(n):
        b, q = plain_read(rng, length)
        kw = dict(flag=99, mapq=60, tlen=350, rg="1")
        kw[field] = values[j]
        idx.append(table.add(b, q, **kw))
    return idx


def spread_values(rng, n, distinct, pool, tie):
    """n values over `distinct` different ones from pool, each at least once, in random order; the rest
    go to one of them (tie: split between two, so the first seen of the two must win)."""
    vals = [int(v) for v in rng.choice(pool, distinct, replace=False)]
    out = list(vals)
    extra = n - distinct
    if distinct == 1:
        return [vals[0]] * n
    w1, w2 = (int(x) for x in rng.choice(distinct, 2, replace=False))
    if tie:
        extra -= extra % 2
        out += [vals[w1]] * (extra // 2) + [vals[w2]] * (extra // 2)
    else:
        out += [vals[w1]] * extra
    out = [out[i] for i in rng.permutation(len(out))]
    return out + [out[0]] * (n - len(out))


def mode_matrix(seed, length=20):
    """Families whose mapq, tlen or flag holds 1, MODE_K, MODE_K + 1, MODE_SLOTS and MODE_SLOTS + 1
    distinct values (as many as the family and the field's width allow), with one winner and with a
    first-seen tie, each in a family of at most VOTE_BIGN members and in a larger one."""
    rng = np.random.default_rng(seed)
    table, fams = Table(), []
    pools = {"mapq": np.arange(256), "tlen": np.arange(-70000, 70000), "flag": np.arange(4096)}
    for big in (False, True):
        for field in ("mapq", "tlen", "flag"):
            seen = set()
            for d in DISTINCT:
                n = VOTE_BIGN if not big else max(VOTE_BIGN + 4, d + VOTE_BIGN)
                d = min(d, n - 2, len(pools[field]))
                for tie in (False, True):
                    if (d, tie) in seen or (tie and d == 1):
                        continue
                    seen.add((d, tie))
                    fams.append(mode_family(table, rng, n, length, field, spread_values(rng, n, d, pools[field], tie)))
    return table, fams


def flag_tie_matrix(seed, length=20):
    """Flag ties among 99, 83, 147 and 163 (the first 2, 3 and 4 of every first-seen order), each beside a
    rarer flag seen first, in families of at most VOTE_BIGN members and in larger ones; then ties
    among other flags, and a priority flag tied with another one seen before it."""
    import itertools
    rng = np.random.default_rng(seed)
    table, fams = Table(), []
    perms = list(itertools.permutations(R.FLAG_PRIORITY))
    for big in (False, True):
        for pi, perm in enumerate(perms):
            for k in (2, 3, 4):
                if big and k < 4 and pi % 4:
                    continue
                m = 2 if not big else VOTE_BIGN // k + 1
                vals = [1024] + list(perm[:k]) * m
                fams.append(mode_family(table, rng, len(vals), length, "flag", vals))
        m = 3 if not big else VOTE_BIGN // 2 + 1
        for vals in ([97, 145] * m, [145, 97] * m, [97, 163] * m, [0, 97, 83, 1024] * m):
            fams.append(mode_family(table, rng, len(vals), length, "flag", vals))
    return table, fams


def rg_matrix(seed, length=20, groups=200):
    """More than 126 read groups (ids from 126 on take the member record's escape to the RG column),
    each seen once in file order first; then families whose RG mode is a low id, a high id, a
    first-seen tie of the two, and families with one member without RG; small and larger ones."""
    rng = np.random.default_rng(seed)
    table, fams = Table(), []
    names = ["g%03d" % i for i in range(groups)]
    fams.append(mode_family(table, rng, groups, length, "rg", names))     # (all tied: the first seen wins)
    for n in (VOTE_BIGN, 2 * BIG_CH + 1):
        lo, hi, hi2 = names[3], names[150], names[199]
        h = n // 2
        for vals in ([lo] * n, [hi] * n, [hi2] + [hi] * (n - 1), [lo] + [hi] * (n - 1), [hi] * (h + 1) + [lo] * (n - h - 1),
                     [hi, lo] * h + [hi2], [lo, hi] * h + [hi2], [hi] * (n - 1) + [None], [None] + [lo] * (n - 1),
                     [hi] * h + [None] + [lo] * (n - h - 1)):
            fams.append(mode_family(table, rng, n, length, "rg", vals))
    return table, fams


# ---- defined errors ---------------------------------------------------------------------------------
def error_matrix(max_len, seed):
    """One clean family of 3 BIG_CH + 1 unanimous reads of length max_len and offending reads to put in
    a member's place: (Table, clean reads, [(kind, family)]), one offender per family.  The families:
    5 and VOTE_BIGN members (the SWAR vote, or k_big_final's own count when max_len makes every
    family slow) with the offender in the middle or last, and all 3 BIG_CH + 1 (items) with it in the first, a
    middle and the last item and as the last member."""
    rng = np.random.default_rng(seed)
    table = Table()
    cons = rng.choice(R.ACGT, max_len)
    n = 3 * BIG_CH + 1
    clean = [table.add(cons, rng.choice(PASS_Q, max_len)) for _ in range(n)]
    spots = sorted(set(p for p in (0, SV_POS - 1, SV_POS, max_len - 1, max_len // SV_POS * SV_POS - 1,
                                   max_len // 2) if 0 <= p < max_len))
    shorts = sorted(set(v for v in (max_len - 1, 1, max_len // 2) if 1 <= v < max_len))
    places = [(5, 2), (5, 4), (VOTE_BIGN, VOTE_BIGN - 1), (n, 1), (n, BIG_CH + BIG_CH // 2), (n, 3 * BIG_CH - 1), (n, n - 1)]
    out = []
    for ki, kind in enumerate((R.SHORT_READ, R.N_HIGHQ, R.BAD_BASE)):
        for pi, (size, at) in enumerate(places):
            b, q = cons.copy(), rng.choice(PASS_Q, max_len)
            if kind == R.SHORT_READ:
                ln = shorts[(pi + ki) % len(shorts)]
                b, q = b[:ln], q[:ln]
            else:
                p = spots[(pi + ki) % len(spots)]
                b[p] = R.N if kind == R.N_HIGHQ else IUPAC[pi % len(IUPAC)]
                q[p] = PASS_Q[pi % len(PASS_Q)] if kind == R.N_HIGHQ else QUALS[pi % len(QUALS)]
            fam = list(clean[:size])
            fam[at] = table.add(b, q)
            out.append((kind, fam))
    return table, clean, out


# ---- pairs ------------------------------------------------------------------------------------------
PAIR_LENS = (1, SV_POS - 1, SV_POS, SV_POS + 1, 150, SV_POS * WAVE, SV_POS * WAVE + 1, SV_POS * (WAVE + 1))
PAIR_FLAGS = (99, 83, 147, 163, 97, 145, 1024)


def pair_reads(table, rng, template, lengths, salt):
    """One read per length over the template: substitutions, N, qualities from QUALS; flags over the
    priority list and beyond, mapq and tlen different per read, every fifth read without RG."""
    idx = []
    for j, ln in enumerate(lengths):
        b = template[:ln].copy()
        sub = rng.random(ln) < 0.25
        b[sub] = rng.choice(R.ACGT, int(sub.sum()))
        b[rng.random(ln) < 0.15] = R.N
        q = rng.choice(QUALS, ln)
        idx.append(table.add(b, q, flag=PAIR_FLAGS[(j * salt + j // len(PAIR_FLAGS)) % len(PAIR_FLAGS)],
                             mapq=(17 * j + salt) % 256, tlen=300 + 3 * j - 50 * salt,
                             rg=None if j % 5 == salt % 5 else "g%d" % ((j + salt) % 3)))
    return idx


def pair_matrix(len1, a_longer, seed):
    """Two tables of different longest read for pairs whose read 1 has len1 bases: table A's reads 1
    (and, with a_longer, one longer read that makes A the table of the longer reads), table B's reads 2 of
    len1 .. len1 + SV_POS bases.  Returns (A, B, reads 1, reads 2, A's long reads, B's short reads)."""
    rng = np.random.default_rng(seed)
    n = 20 if len1 <= 150 else 6
    template = rng.choice(R.ACGT, len1 + 3 * SV_POS)
    a, b = Table(), Table()
    r1 = pair_reads(a, rng, template, [len1] * n, 1)
    long_a = pair_reads(a, rng, template, [len1 + 1] + ([len1 + 2 * SV_POS + 5] if a_longer else []), 2)
    r2 = pair_reads(b, rng, template, [len1 + (0, 1, SV_POS // 2 + 1, SV_POS)[j % 4] for j in range(n)], 3)
    short_b = pair_reads(b, rng, template, [len1 - 1], 4) if len1 > 1 else []
    assert (a.max_len > b.max_len) == bool(a_longer) and a.max_len != b.max_len
    return a, b, r1, r2, long_a, short_b
