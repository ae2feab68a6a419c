"""The cases of tests/test_gpu_duplex_edges.py (cc_duplex_consensus and cc_singleton_correction against
tests/duplex_refs.py) and of tests/test_duplex_refs.py (duplex_refs against the Python oracle):
SSCS-like BAMs in which every record is one read end of a proper pair and the barcode is the qname's
first '_' field, laid out so that families fall on the edges of the joins' geometry.

A molecule has its first end on one contig and its mate mirrored onto a later one, so a whole-file
stream completes the pairs in the order of the later ends: that order (the entry slot) is the
builder's to choose.  The duplex partner of molecule (barcode, 'a': flags 99 / 147) is (swapped
barcode, 'b': flags 163 / 83) at the same coordinates, at both ends.  A coordinate grouping lists
families in (tid, pos) order, so one-molecule filler sites position every group's first family by
index; INSIDE a position group the engine orders families by their seeded tag hash, which no BAM can
choose, so a test group pairs a third of its families mutually and leaves the others without a
partner: whichever families come first and last, some search the whole group in both directions to
the tag that ends the walk, and the planned re-runs reorder them.

The kernel constants are mirrored here (test_duplex_refs.py checks them against csrc/cc_engine.hip).
A case's `edges` are the edges its builder placed; test_duplex_refs.py derives them again from the
finished table.

Orphan tags ("Consensus tag NOT UNIQUE") are constructible through BAM records: a second pair with the
molecule name of an earlier one whose later end differs in orientation adds a third read-end key.

Bed files (class D for DCS, C-bed for SC): duplex partners share tid, pos, mtid and mpos, so both are
read by the same regions and complete in the same one.  A partner family of another region is made
by a stray third record under a molecule's qname in an earlier region: the stream pairs the stray
with the molecule's next end, whose tag is thereby created a region early.  For DCS a processed
partner of another region always ends in the reference's KeyError (one such case is kept), so the
two cases that give a result pair a tag with an ORPHAN tag of an earlier and of a later region.

The issue's "SSCS table of one family" is built as one molecule, two families: a proper pair's two
ends differ in their read number, so no whole-file grouping of proper pairs holds one family."""
import struct

import numpy as np

import duplex_refs as R
import pair_cases as PC

# ---- mirrored from csrc/cc_engine.hip -----------------------------------------------------------
DD_T = 256           # k_dcs_decide_fam: families per block
DD_H = 64            # and staged neighbours on each side
DEEP_MIN = 65        # records from which a position group is deep (the grouping is then not local)
DUPLEX_CHAIN = 32    # earlier-processed partners followed
HT_FLOOR = 1024      # build_ht: smallest table
HT_FACTOR = 2        # and slots per family, rounded up to a power of two

CONTIGS = (("chr1", 1 << 28), ("chr2", 1 << 28), ("chr3", 1 << 28))
GROUPS = (2, 3, DD_H - 1, DD_H)
BLOCKS = (0, 1, "last")
CHAIN_HOPS = (1, 2, 3, 4, 5, DUPLEX_CHAIN - 1, DUPLEX_CHAIN)
FAR = ("present", "absent")
HASHED_F = (511, 512, 513)
QUALS = (12, 28, 29, 29, 30, 30, 31, 35, 40)
PATHS = ("default", "per_entry", "hashed")


def offsets(g):
    return tuple(sorted({-DD_H, -DD_H + 1, -(g - 1), -1, 0, 1}))


def ht_size(F):
    size = HT_FLOOR
    while size < HT_FACTOR * F:
        size <<= 1
    return size


def bucket_geometry(n, ext):
    """k_bucket_geom: the finest shift with at most 2n + ntid buckets, and each contig's first bucket."""
    shift = 30
    for s in range(30):
        if sum((e >> s) + 1 for e in ext) <= 2 * n + len(ext):
            shift = s
            break
    tbase = [0]
    for e in ext:
        tbase.append(tbase[-1] + (e >> shift) + 1)
    return shift, tbase


def bucket_of(shift, tbase, tid, pos):
    ntid = len(tbase) - 1
    if tid < 0 or tid >= ntid:
        return tbase[ntid]
    return min(tbase[tid] + (max(pos, 0) >> shift), tbase[tid + 1])


def table_geometry(t):
    """(shift, tbase) of a sorted table: each contig's extent is its largest position."""
    ntid = int(t.tid.max()) + 1 if len(t) else 0
    ext = [int(t.pos[t.tid == k].max()) if np.any(t.tid == k) else 0 for k in range(ntid)]
    return bucket_geometry(len(t), ext)


# ---- tables ---------------------------------------------------------------------------------------
class Table(PC.Table):
    """pair_cases.Table with a read length (8 or 24), base codes and qualities per record."""

    def __init__(self, n):
        PC.Table.__init__(self, n)
        self.codes = [None] * n
        self.quals = [None] * n
        self.mapq = np.full(n, 60, np.int32)
        self.max_len = 0

    def cigar(self, i):
        return "%dM" % len(self.codes[i])

    def raw(self, i):
        import pysam
        c = np.asarray(self.codes[i], np.uint8)
        L = len(c)
        c2 = np.concatenate([c, np.zeros(L & 1, np.uint8)])
        packed = ((c2[0::2] << 4) | c2[1::2]).astype(np.uint8).tobytes()
        qn = self.qname[i].encode() + b"\x00"
        p = int(self.pos[i])
        body = struct.pack("<iiBBHHHiiii", int(self.tid[i]), p, len(qn), int(self.mapq[i]), pysam.reg2bin(p, p + L), 1,
                           int(self.flag[i]), L, int(self.mtid[i]), int(self.mpos[i]), int(self.tlen[i]))
        body += qn + struct.pack("<I", (L << 4) | 0) + packed + np.asarray(self.quals[i], np.uint8).tobytes()
        return struct.pack("<i", len(body)) + body

    def header(self):
        import pysam
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
        return pysam.AlignmentHeader(text, list(CONTIGS))

    def segment(self, i, header=None):
        import pysam
        r = pysam.AlignedSegment(header or self.header())
        r.query_name = self.qname[i]
        r.flag = int(self.flag[i])
        r.reference_id = int(self.tid[i])
        r.reference_start = int(self.pos[i])
        r.mapping_quality = int(self.mapq[i])
        r.cigartuples = [(0, len(self.codes[i]))]
        r.next_reference_id = int(self.mtid[i])
        r.next_reference_start = int(self.mpos[i])
        r.template_length = int(self.tlen[i])
        r.query_sequence = "".join(PC.NT16[c] for c in self.codes[i])
        r.query_qualities = [int(q) for q in self.quals[i]]
        return r


FLAGS = {"a": (99, 147), "b": (163, 83)}


def dotted(k):
    """Barcode k of a family of mutual pairs: no two of them, swapped or not, are equal."""
    b = "ACGT"
    enc = lambda v: "".join(b[(v >> (2 * j)) & 3] for j in range(7))
    return enc(2 * k) + "." + enc(2 * k + 1)


class Layout(object):
    """A table under construction, molecule by molecule."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.mols = []
        self.nbc = 0
        self.site_seq = {}

    def fresh(self):
        self.nbc += 1
        return dotted(self.nbc)

    def add(self, bc, orient, a, b, order=None, flags=None, tlen=0, stray=None):
        """One molecule: ends at a = (tid, pos) and b, a < b; order: its later end's place among the
        records of b (the pair completes there); flags: the two ends' flags instead of orient's;
        stray = ((tid, pos), end): a third record under the molecule's qname in place of that end, before
        both: the stream pairs it with the other end."""
        assert a < b and (stray is None or stray[0] < a)
        self.mols.append(dict(bc=bc, flags=flags or FLAGS[orient], a=a, b=b, tlen=tlen, stray=stray,
                              order=len(self.mols) if order is None else order))
        return len(self.mols) - 1

    def reads(self, where, L):
        if where not in self.site_seq:
            self.site_seq[where] = self.rng.choice((1, 2, 4, 8), L).astype(np.uint8)
        c = self.site_seq[where].copy()
        hit = self.rng.random(L)
        c[hit < 0.08] = self.rng.choice((1, 2, 4, 8), int((hit < 0.08).sum()))
        c[hit > 0.96] = 15
        return c, self.rng.choice(QUALS, L).astype(np.uint8)

    def table(self):
        ends = []
        for m, mol in enumerate(self.mols):
            ends.append((mol["a"], 0, m, m, 0, False))
            ends.append((mol["b"], 1, mol["order"], m, 1, False))
            if mol["stray"]:
                ends.append((mol["stray"][0], 0, m, m, mol["stray"][1], True))
        ends.sort()
        length = lambda pos: 24 if (pos // 40) % 3 == 0 else 8       # one length per site
        t = Table(len(ends))
        for i, (at, _, _, m, end, stray) in enumerate(ends):
            mol = self.mols[m]
            mate = mol["b"] if end == 0 else mol["a"]
            L = length(mate[1] if stray else at[1])
            t.qname[i] = "%s_%d_%s_0:%d" % (mol["bc"], m, "pos" if mol["flags"][0] == 99 else "neg", 1 + m % 4)
            t.tid[i], t.pos[i], t.mtid[i], t.mpos[i] = at[0], at[1], mate[0], mate[1]
            t.flag[i] = mol["flags"][end]
            same = at[0] == mate[0]
            t.tlen[i] = (mate[1] + L - at[1] if at < mate else -(at[1] + L - mate[1])) if same else \
                (mol["tlen"] if end == 0 else -mol["tlen"])
            t.mapq[i] = 60 if m % 5 else 37
            t.codes[i], t.quals[i] = self.reads((at, mate, stray) if end == 0 else (mate, at, 1, stray), L)
        t.max_len = max([len(c) for c in t.codes] or [0])
        assert t.is_sorted()
        return t


def site(i):
    """Site i: the first ends on chr1, the mates mirrored onto chr2."""
    return (0, 1000 + 40 * i), (1, 1000 + 40 * i)


class Case(object):
    def __init__(self, name, kind, table, edges, sscs=None, error=None, engine_error=None, hashed=False,
                 s_hashed=False, regions=None, ran=(), not_ran=()):
        self.regions = regions                # the bed file's regions (tid, start, end), in file order
        self.ran, self.not_ran = tuple(ran), tuple(not_ran)   # bed cases: the lookup scopes observed
        self.name, self.kind, self.table, self.edges, self.sscs = name, kind, table, set(edges), sscs
        self.error = error                    # what the reference raises
        self.engine_error = engine_error      # the engine's defined error where the reference gives a result
        self.hashed = hashed                  # DCS: the grouping is not local; SC: the singleton side is hashed
        self.s_hashed = s_hashed              # SC: the SSCS side is hashed (no family buckets)


# ---- groups -----------------------------------------------------------------------------------------
def filler(L, i):
    L.add(L.fresh(), "ab"[i % 2], *site(i))


def group(L, i, g):
    """g molecules at site i: max(1, g // 3) mutual pairs, the later ends in both orders, the rest
    without a partner."""
    pairs = max(1, g // 3)
    a, b = site(i)
    for k in range(pairs):
        bc = L.fresh()
        L.add(bc, "a", a, b, order=(k if k % 2 else 10000 + k))
        L.add(R.swap_barcode(bc), "b", a, b, order=(10000 + k if k % 2 else k))
    for k in range(g - 2 * pairs):
        L.add(L.fresh(), "ab"[k % 2], a, b, order=5000 + k)


def deep_group(L, i, n=DEEP_MIN):
    """n records at one chr1 position, their mates at positions of their own: the grouping is not local."""
    a, _ = site(i)
    for k in range(n):
        L.add(L.fresh(), "a", a, (1, 1000 + 40 * (i + 1 + k)))


def one_tag(L, i, bc):
    """At site i a molecule and a second pair with its first end's tag, another orientation of the later
    end and another template length: the second pair's entry holds one tag."""
    a, b = site(i)
    L.add(bc, "a", a, b, order=0)
    L.add(bc, None, a, b, order=1, flags=(99, 163), tlen=7)


def sided(L, groups, M):
    """Sites such that the chr1 side's families number M: groups[index of the first family] = size."""
    f = i = 0
    while f < M:
        g = groups.get(f, 1)
        assert all(x not in groups for x in range(f + 1, f + g)) and f + g <= M, (f, g)
        if g == 1:
            filler(L, i)
        else:
            group(L, i, g)
        f += g
        i += 1
    return i


# ---- A. k_dcs_decide_fam's geometry --------------------------------------------------------------------
def class_a():
    M = 2 * DD_T                                   # F = 4 blocks: boundary 256 on chr1's side, the last on chr2's
    neg = [(g, s) for g in GROUPS for s in offsets(g) if s < 0]
    pos = [(g, s) for g in GROUPS for s in offsets(g) if s >= 0]
    first = list(pos)
    out = []
    for n, (g, s) in enumerate(neg):
        groups, edges = {DD_T + s: g}, {("grp", g, s, 1), ("grp", g, s, "last")}
        fit = [p for p in pos if DD_T + p[1] >= DD_T + s + g]
        if fit:
            pos.remove(fit[0])
            groups[DD_T + fit[0][1]] = fit[0][0]
            edges |= {("grp",) + fit[0] + (1,), ("grp",) + fit[0] + ("last",)}
        if first:
            g0, s0 = first.pop(0)
            groups[s0] = g0
            edges.add(("grp", g0, s0, 0))
        L = Layout(100 + n)
        sided(L, groups, M)
        out.append(Case("A-g%d-s%d" % (g, s), "dcs", L, edges))
    assert not pos and not first
    return out


def class_a_f():
    """F = 0, 1 and 255 (mod 256) with a group of 64 ending at F - 1, one-tag entries (Q > F, the last
    slot empty and past F) and orphan tags."""
    out = []
    for name, M, extra in (("A-F512", DD_T, False), ("A-F513", DD_T, True), ("A-F511", DD_T - 1, True)):
        L = Layout(len(name) + M)
        if extra:
            one_tag(L, 0, L.fresh())
        sided(L, {M - DD_H - (1 if extra else 0): DD_H}, M - (1 if extra else 0))
        if extra:                                 # (the one-tag site first: renumber it before the others)
            for m in L.mols[:2]:
                m["a"], m["b"] = (0, 900), (1, 900)
        F = 2 * M + (1 if extra else 0)
        out.append(Case(name, "dcs", L, {("F", F), ("group_ends_at_F", DD_H)} | ({("one_tag",)} if extra else set())))
    # the one-tag entry the last: its empty slot is Q - 1 = F
    L = Layout(7)
    n = sided(L, {4: 3}, 40)
    one_tag(L, n, L.fresh())
    out.append(Case("A-one-tag-last", "dcs", L, {("one_tag",), ("empty_slot_at_F",)}))
    # orphans: a third tag under a molecule name that has two; one the partner of a fourth molecule's tag
    L = Layout(8)
    n = sided(L, {5: 3}, 30)
    for k, partnered in enumerate((True, False)):
        a, b = site(n + k)
        bc = L.fresh()
        L.add(bc, "a", a, b, order=0)
        L.add(bc, None, a, b, order=1, flags=(99, 163))            # same molecule name: the orphan
        if partnered:
            L.add(R.swap_barcode(bc), None, a, b, order=2, flags=(145, 97))
    out.append(Case("A-orphans", "dcs", L, {("orphan", "partner"), ("orphan", "alone")}))
    return out


# ---- B. decisions and chains ---------------------------------------------------------------------------
def chain(L, i, hops, far, length):
    """At site i a chain of `hops` earlier-processed partners from its last-processed tag: barcodes
    without '.', of odd length, each the rotation of the one before; the far end's partner processed
    after it (present) or not there (absent)."""
    assert hops + 3 <= length and length % 2
    a, b = site(i)
    bc = "A" * (length - 3) + "CGT"
    n = hops + (2 if far == "present" else 1)
    for k in range(n):
        # element k is processed at place hops - k; the far end's partner (k = hops + 1) last
        L.add(bc, "ab"[k % 2], a, b, order=(hops - k if k <= hops else hops + 1))
        bc = R.swap_barcode(bc)


def mutual(L, i):
    a, b = site(i)
    for k, first in enumerate("ab"):
        bc = L.fresh()
        L.add(bc, "a", a, b, order=2 * k + (0 if first == "a" else 1))
        L.add(R.swap_barcode(bc), "b", a, b, order=2 * k + (1 if first == "a" else 0))


def class_b():
    out = []
    for hops in CHAIN_HOPS + (DUPLEX_CHAIN + 1,):
        for far in FAR:
            if hops > DUPLEX_CHAIN and far == "absent":
                continue
            L = Layout(300 + hops)
            n = sided(L, {3: 2}, 12)
            chain(L, n, hops, far, 9 if hops <= 5 else 37)
            mutual(L, n + 1)
            out.append(Case("B-chain-%d-%s" % (hops, far), "dcs", L, {("chain", hops, far), ("mutual", 2)},
                            error="KeyError" if far == "absent" else None,
                            engine_error="CC_E_UNSUPPORTED" if hops > DUPLEX_CHAIN else None))
    return out


def class_h():
    """The hashed path's table sizes: F = 511, 512 and 513 with the deep group's families."""
    out = []
    for F in HASHED_F:
        L = Layout(F)
        extra = F % 2
        M = (F - extra - 2 * DEEP_MIN) // 2
        if extra:
            one_tag(L, 0, L.fresh())
            for m in L.mols[:2]:
                m["a"], m["b"] = (0, 900), (1, 900)
        n = sided(L, {7: 3, 100: DD_H}, M - extra)
        out.append(Case("H-F%d" % F, "dcs", L, {("F_hashed", F, ht_size(F))}, hashed=True))
        out[-1].deep_at = n + 5
    return out


def hashed(case):
    """The case with one deep position group appended far from its edges."""
    if case.hashed:
        L = case.table
        deep_group(L, case.deep_at)
        return case
    c = Case.__new__(Case)
    c.__dict__.update(case.__dict__)
    L = Layout(0)
    L.__dict__.update(case.table.__dict__)
    L.mols = [dict(m) for m in case.table.mols]
    L.site_seq = dict(case.table.site_seq)
    L.rng = np.random.default_rng(len(L.mols))
    deep_group(L, 20000)
    c.table, c.hashed, c.name = L, True, case.name + "+deep"
    return c


# ---- C. singleton correction -----------------------------------------------------------------------------
BUCKET_SHIFT = 10


def c_gside(deep):
    G, S = Layout(500), Layout(501)
    n = sided(G, {0: 2, 9: DD_H, 80: 3, 98: 2}, 100)       # f = 0, 1 and F - 2, F - 1 are mutual pairs
    S.add(S.fresh(), "a", *site(3))
    if deep:
        deep_group(G, n + 3)
    edges = {("g_group", 2, "first"), ("g_group", DD_H), ("g_group", 1)} | (set() if deep else {("g_group", 2, "last")})
    return Case("C-gside" + ("-deep" if deep else ""), "sc", G, edges, sscs=S, hashed=deep)


def c_buckets(deep):
    """Singletons whose SSCS partners lie at chosen places of the SSCS table's position buckets."""
    W = 1 << BUCKET_SHIFT
    G, S = Layout(510), Layout(511)

    def at(p):
        return (0, p), (1, p)

    def both(p):
        bc = S.fresh()
        S.add(bc, "a", *at(p))
        G.add(R.swap_barcode(bc), "b", *at(p))

    def only_s(p):
        S.add(S.fresh(), "a", *at(p))

    def only_g(p):
        G.add(dotted(5000 + p), "b", *at(p))

    both(W), both(2 * W - 1)                           # a bucket's first and last position
    only_s(2 * W + 5), only_g(3 * W + 7), only_s(4 * W + 5)    # an empty bucket between two occupied ones
    dense = [6 * W + d for d in (1, 3, 9, 20, 33, 50)]
    for k, p in enumerate(dense):                      # six positions in one bucket: first, middle, last
        both(p) if k in (0, 3, 5) else only_s(p)
    only_g(6 * W + 15)                                 # absent between two present
    both(20 * W + 3)                                   # the table's last position (on chr2: the last bucket)
    only_g(30 * W + 1)                                 # beyond it
    G.add(dotted(9000), "a", (2, 500), (2, 1500))      # a contig the SSCS table has no record on
    edges = {("bucket", k) for k in ("first", "last", "empty", "dense_first", "dense_middle", "dense_last",
                                     "dense_absent", "beyond", "no_contig", "last_bucket")}
    if deep:                                            # the same lookups hashed: the buckets are not in use
        deep_group(S, 9000 // 40)
        edges = {("s_hashed",)}
    return Case("C-buckets" + ("-deep" if deep else ""), "sc", G, edges, sscs=S, s_hashed=deep)


def c_decisions():
    G, S = Layout(520), Layout(521)
    for k, first in enumerate("xy"):                   # both singletons there, and y's tag an SSCS family too
        a, b = site(k)
        bc = G.fresh()
        G.add(bc, "a", a, b, order=0 if first == "x" else 1)
        G.add(R.swap_barcode(bc), "b", a, b, order=1 if first == "x" else 0)
        S.add(R.swap_barcode(bc), "b", a, b)
    mutual(G, 2)
    n = 3
    for hops in (1, 2, 3, 4):
        for far in FAR:
            chain(G, n, hops, far, 9)
            n += 1
    S.add(S.fresh(), "a", *site(n))
    return Case("C-decisions", "sc", G, {("sscs_wins", "x"), ("sscs_wins", "y"), ("mutual", 2)} |
                {("chain", h, f) for h in (1, 2, 3, 4) for f in FAR}, sscs=S)


def c_chain(hops):
    G, S = Layout(530 + hops), Layout(531)
    n = sided(G, {}, 5)
    chain(G, n, hops, "present", 37)
    chain(G, n + 1, hops - 1, "absent", 37)
    S.add(S.fresh(), "a", *site(1))
    return Case("C-chain-%d" % hops, "sc", G, {("chain", hops, "present")}, sscs=S,
                engine_error="CC_E_UNSUPPORTED" if hops > DUPLEX_CHAIN else None)


def c_small(empty):
    G, S = Layout(540), Layout(541)
    sided(G, {2: 3}, 8)
    bc = G.fresh()
    G.add(bc, "a", *site(20))
    if not empty:
        S.add(R.swap_barcode(bc), "b", *site(20))
    return Case("C-sscs-%s" % ("empty" if empty else "one"), "sc", G, {("sscs_families", 0 if empty else 2)}, sscs=S)


def class_c():
    return [c_gside(False), c_gside(True), c_buckets(False), c_buckets(True), c_decisions(), c_chain(DUPLEX_CHAIN),
            c_chain(DUPLEX_CHAIN + 1), c_small(False), c_small(True)]


# ---- D. bed files ----------------------------------------------------------------------------------------
CUT = 5000
DCS_BED = ((0, 0, CUT), (1, 0, 1 << 27), (0, CUT, 1 << 27))       # chr1's later part is read after chr2
SC_BED = ((0, 0, CUT), (0, CUT, 1 << 27), (1, 0, 1 << 27))        # two regions of one chromosome run, then chr2


def bed_text(regions):
    return "".join("%s\t%d\t%d\tr%d\n" % (CONTIGS[t][0], a, b, k) for k, (t, a, b) in enumerate(regions))


def d_bed(raising):
    """Molecules of sites before CUT complete in region 1, the others in region 2; a stray chr1 record
    before CUT completes a later site's chr2 end in region 1."""
    L = Layout(600 + raising)
    for i in range(6):
        filler(L, i)
        filler(L, 140 + i)
    mutual(L, 50)
    mutual(L, 150)
    if raising:                                   # a processed partner of an earlier region: the reference's KeyError
        a, b = site(120)
        bc = L.fresh()
        L.add(bc, "a", a, b, stray=((0, 100), 0))
        L.add(R.swap_barcode(bc), "b", a, b)
        return Case("D-bed-keyerror", "dcs", L, {("bed", "dcs", "keyerror")}, error="KeyError", regions=DCS_BED)
    # the partner an orphan tag of an earlier region: a DCS with it
    a, b = site(120)
    bc = L.fresh()
    L.add(bc, "a", a, b, order=0, stray=((0, 100), 0))
    L.add(bc, None, a, b, order=1, flags=(99, 163), stray=((0, 100), 0))
    L.add(R.swap_barcode(bc), None, a, b, order=2, flags=(145, 97))
    # the partner an orphan tag of a later region: not there yet, an SSCS singleton
    a, b = site(130)
    bc = L.fresh()
    L.add(bc, "a", a, b, order=0)
    L.add(bc, None, a, b, order=1, flags=(99, 131))
    L.add(R.swap_barcode(bc), None, a, b, order=2, flags=(145, 97), stray=((0, 140), 0))
    return Case("D-bed", "dcs", L, {("bed", "dcs", "partner_earlier"), ("bed", "dcs", "partner_later")},
                regions=DCS_BED, not_ran=("k_ht_insert", "k_bucket_geom"))     # (observed: the grouping stays local)


def c_bed():
    """Molecules with both ends on chr1, the later end past CUT, complete in region 1; a stray record
    completes the first end's tag in region 0."""
    G, S = Layout(610), Layout(611)
    far = 6000

    def at(p):
        return (0, p), (0, p + far)

    for i in range(4):
        G.add(G.fresh(), "ab"[i % 2], (0, 1000 + 40 * i), (0, 3000 + 40 * i))      # complete in region 0
        G.add(G.fresh(), "ab"[i % 2], *at(1200 + 40 * i))                           # in region 1
        S.add(S.fresh(), "a", *at(1400 + 40 * i))
    bc = S.fresh()                                 # the SSCS partner read by a later region: uncorrected
    S.add(bc, "a", *at(2000))
    G.add(R.swap_barcode(bc), "b", *at(2000), stray=((0, 200), 1))
    bc = S.fresh()                                 # the SSCS partner read by an earlier region
    S.add(bc, "a", *at(2400), stray=((0, 240), 1))
    G.add(R.swap_barcode(bc), "b", *at(2400))
    bc = G.fresh()                                 # the singleton partner created by a later / an earlier region
    G.add(bc, "a", *at(2800), stray=((0, 280), 1))
    G.add(R.swap_barcode(bc), "b", *at(2800))
    for k in range(2):                             # the same region: corrected by the SSCS, by the singleton
        bc = S.fresh()
        S.add(bc, "a", *at(3200 + 40 * k))
        G.add(R.swap_barcode(bc), "b", *at(3200 + 40 * k))
        bc = G.fresh()
        G.add(bc, "a", *at(3600 + 40 * k))
        G.add(R.swap_barcode(bc), "b", *at(3600 + 40 * k))
    bc = S.fresh()                                 # the second chromosome run
    S.add(bc, "a", (1, 1000), (1, 1400))
    G.add(R.swap_barcode(bc), "b", (1, 1000), (1, 1400))
    edges = {("bed", "sc", k) for k in ("sscs_later", "sscs_earlier", "single_later", "single_earlier", "second_run")}
    return Case("C-bed", "sc", G, edges, sscs=S, regions=SC_BED, ran=("k_bucket_geom",), not_ran=("k_ht_insert",))    # (observed)


def class_d():
    return [d_bed(False), d_bed(True), c_bed()]


# ---- all ----------------------------------------------------------------------------------------------------
def all_cases():
    """Every case with its tables built: the DCS cases also with a deep group appended (hashed)."""
    dcs = class_a() + class_a_f() + class_b()
    out = dcs + [hashed(c) for c in dcs] + [hashed(c) for c in class_h()] + class_c() + class_d()
    for c in out:
        c.table = c.table.table()
        if c.sscs is not None:
            c.sscs = c.sscs.table()
        assert len(c.table) <= 3200, (c.name, len(c.table))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
