"""The cases of tests/test_gpu_group_edges.py (read_bam's read-end grouping against tests/group_refs.py)
and of tests/test_group_refs.py (group_refs against the Python oracle): tables of proper pairs laid out by
record index (pair_cases.Layout) so that position groups, families and csn entries fall on the edges of
the grouping kernels' geometry.

The kernel constants are mirrored here (test_group_refs.py checks them against csrc/cc_engine.hip); every
edge is derived from them.  A case's `edges` are what its builder placed; test_group_refs.py derives them
again from the finished table.

Not built: more deep position groups than k_deep_fam's grid (CC_DF_GRID = 8192 blocks: 8193 groups of 65
records are 532,545 records, past the 20,000 a table here may hold)."""
import numpy as np

import group_refs as R
import pair_cases as PC

# ---- mirrored from csrc/cc_engine.hip -----------------------------------------------------------
GT = 256             # records per ranking tile
GH = 64              # halo records staged on either side
GRP_SMALL = 64       # a position group of more records is deep
GC_TILES = 4         # tiles per k_group_count block (a wave each, 4 records per lane)
DF_T = 512           # k_deep_fam threads: a sub-round's records
DF_U, DF_U3 = 4, 2   # sub-rounds per round of k_deep_fam's table and placement phases
DF_SLOTS = 1024      # k_deep_fam's hash table
DF_FAMS = 512        # families a deep group may hold to be ranked in place
DF_SORT = 8192       # ends a family may hold for k_deep_sortfam
DF_ST = 512          # k_deep_sortfam threads (its store loop takes 4 * DF_ST slots a turn)
DF_GRID = 8192       # k_deep_fam blocks
CT = 1024            # creation entries per k_csn_fast tile
CW = 128             # and its window before the tile

DEEP_MIN = GRP_SMALL + 1
WAVE = 64
PLACE_SIZES = (1, 2, GRP_SMALL - 1, GRP_SMALL, GRP_SMALL + 1)
STRADDLE_K = (1, GH // 2 - 1, GH // 2, GH // 2 + 1, GH - 1)
TABLE_SIZES = (2, GT - 1, GT, GT + 1, GC_TILES * GT - 1, GC_TILES * GT, GC_TILES * GT + 1, GC_TILES * GT + 3)
DEEP_SIZES = (DEEP_MIN, DF_T - 1, DF_T, DF_T + 1, 2 * DF_T - 1, 2 * DF_T, 2 * DF_T + 1,
              DF_U * DF_T - 1, DF_U * DF_T, DF_U * DF_T + 1)
FAMS_PER_GROUP = (1, 2, DF_FAMS - 1, DF_FAMS, DF_FAMS + 1)
EMIT_SIZES = (1, 2, WAVE - 1, WAVE)
SORTFAM_SIZES = (WAVE + 1, DF_ST - 1, DF_ST, DF_ST + 1, 4 * DF_ST, 4 * DF_ST + 1, DF_SORT, DF_SORT + 1)
S4 = [(4, 4), (0, 4)]    # 4S4M: another cigar of READ_LEN bases
FREE_BC = 1 << 14        # barcode numbers from here on are given out by link number

Case = PC.Case


def bc(k):
    """Barcode number k (below 65,536) as four and four letters."""
    s = "".join("ACGT"[(k >> (2 * i)) & 3] for i in range(8))
    return s[:4] + "." + s[4:]


class GLayout(PC.Layout):
    """pair_cases.Layout with a barcode number, the two flags and the two cigars per pair, reads that a
    filter takes out, and optionally the position of a record of tid 0 for the first group of tid 1."""

    def __init__(self, n, tid1_from=None):
        PC.Layout.__init__(self, n, tid1_from)
        self.opts = {}          # a link's lower record -> (barcode number, flags, cigars)
        self.bad = []           # (record, flag)
        self.tid1_pos_of = None  # a record of tid 0 whose position the first group of tid 1 takes

    def pair(self, i, j, b, flags=(99, 147), cigars=(None, None)):
        """Records i < j as mates: the flag and cigar of i first."""
        assert i < j
        self.link(i, j)
        self.opts[i] = (b, flags, cigars)

    def table(self, seed=0):
        for k, (i, j, _) in enumerate(self.links):
            b = self.opts[i][0] if i in self.opts else FREE_BC + k
            self.names[i] = self.names[j] = "g%d|%s" % (k, bc(b))
        t = PC.Layout.table(self, seed)
        for i, j, _ in self.links:
            if i in self.opts:
                _, flags, cigars = self.opts[i]
                t.flag[i], t.flag[j] = flags
                t.cig[i], t.cig[j] = cigars
        for i, flag in self.bad:
            t.flag[i] = flag
        if self.tid1_pos_of is not None:
            c = int(np.flatnonzero(self.tid == 1)[0])
            inside = set(np.flatnonzero(self.gs == c).tolist())
            p = t.pos[self.tid1_pos_of]
            for r in inside:
                t.pos[r] = p
            for i, j, _ in self.links:
                if j in inside:
                    t.mpos[i] = p
                if i in inside:
                    t.mpos[j] = p
            assert t.is_sorted()
        return t


def pairs_in(L, recs, nb, b0, odd="single"):
    """The records paired two by two in their order, the barcodes b0 + (0 .. nb-1) in turn; an odd last
    one has no mate, or (odd == "out") the record after it as its mate."""
    for k in range(len(recs) // 2):
        L.pair(recs[2 * k], recs[2 * k + 1], b0 + k % nb)
    if len(recs) % 2:
        if odd == "out":
            L.pair(recs[-1], recs[-1] + 1, b0 + nb)
        else:
            L.single(recs[-1])


def family(L, xs, ys, b, flags=(99, 147), reverse=False):
    """len(xs) pairs of one barcode from the records xs to the later records ys: one family at each end.
    reverse: the first of xs with the last of ys, so that xs' record order is the reverse of end order."""
    m = len(xs)
    for k in range(m):
        L.pair(xs[k], ys[m - 1 - k] if reverse else ys[k], b, flags)


class Cursor(object):
    """Groups handed out one after the other, `gap` one-record groups between them."""

    def __init__(self, L, at=8, gap=3):
        self.L, self.at, self.gap = L, at, gap

    def take(self, g):
        a = self.at
        self.L.group(a, g)
        self.at += g + self.gap
        return list(range(a, a + g))


# ---- A. small position groups and the ranking tile ----------------------------------------------------
def a_place():
    """Groups of PLACE_SIZES records ending on a tile's last record, starting on a tile's first, and
    with k of STRADDLE_K records in the earlier tile."""
    plan = []
    for g in PLACE_SIZES:
        plan += [(g, "end", None), (g, "start", None)] + [(g, "straddle", k) for k in STRADDLE_K if k < g]
    L, edges = GLayout((len(plan) + 1) * GT + 7), set()
    for m, (g, how, k) in enumerate(plan):
        edge = (m + 1) * GT
        a = edge - g if how == "end" else edge if how == "start" else edge - k
        L.group(a, g)
        pairs_in(L, list(range(a, a + g)), 3, 10 * m, odd="out")
        edges.add(("place", g, how) if k is None else ("place", g, how, k))
    L.fill()
    return Case("A-place", L.table(1), edges)


def a_ends():
    """A 64-record group at record 0 and one ending at the last record (tile_range's lo and hi)."""
    n = 3 * GT + 37
    L = GLayout(n)
    for a in (0, n - GRP_SMALL):
        L.group(a, GRP_SMALL)
        pairs_in(L, list(range(a, a + GRP_SMALL)), 2, a)
    L.fill()
    return Case("A-ends", L.table(2), {("first", GRP_SMALL), ("last", GRP_SMALL)})


def a_flank():
    L, edges = GLayout(3 * GT), set()
    at = 100
    for mid in (GRP_SMALL, DEEP_MIN):
        other = DEEP_MIN if mid == GRP_SMALL else GRP_SMALL
        for g in (other, mid, other):
            L.group(at, g)
            pairs_in(L, list(range(at, at + g)), 2, at)
            at += g
        edges.add(("flank", mid, other))
        at += 40
    L.fill()
    return Case("A-flank", L.table(3), edges)


START_BITS = ((31, GRP_SMALL), (0, GRP_SMALL), (1, GRP_SMALL), (31, 3), (1, 2))


def a_bits():
    """Group starts at staged index 31, 0 and 1 (mod 32): GH and GT are multiples of 32, so a record's
    staged index is its record index mod 32 in every tile that stages it."""
    assert GH % 32 == 0 and GT % 32 == 0
    L, edges = GLayout(4 * GT), set()
    for m, (s, g) in enumerate(START_BITS):
        a = 128 * (m + 1) + s
        L.group(a, g)
        pairs_in(L, list(range(a, a + g)), 2, 10 * m)
        edges.add(("start_bit", s, g))
    L.fill()
    return Case("A-bits", L.table(4), edges)


def a_tid():
    c = 150
    L = GLayout(GT + 100, tid1_from=c)
    for a in (c - 4, c):
        L.group(a, 4)
        pairs_in(L, list(range(a, a + 4)), 1, 7)
    L.tid1_pos_of = c - 1
    L.fill()
    return Case("A-tid", L.table(5), {("tid_change_same_pos",)})


def a_noends():
    """Records without a read end inside groups: 66 records with 60 ends (deep), 64 with 2 (small);
    the others' mates are absent, or a filter takes them out."""
    L = GLayout(2 * GT)
    L.group(20, 66)
    out = (20, 31, 42, 53, 64, 85)
    for r in out:
        L.single(r)
    pairs_in(L, [r for r in range(20, 86) if r not in out], 3, 0)
    L.group(200, GRP_SMALL)
    L.pair(210, 250, 5)
    for r in range(200, 200 + GRP_SMALL):
        if r not in (210, 250):
            L.single(r, "no_mtid" if r == 207 else "absent")
    L.bad = [(203, 99 | 0x100), (260, 99 | 0x800)]
    L.fill()
    return Case("A-noends", L.table(6), {("noends", 66, 60), ("noends", GRP_SMALL, 2), ("badread_in_group",)})


def a_sizes():
    out = []
    for n in TABLE_SIZES:
        L, edges = GLayout(n), {("n", n)}
        if n >= 2 * GT:
            for r in range(GT, 2 * GT):
                L.single(r)
            edges.add(("empty_tile",))
        L.fill()
        out.append(Case("A-size-%d" % n, L.table(n), edges))
    return out


def class_a():
    return [a_place(), a_ends(), a_flank(), a_bits(), a_tid(), a_noends()] + a_sizes()


# ---- B. families inside small groups ------------------------------------------------------------------------
DIFFER = ("barcode", "mtid", "mpos", "cigar_a", "cigar_b", "orientation", "read_number")
TAG_FIELDS = ("barcode", "tid", "pos", "mtid", "mpos", "cigar_a", "cigar_b", "orientation", "read_number")
LRT_PLACES = ("alone", "first", "middle", "last")


def b_families():
    n, cut = 1300, 1200
    L, edges = GLayout(n, tid1_from=cut), set()
    c = Cursor(L)
    g = GRP_SMALL
    family(L, c.take(g), c.take(g), 1)
    edges.add(("one_family", g))
    for k, (x, y) in enumerate(zip(c.take(g), c.take(g))):
        L.pair(x, y, 100 + k)
    edges.add(("singletons", g))
    for nf in (2, 3):
        for k, (x, y) in enumerate(zip(c.take(g), c.take(g))):
            L.pair(x, y, 200 + 10 * nf + k % nf)
        edges.add(("interleaved", nf))
    family(L, c.take(32), c.take(32), 300, reverse=True)
    edges.add(("reversed",))
    # families of two ends at one position that differ from the first one in one field of the tag
    X, Ya, Yb = c.take(16), c.take(12), c.take(2)
    L.group(cut, 2)
    Yt = [cut, cut + 1]
    L.tid1_pos_of = Ya[0]                                         # (the other contig, the same position)
    variants = ((Ya[0:2], 400, (99, 147), (None, None)),          # the family the others differ from
                (Ya[2:4], 401, (99, 147), (None, None)),          # barcode
                (Yb, 400, (99, 147), (None, None)),               # mate position
                (Yt, 400, (99, 147), (None, None)),               # mate tid
                (Ya[4:6], 400, (83, 163), (None, None)),          # orientation
                (Ya[6:8], 400, (163, 83), (None, None)),          # read number
                (Ya[8:10], 400, (99, 147), (S4, None)),           # own cigar
                (Ya[10:12], 400, (99, 147), (None, S4)))          # mate's cigar
    for v, (ys, b, flags, cigars) in enumerate(variants):
        for k in range(2):
            L.pair(X[2 * v + k], ys[k], b, flags, cigars)
    edges |= {("differs", f) for f in DIFFER}
    # "line read twice": both ends of a pair with one tag, alone and inside a family of seven
    for where in LRT_PLACES:
        recs = c.take(2 if where == "alone" else 12)
        at = {"alone": 0, "first": 0, "middle": 2, "last": 5}[where]
        for k in range(len(recs) // 2):
            L.pair(recs[2 * k], recs[2 * k + 1], 500, (99, 99) if k == at else (99, 147))
        edges.add(("lrt", where))
    assert c.at < cut
    L.fill()
    return Case("B-families", L.table(7), edges)


def class_b():
    return [b_families()]


# ---- C. deep groups ---------------------------------------------------------------------------------------------
DEEP_RAN = ("k_group_rank", "k_deep_count", "k_deep_fam", "k_deep_emit")


def c_sizes(sizes, name, seed):
    L, edges = GLayout(sum(sizes) + 5 * len(sizes) + 20), set()
    c = Cursor(L, gap=5)
    for k, g in enumerate(sizes):
        pairs_in(L, c.take(g), 1 + 2 * (k % 3), 20 * k)
        edges.add(("deep_size", g))
    L.fill()
    return Case(name, L.table(seed), edges, ran=DEEP_RAN, not_ran=("sort_tags_big", "sort_tags"))


def c_nfam(nfs, name, seed, **kw):
    """Deep groups of exactly nf families: nf // 2 barcodes paired inside the group (two families each,
    two pairs per barcode), an odd nf's last family by a mate after the group; one family: all mates in
    a second group."""
    L, edges = GLayout(sum(max(2 * nf, DEEP_MIN) + DEEP_MIN for nf in nfs) + 60), set()
    c = Cursor(L)
    for k, nf in enumerate(nfs):
        if nf == 1:
            family(L, c.take(DEEP_MIN), c.take(DEEP_MIN), 1000)
        else:
            nb = nf // 2
            npairs = max(2 * nb, (DEEP_MIN + 1) // 2)
            recs = c.take(2 * npairs + nf % 2)
            pairs_in(L, recs, nb, 2000 * (k + 1), odd="out")
        edges.add(("nfam", nf))
    L.fill()
    return Case(name, L.table(seed), edges, **kw)


def subround_family(k):
    sr, off = k // DF_T, k % DF_T
    if sr == 1:
        return 0                                   # a whole sub-round
    if sr == 0 and off % WAVE == 5:
        return 1                                   # one end in each wave of a sub-round
    if off % 7 == 0:
        return 2                                   # sub-rounds 0, 2 and 3, others between
    return 3 + k % 3


def c_subrounds():
    g = 4 * DF_T - 100
    L = GLayout(2 * g + 40)
    c = Cursor(L)
    for k, (x, y) in enumerate(zip(c.take(g), c.take(g))):
        L.pair(x, y, 3000 + subround_family(k))
    L.fill()
    return Case("C-subrounds", L.table(23), {("whole_subround",), ("one_per_wave",), ("three_subrounds",)},
                ran=DEEP_RAN + ("k_deep_sortfam",), not_ran=("sort_tags_big", "sort_tags"))


LRT_GROUP_PAIRS = 70
LRT_CROSS_AT = 16      # pairs after the family's lowest (odd) end: bits 31 and 32 of its bitmap


def c_famsizes():
    """Families of EMIT_SIZES and WAVE + 1 ends inside one deep group, in end order and reversed (the
    mates' group holds every size in end order); a line-read-twice pair across two bitmap words and one
    that is its family's lowest end."""
    sizes = EMIT_SIZES + (WAVE + 1,)
    plan = [(s, False) for s in sizes] + [(s, True) for s in sizes if s > 1]
    g = sum(s for s, _ in plan)
    L, edges = GLayout(2 * g + 4 * LRT_GROUP_PAIRS + 60), set()
    c = Cursor(L)
    X, Y = c.take(g), c.take(g)
    at = 0
    for k, (s, rev) in enumerate(plan):
        family(L, X[at:at + s], Y[at:at + s], 4000 + k, reverse=rev)
        at += s
        for order in ("ordered", "reversed") if rev else ("ordered",):
            edges.add(("family_size", s, order))
    for first_lrt in (False, True):
        recs = c.take(2 * LRT_GROUP_PAIRS)
        for k in range(LRT_GROUP_PAIRS):
            if first_lrt:
                flags = (99, 99) if k == 0 else (99, 147)
            else:
                flags = (147, 99) if k == 0 else (99, 99) if k == LRT_CROSS_AT else (99, 147)
            L.pair(recs[2 * k], recs[2 * k + 1], 4100 + first_lrt, flags)
        edges.add(("lrt_lowest",) if first_lrt else ("lrt_word_cross",))
    L.fill()
    return Case("C-famsizes", L.table(24), edges, ran=DEEP_RAN + ("k_deep_sortfam",),
                not_ran=("sort_tags_big", "sort_tags"))


def c_sortfam(dense, sparse, name, seed, **kw):
    """Families of `dense` ends that are their whole group, and of `sparse` ends dealt record by record
    with three others; every second one with its records in reversed end order."""
    L, edges = GLayout(2 * sum(dense) + 8 * sum(sparse) + 6 * (len(dense) + len(sparse)) + 30), set()
    c = Cursor(L)
    for k, s in enumerate(dense):
        family(L, c.take(s), c.take(s), 5000 + k, reverse=k % 2 == 1)
        edges.add(("sortfam", s, "dense"))
    for k, s in enumerate(sparse):
        for j, (x, y) in enumerate(zip(c.take(4 * s), c.take(4 * s))):
            L.pair(x, y, 5100 + 4 * k + j % 4)
        edges.add(("sortfam", s, "sparse"))
    L.fill()
    kw.setdefault("ran", DEEP_RAN + ("k_deep_sortfam",))
    kw.setdefault("not_ran", ("sort_tags_big", "sort_tags"))
    return Case(name, L.table(seed), edges, **kw)


def c_mixed():
    sizes = (2, 40, DEEP_MIN, GRP_SMALL, 3, 130, 1, GRP_SMALL, 200, 17)
    L = GLayout(sum(sizes) + 3 * len(sizes) + 20)
    c = Cursor(L)
    for k, g in enumerate(sizes):
        pairs_in(L, c.take(g), 2, 50 * k)
    L.fill()
    return Case("C-mixed", L.table(25), {("mixed",)}, ran=DEEP_RAN, not_ran=("sort_tags_big", "sort_tags"))


def class_c():
    half = 7
    over = dict(ran=("k_group_rank", "k_deep_fam", "sort_tags_big"), not_ran=("sort_tags",))
    return [c_sizes(DEEP_SIZES[:half], "C-sizes-a", 20), c_sizes(DEEP_SIZES[half:], "C-sizes-b", 21),
            c_nfam(FAMS_PER_GROUP[:-1], "C-nfam", 22, ran=DEEP_RAN, not_ran=("sort_tags_big", "sort_tags")),
            # a group of DF_FAMS + 1 families is not ranked in place: the pass sorts every deep end
            c_nfam((2, FAMS_PER_GROUP[-1]), "C-nfam-over", 26, **over),
            c_subrounds(), c_famsizes(),
            c_sortfam(SORTFAM_SIZES[:6], SORTFAM_SIZES[:1] + SORTFAM_SIZES[3:4], "C-sortfam", 27),
            c_sortfam(SORTFAM_SIZES[6:7], (), "C-sortfam-max", 28),
            # a family of DF_SORT + 1 ends: EB_DEEPSORT, and the pass runs again on the sorted path
            c_sortfam(SORTFAM_SIZES[7:8], (), "C-sortfam-over", 29, ran=("k_deep_fam", "k_deep_sortfam", "sort_tags_big"),
                      not_ran=("sort_tags",)),
            c_mixed()]


# ---- D. creation order and csn_pair_dict ----------------------------------------------------------------------
D_BEFORE = 60          # the first shared pair's creation entry lies this far before a multiple of CT
SHARED_FLAGS = ((99, 147), (67, 131), (147, 99))


def d_shared(name, seed, deep=False, pairs=2, lrt=False):
    """Pairs of one molecule name and different read-end tags, both ends in one group each, the first and
    the last record of the earlier group: GRP_SMALL - 2 pairs of their own names complete between them,
    and the first one's creation entry is D_BEFORE before entry CT.  lrt: two line-read-twice pairs,
    whose one family each share an entry."""
    pre = (CT - D_BEFORE) // 2
    L, edges = GLayout(2 * pre + 2 * GRP_SMALL + 40), set()
    for k in range(pre):
        L.pair(2 * k, 2 * k + 1, 6000 + k)
    c = Cursor(L, at=2 * pre, gap=0)
    if lrt:
        X = c.take(GRP_SMALL)
        for k in range(GRP_SMALL // 2):
            flags = (99, 99) if k == 0 else (147, 147) if k == GRP_SMALL // 2 - 1 else (99, 147)
            L.pair(X[2 * k], X[2 * k + 1], 7000 if flags[0] == flags[1] else 7001 + k, flags)
        edges.add(("entry_of_two_pairs",))
    else:
        X, Y = c.take(GRP_SMALL), c.take(GRP_SMALL + (2 if deep else 0))
        at = {0: 0, 1: GRP_SMALL - 1, 2: GRP_SMALL // 2}
        shared = {at[k]: SHARED_FLAGS[k] for k in range(pairs)}
        for k in range(GRP_SMALL):
            L.pair(X[k], Y[k], 7000 if k in shared else 7001 + k, shared.get(k, (99, 147)))
        for r in Y[GRP_SMALL:]:
            L.single(r)
        span = 2 * (GRP_SMALL - 1)
        edges.add(("shared_name", "deep" if deep else "small", pairs, span, True))
        assert span < CW
    L.fill()
    return Case(name, L.table(seed), edges, ran=("k_csn_fast", "sort_csn"))


def d_regions():
    L = GLayout(4 * GT + 9)
    c = Cursor(L)
    for k, g in enumerate((GRP_SMALL, 30, DEEP_MIN, 2, GRP_SMALL, 90, 12)):
        pairs_in(L, c.take(g), 2, 40 * k)
        if k == 3:
            cut = c.at - 2                       # (a record between two groups)
    free = np.flatnonzero(~L.used)
    assert np.sum(free < cut) % 2 == 0           # fill pairs neighbours: no pair across the cut
    L.fill()
    n = L.n
    region = (np.arange(n) >= cut).astype(np.int32)
    return Case("D-regions", L.table(33), {("regions", 2)}, stream=np.arange(n), region=region, n_regions=2,
                ran=("k_group_rank", "k_csn_fast"), not_ran=("sort_csn",))


def class_d():
    return [d_shared("D-shared-small", 30), d_shared("D-shared-deep", 31, deep=True),
            d_shared("D-three-pairs", 32, pairs=3), d_shared("D-lrt-entry", 34, lrt=True), d_regions()]


# ---- E. unsorted table ---------------------------------------------------------------------------------------------
E_FAMILIES = (2, DEEP_MIN, 300)


def e_shuffled():
    L, edges = GLayout(2 * sum(E_FAMILIES) + 400), {("unsorted",)}
    c = Cursor(L)
    for k, s in enumerate(E_FAMILIES):
        family(L, c.take(s), c.take(s), 8000 + k)
        edges.add(("family", s))
    L.fill()
    t = L.table(40)
    order = np.random.default_rng(41).permutation(len(t))
    return Case("E-shuffled", t.take(order), edges, ran=("sort_tags", "k_fam_mark"),
                not_ran=("k_group_rank", "k_deep_fam", "sort_tags_big"))


def class_e():
    return [e_shuffled()]


# ---- all ----------------------------------------------------------------------------------------------------------------
STAGED_DRAW = ("A-place", "A-size-1027", "B-families", "C-sizes-a", "C-mixed", "D-shared-small", "E-shuffled")
DEEP_SORT_DRAW = ("A-flank", "B-families", "D-shared-deep", "E-shuffled")


def all_cases():
    base = []
    for cls in (class_a, class_b, class_c, class_d, class_e):
        for c in cls():
            if not c.ran:
                c.ran, c.not_ran = ("k_group_rank",), ("sort_tags",)
            c.switch = None
            base.append(c)
    out = list(base)
    for c in base:
        if c.name[0] in "ABC":
            out.append(c.with_("-bypair", env={"CC_GR_BY_PAIR": "1"}, switch="CC_GR_BY_PAIR", pipeline=False))
    for c in base:
        if c.name in STAGED_DRAW:
            out.append(c.with_("-staged", env={"CC_GROUP_STAGED": "1"}, switch="CC_GROUP_STAGED", pipeline=False))
    for c in base:
        if c.name[0] == "C" or c.name in DEEP_SORT_DRAW:
            # the deep ends by the sort: none of the in-place kernels, whatever the case was built for
            ran = tuple(k for k in c.ran if not k.startswith("k_deep_"))
            has_deep = c.name[0] == "C" or c.name in ("A-flank", "D-shared-deep")
            out.append(c.with_("-deepsort", env={"CC_DEEP_SORT": "1"}, switch="CC_DEEP_SORT", pipeline=False,
                               ran=ran + (("sort_tags_big",) if has_deep else ()),
                               not_ran=tuple(k for k in c.not_ran if k != "sort_tags_big") +
                               ("k_deep_fam", "k_deep_emit", "k_deep_sortfam")))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def grouping(case):
    """group_refs.group over the case's completed pairs: (the pairs, the reference's result)."""
    pairs, _ = case.expected()
    t = case.table
    cache = {}

    def read(i):
        if i not in cache:
            cache[i] = R.read_of(t, i)
        return cache[i]

    return pairs, R.group(pairs, read)
