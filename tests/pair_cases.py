"""The cases of tests/test_gpu_pair_edges.py (read_bam's mate search against tests/pair_refs.py) and,
in a reduced draw, of tests/test_pair_refs.py (pair_refs against the Python oracle): tables of
well-formed proper pairs built on arrays, laid out by record index in the coordinate-sorted table so
that a searcher, its mate and the mate's position group fall on the edges of the search's geometry.

The kernel constants are mirrored here (test_pair_refs.py checks them against csrc/cc_engine.hip);
every edge is derived from them.  A case's `edges` are the edges its builder placed; test_pair_refs.py
derives them again from the finished table's record indices."""
import struct

import numpy as np

import pair_refs as R

# ---- mirrored from csrc/cc_engine.hip -----------------------------------------------------------
TILES = (512, 1024)  # k_pair_coord_tile<512 | 1024>
PC_HALO = 512        # records staged before a tile
GRP_SMALL = 64       # a target group of more records is not walked
DEEP_MIN = 65        # records from which a position group is deep
PD_W = 512           # pair spans above this enter the long-pair check
PD_TILE = 2048       # stream entries per k_pair_resid block
DQ_T = 512           # k_deep_qsort threads: deep_group_end probes 16 DQ_T records
DQ_CAP = 16384       # records a deep group may hold to be bucketed
DQ_GRID = 2048       # k_deep_qsort blocks (CC_DQ_GRID)
GALLOP0 = 256        # mate_search_global's first step down, growing 4x

READ_LEN = 8
NT16 = "=ACMGRSVTWYHKDBN"
CONTIGS = (("chr1", 1 << 28), ("chr2", 1 << 28))

HALO_D = (1, 2, PC_HALO - 1, PC_HALO, PC_HALO + 1)
GALLOP_D = tuple(GALLOP0 * 4 ** k + e for k in range(4) for e in (-1, 0, 1))
# The steps add up: the gallop's probes lie 256, 1280, 5376 and 21760 below the hint.  Of GALLOP_D only
# the first three sit at a probe (the rest fall inside a step and are found by the bisection), so the
# targets also lie around the second and third probe.  The fourth probe is taken for every target more
# than 5376 below the hint and lies below all of them.
GALLOP_PROBES = tuple(sum(GALLOP0 * 4 ** j for j in range(k + 1)) for k in range(4))
GALLOP_AT_PROBES = tuple(p + e for p in GALLOP_PROBES[1:3] for e in (-1, 0, 1))
DEEP_SIZES = (DEEP_MIN, DEEP_MIN + 1, 16 * DQ_T - 1, 16 * DQ_T, 16 * DQ_T + 1, DQ_CAP, DQ_CAP + 1)
QNAME_LENS = (1, 7, 8, 9, 31, 32, 33, 40, 200)


def tile_offsets(T):
    return (0, 1, 255, 256, T - 1)


def window(s, T, n):
    """(t0, t1, w0, w1) of the tile that record s searches from: its entries and the staged range."""
    t0 = s // T * T
    t1 = min(n, t0 + T)
    return t0, t1, (t0 - PC_HALO if t0 > PC_HALO else 0), min(n, t1 + GRP_SMALL + 2)


# ---- tables ---------------------------------------------------------------------------------------
class Table(object):
    """Records as arrays: qname, tid, pos, mtid, mpos, flag, tlen and READ_LEN base codes (every quality
    40; the cigar one M unless `cig` holds (op, length) tuples for the record)."""

    def __init__(self, n, seed=0):
        self.qname = [None] * n
        self.tid = np.zeros(n, np.int32)
        self.pos = np.zeros(n, np.int32)
        self.mtid = np.zeros(n, np.int32)
        self.mpos = np.zeros(n, np.int32)
        self.flag = np.zeros(n, np.int32)
        self.tlen = np.zeros(n, np.int32)
        self.seq = np.random.default_rng(seed).choice((1, 2, 4, 8), (max(n, 1), READ_LEN)).astype(np.uint8)[:n]
        self.cig = [None] * n

    def cigar_of(self, i):
        return self.cig[i] or [(0, READ_LEN)]

    def __len__(self):
        return len(self.qname)

    def take(self, order):
        """The table with its records in another order."""
        t = Table(len(order))
        t.qname = [self.qname[i] for i in order]
        t.cig = [self.cig[i] for i in order]
        for name in ("tid", "pos", "mtid", "mpos", "flag", "tlen", "seq"):
            setattr(t, name, getattr(self, name)[np.asarray(order, np.int64)])
        return t

    def raw(self, i):
        """Record i as a BAM record (block_size first)."""
        import pysam
        c = self.seq[i]
        packed = ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()
        qn = self.qname[i].encode() + b"\x00"
        p = int(self.pos[i])
        cig = self.cigar_of(i)
        span = sum(ln for op, ln in cig if op in (0, 2, 3, 7, 8))
        body = struct.pack("<iiBBHHHiiii", int(self.tid[i]), p, len(qn), 60, pysam.reg2bin(p, p + span), len(cig),
                           int(self.flag[i]), READ_LEN, int(self.mtid[i]), int(self.mpos[i]), int(self.tlen[i]))
        body += qn + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cig) + packed + b"\x28" * READ_LEN
        return struct.pack("<i", len(body)) + body

    def header(self):
        import pysam
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
        return pysam.AlignmentHeader(text, list(CONTIGS))

    def write(self, path):
        import pysam
        pysam.write_bam_file(path, self.header(), [self.raw(i) for i in range(len(self))], level=1)

    def segment(self, i, header=None):
        """Record i as the oracle's record type."""
        import pysam
        r = pysam.AlignedSegment(header or self.header())
        r.query_name = self.qname[i]
        r.flag = int(self.flag[i])
        r.reference_id = int(self.tid[i])
        r.reference_start = int(self.pos[i])
        r.mapping_quality = 60
        r.cigartuples = list(self.cigar_of(i))
        r.next_reference_id = int(self.mtid[i])
        r.next_reference_start = int(self.mpos[i])
        r.template_length = int(self.tlen[i])
        r.query_sequence = "".join(NT16[c] for c in self.seq[i])
        r.query_qualities = [40] * READ_LEN
        return r

    # -- the sorted table's position groups
    def keys(self):
        return (self.tid.astype(np.int64) << 32) + self.pos.astype(np.int64)

    def is_sorted(self):
        k = self.keys()
        return bool(np.all(k[1:] >= k[:-1]))


class Case(object):
    """One read_bam call: the table, the stream (record per entry, region per entry, regions), the
    filters' switches, the environment, the edges the layout holds and the paths it was built for."""

    def __init__(self, name, table, edges, stream=None, region=None, n_regions=1, badread=1, delim_filter=1,
                 env=None, ran=(), not_ran=(), ran_any=(), pipeline=True):
        n = len(table)
        self.name, self.table, self.edges = name, table, set(edges)
        self.stream = np.arange(n, dtype=np.int32) if stream is None else np.asarray(stream, np.int32)
        self.region = np.zeros(len(self.stream), np.int32) if region is None else np.asarray(region, np.int32)
        self.n_regions, self.badread, self.delim_filter = n_regions, badread, delim_filter
        self.env = dict(env or {})
        self.ran, self.not_ran, self.ran_any = tuple(ran), tuple(not_ran), tuple(ran_any)
        self.pipeline = pipeline and n <= 10000 and stream is None
        self.tile = TILES[0]

    def with_(self, suffix, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name = self.name + suffix
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def expected(self):
        """pair_refs.pairs over the case's stream."""
        t = self.table
        qn = [t.qname[r] for r in self.stream]
        ps = [R.passes(t.qname[r], int(t.flag[r]), self.delim_filter, self.badread) for r in self.stream]
        return R.pairs(self.stream, self.region, qn, ps)


def barcode(k):
    b = "ACGT"
    return b[k & 3] + b[(k >> 2) & 3] + "." + b[(k >> 4) & 3] + b[(k >> 6) & 3]


class Layout(object):
    """A sorted table under construction: record i's position group (records of one (tid, pos)) and
    its mate, by record index."""

    def __init__(self, n, tid1_from=None):
        self.n = n
        self.gs = np.arange(n, dtype=np.int64)          # each record's group's first record
        self.tid = np.zeros(n, np.int32)
        if tid1_from is not None:
            self.tid[tid1_from:] = 1
        self.used = np.zeros(n, bool)
        self.links = []                                  # (i, j, wrong): mates i < j; wrong: j's mpos is off
        self.singles = []                                # (i, kind)
        self.names = {}                                  # record -> forced qname

    def group(self, a, size):
        assert a >= 0 and a + size <= self.n and np.array_equal(self.gs[a:a + size], np.arange(a, a + size)), (a, size)
        assert len(set(self.tid[a:a + size].tolist())) == 1
        self.gs[a:a + size] = a

    def link(self, i, j, wrong=False):
        i, j = (i, j) if i < j else (j, i)
        assert 0 <= i < j < self.n and not self.used[i] and not self.used[j], (i, j)
        self.used[i] = self.used[j] = True
        self.links.append((i, j, wrong))

    def single(self, i, kind="absent"):
        assert not self.used[i], i
        self.used[i] = True
        self.singles.append((i, kind))

    def fill(self):
        """Every free record paired with the next free one; an odd last one's mate is absent."""
        free = np.flatnonzero(~self.used)
        for a, b in zip(free[0::2], free[1::2]):
            self.link(int(a), int(b))
        if len(free) % 2:
            self.single(int(free[-1]))

    def table(self, seed=0):
        t = Table(self.n, seed)
        t.tid[:] = self.tid
        t.pos[:] = 100 + 4 * self.gs                     # (pos + 2 is the position of no record)
        for k, (i, j, wrong) in enumerate(self.links):
            q = self.names.get(i, "p%d|%s" % (k, barcode(k)))
            t.qname[i], t.qname[j] = q, self.names.get(j, q)
            t.mtid[i], t.mpos[i] = t.tid[j], t.pos[j]
            t.mtid[j], t.mpos[j] = t.tid[i], t.pos[i] + (2 if wrong else 0)
            t.flag[i], t.flag[j] = (99, 147) if k % 2 == 0 else (163, 83)
            if t.tid[i] == t.tid[j]:
                t.tlen[i] = t.pos[j] + READ_LEN - t.pos[i]
                t.tlen[j] = -t.tlen[i]
        for k, (i, kind) in enumerate(self.singles):
            t.qname[i] = self.names.get(i, "s%d|%s" % (k, barcode(k)))
            t.flag[i] = 99
            t.mtid[i], t.mpos[i] = (-1, -1) if kind == "no_mtid" else (t.tid[i], t.pos[i] + 2)
            t.tlen[i] = 0 if kind == "no_mtid" else 2 + READ_LEN
        assert t.is_sorted() and all(q is not None for q in t.qname)
        return t


# ---- A. tile and halo -------------------------------------------------------------------------------
def a_sizes(T):
    """Tables of 1, 2, 255, 256, 257, 2T and 4T + 37 records: neighbours paired, and in the two
    larger ones mates d records before searchers at the tile offsets, wherever d fits."""
    out = []
    for n in (1, 2, 255, 256, 257, 2 * T, 4 * T + 37):
        L, edges = Layout(n), {("n", n)}
        if n >= 2 * T:
            for tile in range(1, (n + T - 1) // T):
                for oi, off in enumerate(tile_offsets(T)):
                    d = HALO_D[(tile + oi) % len(HALO_D)]
                    s = tile * T + off
                    if s < n and s - d >= 0 and not L.used[s] and not L.used[s - d]:
                        L.link(s - d, s)
                        edges.add(("place", d, off))
        L.fill()
        out.append(Case("A-size-%d-T%d" % (n, T), L.table(n), edges))
    return out


MATRIX_TILES = 14


def a_matrix(T):
    """Every d of HALO_D at every tile offset: the mate in the own tile, in the halo, and at or before
    the staged range's first record (the global search)."""
    L, edges = Layout(MATRIX_TILES * T + 37), set()
    for di, d in enumerate(HALO_D):
        for oi, off in enumerate(tile_offsets(T)):
            # the first tile (with a staged range that does not begin the table) where both are free
            s = next(t * T + off for t in range(2, MATRIX_TILES)
                     if not L.used[t * T + off] and not L.used[t * T + off - d])
            L.link(s - d, s)
            t0, _, w0, _ = window(s, T, L.n)
            edges.add(("place", d, off))
            edges.add(("route", "own" if s - d >= t0 else "halo" if s - d > w0 else "global"))
    s = MATRIX_TILES * T + 36                                        # the partial last tile's last record
    L.link(s - 1, s)
    edges.add(("last_record",))
    L.fill()
    return Case("A-matrix-T%d" % T, L.table(1), edges)


def a_gallop(T):
    """Searchers of one tile whose targets' lower bounds lie GALLOP_D and GALLOP_AT_PROBES below the
    global search's hint (the staged range's first record), and one whose target is the table's first
    record."""
    tile = (GALLOP_PROBES[-1] + PC_HALO) // T + 2          # (the last probe lies inside the table)
    L, edges = Layout((tile + 1) * T), set()
    t0 = tile * T
    w0 = t0 - PC_HALO
    for k, d in enumerate(GALLOP_D + GALLOP_AT_PROBES):
        gs = w0 - d
        two = k % 3 == 0
        if two:
            L.group(gs, 2)                                 # the mate the group's second record
        L.link(gs + (1 if two else 0), t0 + 3 * k)
        edges.add(("gallop", d))
    L.group(0, 2)
    L.link(0, t0 + 3 * len(GALLOP_D + GALLOP_AT_PROBES))
    edges.add(("gallop_to_first",))
    L.fill()
    return Case("A-gallop-T%d" % T, L.table(2), edges)


def a_window_start(T):
    """Target groups of g records with k of them before the staged range's first record, the mate in
    the part before and in the part after."""
    combos = [(g, k, side) for g in (2, GRP_SMALL, GRP_SMALL + 1, GRP_SMALL + 2) for k in sorted({1, g - 1})
              for side in ("before", "after")]
    first = PC_HALO // T + 2
    L, edges = Layout((first + len(combos)) * T + 5), set()
    for c, (g, k, side) in enumerate(combos):
        t0 = (first + c) * T
        w0 = t0 - PC_HALO
        L.group(w0 - k, g)
        m = w0 - k if side == "before" else w0 - k + g - 1
        L.link(m, t0 + 100 + 7 * (c % 5))
        edges.add(("w0_split", g, k, side))
    L.fill()
    return Case("A-window-start-T%d" % T, L.table(3), edges)


def a_window_end(T):
    """Groups of 65 and 66 records holding both ends of their pairs (both ends search) that begin in
    the last GRP_SMALL + 2 records of a tile, and exactly at the next tile's first record."""
    combos = [(g, back) for g in (GRP_SMALL + 1, GRP_SMALL + 2) for back in (GRP_SMALL + 2, 1, 0)]
    L, edges = Layout((2 * len(combos) + 2) * T + 9), set()
    for c, (g, back) in enumerate(combos):
        t1 = (2 * c + 2) * T
        L.group(t1 - back, g)
        edges.add(("past_end", g, back))
    L.fill()
    return Case("A-window-end-T%d" % T, L.table(4), edges)


def a_one_position(T):
    """One-position groups holding both ends: 2, 3 (one odd read), 64, 65 and 66 records."""
    L, edges = Layout(T + 300), set()
    at = 10
    for g in (2, 3, GRP_SMALL, GRP_SMALL + 1, GRP_SMALL + 2):
        L.group(at, g)
        for i in range(at, at + g - 1, 2):
            L.link(i, i + 1)
        if g % 2:
            L.single(at + g - 1)
        edges.add(("same_pos", g))
        at += g + 3
    L.fill()
    return Case("A-one-position-T%d" % T, L.table(5), edges)


def a_contigs(T):
    """Mates on the other contig (only the later end searches, across the tiles between), and reads
    with a pairing flag whose mate has no contig."""
    n = 3 * T + 11
    cut = T + T // 2
    L, edges = Layout(n, tid1_from=cut), set()
    for k in range(6):
        L.link(5 + 3 * k, cut + 9 + 40 * k)
    edges.add(("other_contig",))
    L.single(2, "no_mtid")
    L.single(cut + 2, "no_mtid")
    edges.add(("no_mtid",))
    L.fill()
    return Case("A-contigs-T%d" % T, L.table(6), edges)


def class_a(T):
    return a_sizes(T) + [a_matrix(T), a_gallop(T), a_window_start(T), a_window_end(T), a_one_position(T), a_contigs(T)]


# ---- B. deep groups ---------------------------------------------------------------------------------
def b_deep(T):
    """Deep groups of DEEP_SIZES records, the table's first and last records among them, their mates
    in the same group, in another deep group and in small groups."""
    sizes = DEEP_SIZES + (DEEP_MIN, DEEP_MIN + 1)               # 65 first, 66 last
    gap = 40
    n = sum(sizes) + gap * (len(sizes) - 1)
    L, edges, starts, at = Layout(n), set(), [], 0
    for g in sizes:
        L.group(at, g)
        starts.append(at)
        at += g + gap
    edges |= {("deep_first",), ("deep_last",)}
    for k in range(len(sizes) - 1):
        a, b = starts[k], starts[k + 1]
        for j in range(20):                                   # into the next deep group
            L.link(a + 3 + 2 * j, b + 2 + 2 * j)
        for j in range(10):                                   # into the small groups between
            L.link(a + sizes[k] + 1 + j, b + sizes[k + 1] - 1 - j)
            L.link(a + 42 + j, a + sizes[k] + 11 + j)
    L.fill()                                                  # the rest: neighbours, the same group
    for g in sizes:
        edges |= {("deep", g, "same"), ("deep", g, "deep"), ("deep", g, "small")}
    return Case("B-deep-T%d" % T, L.table(7), edges, ran=("k_deep_qsort",), pipeline=False)


def b_grid(T):
    """DQ_GRID + 1 deep groups of DEEP_MIN records: k_deep_qsort's grid-stride loop takes a second
    round.  Each group pairs inside itself, its odd record with the next group's."""
    ng = DQ_GRID + 1
    L = Layout(ng * DEEP_MIN + 1)
    for k in range(ng):
        L.group(k * DEEP_MIN, DEEP_MIN)
    L.fill()
    return Case("B-grid-T%d" % T, L.table(8), {("deep_groups", ng)}, ran=("k_deep_qsort",), pipeline=False)


def class_b(T):
    return [b_deep(T), b_grid(T)]


# ---- C. stream-order semantics ------------------------------------------------------------------------
def quad(L, a, b, c, d, name):
    """Four records of one qname whose coordinates pair (a, c) and (b, d)."""
    L.link(a, c)
    L.link(b, d)
    for r in (a, b, c, d):
        L.names[r] = name


# (second - first, third - first, fourth - first) of a qname's four records a < b < c < d, whose coordinates
# pair (a, c) and (b, d) where the stream pairs (a, b) and (c, d)
C_QUADS = (
    (10, PD_W - 12, PD_W),            # both spans below PD_W
    (1, PD_W, PD_W + 1),              # both exactly PD_W
    (10, PD_W + 1, PD_W + 3),         # (a, c) long, (b, d) short
    (100, 150, 100 + PD_W + 1),       # (a, c) short, (b, d) long
    (7, PD_W + 1, PD_W + 18),         # both long
    (1, PD_W + 88, 2 * PD_W + 88),    # the later ends PD_W apart
    (1, PD_W + 88, 2 * PD_W + 89),    # and PD_W + 1
)


def quad_edge(a, b, c, d):
    return ("quad", c - a, d - b, d - c)


def c_multi():
    """Qnames seen four and three times whose coordinates pair them otherwise than the stream does."""
    L, edges = Layout(9900), set()
    at = 20
    for k, (db, dc, dd) in enumerate(C_QUADS):
        a, b, c, d = at, at + db, at + dc, at + dd
        assert a < b < c < d
        quad(L, a, b, c, d, "quad%d|AC.GT" % k)
        edges.add(quad_edge(a, b, c, d))
        at = d + 13
    # the later ends in stream slots PD_TILE - 1 and PD_TILE, and PD_W + 1 apart across that boundary
    base = (at // PD_TILE + 1) * PD_TILE
    quad(L, base - 300, base - 290, base - 1, base, "quadt|AC.GT")
    edges |= {quad_edge(base - 300, base - 290, base - 1, base), ("pd_tile_boundary", 1)}
    base += PD_TILE
    quad(L, base - 700, base - 690, base - 1, base + PD_W, "quadu|AC.GT")
    edges |= {quad_edge(base - 700, base - 690, base - 1, base + PD_W), ("pd_tile_boundary", PD_W + 1)}
    # three occurrences: coordinates pair the first with the third, the stream the first with the second
    for k, span in enumerate((30, PD_W, PD_W + 1)):
        a = base + 600 + 2 * k
        L.link(a, a + span)
        L.single(a + 7 + k)
        for r in (a, a + span, a + 7 + k):
            L.names[r] = "tri%d|AC.GT" % k
        edges.add(("triple", span))
    L.fill()
    return Case("C-multi", L.table(9), edges, ran=("k_pair_coord", "sort_qname"))


def c_apart():
    """Two pairs of one qname one after the other in the stream, their later ends PD_W and PD_W + 1
    apart: the coordinates pair them as the stream does (a re-run may or may not be taken)."""
    L, edges = Layout(2 * PD_TILE + 100), set()
    at = 10
    for k, gap in enumerate((PD_W, PD_W + 1)):
        a, c = at, at + 20
        d = c + gap
        L.link(a, c)
        L.link(d - 20, d)
        for r in (a, c, d - 20, d):
            L.names[r] = "twice%d|AC.GT" % k
        edges.add(("apart", gap))
        at = d + 10
    L.fill()
    return Case("C-apart", L.table(11), edges, ran=("k_pair_coord",))


def c_long():
    """Pairs of unique qnames spanning PD_W and PD_W + 1 entries, also across k_pair_resid's tile
    boundary: the long-pair check takes the longer ones, no re-run."""
    L, edges = Layout(2 * PD_TILE + 100), set()
    at = 10
    for span in (PD_W, PD_W + 1, PD_W, PD_W + 1):
        L.link(at, at + span)
        edges.add(("span", span))
        at += 3
    at = PD_TILE - 5
    L.link(at, at + PD_W + 1)
    L.link(at + 1, at + PD_W)
    edges.add(("span_over_pd_tile",))
    L.fill()
    return Case("C-long", L.table(10), edges, ran=("k_pair_coord",), not_ran=("sort_qname",))


def class_c():
    out = []
    for c in (c_multi(), c_apart(), c_long()):
        out.append(c)
        out.append(c.with_("-cas", env={"CC_LTAB_CAS": "1"}))
        out.append(c.with_("-lp0", env={"CC_LP_MIN": "0"}, ran=c.ran + ("k_lp_check",)))
    return out


# ---- D. residual paths --------------------------------------------------------------------------------
def d_resid(n, wrong, absent, name, triple=False, found_and_resid=False):
    """`wrong` pairs whose later end carries a wrong mpos (only the qname finds them) and `absent`
    reads without a mate, spread over the table; optionally a residual qname seen three times and a
    qname both paired by coordinates and residual."""
    L, edges = Layout(n), set()
    step = max(1, (n - 40) // max(1, wrong + absent))
    at = 3
    for k in range(wrong):
        L.link(at, at + 1 + k % 7 if at + 1 + k % 7 < n else at + 1, wrong=True)
        at += max(step, 9)
    for k in range(absent):
        while L.used[at % n]:
            at += 1
        L.single(at % n)
        at += max(step, 2)
    free = [int(i) for i in np.flatnonzero(~L.used)]
    if triple:
        a, b, c = free[5], free[40], free[90]
        L.link(a, b, wrong=True)
        L.single(c)
        for r in (a, b, c):
            L.names[r] = "rtri|AC.GT"
        edges.add(("resid_triple",))
    if found_and_resid:
        a, b, c = free[7], free[8], free[60]
        L.link(a, b)
        L.single(c)
        for r in (a, b, c):
            L.names[r] = "fres|AC.GT"
        edges.add(("found_and_resid",))
    L.fill()
    resid = 2 * sum(1 for _, _, w in L.links if w) + len(L.singles)
    # (pairs and reads of a qname of their own: the triples above are counted apart)
    edges |= {("wrong_mpos", sum(1 for i, _, w in L.links if w and i not in L.names)),
              ("absent", sum(1 for i, _ in L.singles if i not in L.names)), ("resid", resid, n)}
    edges.add(("resid_many",) if resid > n // 4 else ("resid_few",))
    return Case(name, L.table(12), edges)


def class_d():
    n = 2400
    few = d_resid(n, 100, 50, "D-few")                                    # 250 residual of 2400: the table
    below = d_resid(n, 250, 100, "D-quarter")                             # 600 of 2400: S / 4 exactly, the table still
    above = d_resid(n + 1, 250, 100, "D-over-quarter")                    # 601 of 2401: the sorted probe
    assert ("resid", n // 4, n) in below.edges and ("resid", n // 4 + 1, n + 1) in above.edges
    tri = d_resid(n, 100, 50, "D-triple", triple=True)
    fres = d_resid(n, 100, 50, "D-found-and-resid", found_and_resid=True)
    coord = dict(ran=("k_pair_coord", "k_pair_resid", "k_pair_mark"))
    out = [few.with_("", not_ran=("sort_qname", "sort_qname_resid"), **coord),
           below.with_("", not_ran=("sort_qname", "sort_qname_resid"), **coord),
           above.with_("", ran=coord["ran"] + ("sort_qname_resid",), not_ran=("sort_qname",)),
           tri.with_("", ran=coord["ran"] + ("sort_qname_resid",), not_ran=("sort_qname",)),
           fres.with_("", ran=coord["ran"] + ("sort_qname",))]
    # the same inputs with the residual keys compacted by the scan, and paired by the residual's sort:
    # the paths of the default runs, but the sort where CC_RESID_SORT asks for it; a re-run on the
    # exact sort path (sort_qname) would be a quiet fallback
    out += [few.with_("-scan", env={"CC_RESID_SCAN": "1"}, not_ran=("sort_qname", "sort_qname_resid"), **coord),
            few.with_("-sort", env={"CC_RESID_SORT": "1"}, ran=coord["ran"] + ("sort_qname_resid",),
                      not_ran=("sort_qname",)),
            tri.with_("-scan", env={"CC_RESID_SCAN": "1"}, ran=coord["ran"] + ("sort_qname_resid",),
                      not_ran=("sort_qname",)),
            tri.with_("-sort", env={"CC_RESID_SORT": "1"}, ran=coord["ran"] + ("sort_qname_resid",),
                      not_ran=("sort_qname",)),
            fres.with_("-scan", env={"CC_RESID_SCAN": "1"}, ran=coord["ran"] + ("sort_qname",)),
            fres.with_("-sort", env={"CC_RESID_SORT": "1"}, ran=coord["ran"] + ("sort_qname",))]
    return out


# ---- E. streams and filters -----------------------------------------------------------------------------
def e_streams(T):
    base = a_matrix(T)
    t = base.table
    n = len(t)
    rng = np.random.default_rng(21)
    keep = np.ones(n, bool)
    mates = {}
    for i, q in enumerate(t.qname):
        mates.setdefault(q, []).append(i)
    pairs = [v for v in mates.values() if len(v) == 2]
    for k in rng.choice(len(pairs), len(pairs) // 5, replace=False):      # found mates left out
        keep[pairs[k][0 if k % 2 else 1]] = False
    for tile in range(1, n // T, 3):                                       # whole tile-edge ranges left out
        keep[tile * T - 3: tile * T + 2] = False
    stream = np.flatnonzero(keep).astype(np.int32)
    edges = {("subset", int(len(stream))), ("left_out_found_mate",), ("left_out_searcher",), ("left_out_tile_edge",)}
    one = Case("E-subset-T%d" % T, t, edges, stream=stream, ran=("k_pair_coord",), not_ran=("sort_qname",))
    half = len(stream) // 2
    two = Case("E-subset-2regions-T%d" % T, t, edges | {("regions", 2)}, stream=stream,
               region=(np.arange(len(stream)) >= half).astype(np.int32), n_regions=2,
               ran=("k_pair_coord",), not_ran=("sort_qname",))
    again = np.concatenate([np.arange(n), [5, 6, 2 * T + 1, n - 1]]).astype(np.int32)
    twice = Case("E-overlap-T%d" % T, t, {("entered_twice", 4)}, stream=again, ran=("sort_qname",),
                 not_ran=("k_pair_coord",))
    order = rng.permutation(n)
    shuffled = Case("E-shuffled-T%d" % T, t.take(order), {("unsorted",)}, ran=("sort_qname",),
                    not_ran=("k_pair_coord",))
    return [one, two, twice, shuffled]


INTERLOPERS = (("unmapped", 99 | 4), ("mate_unmapped", 73), ("secondary", 99 | 0x100), ("supplementary", 99 | 0x800))


def e_filters(T):
    """Filtered records inside the target group, each with the qname of a live pair whose later end
    searches that group; and one without the delimiter (its qname can be no live one)."""
    L = Layout(T + 400)
    groups = []
    at = 20
    for k in range(len(INTERLOPERS) + 1):
        L.group(at, 4)
        L.link(at + 1, at + 300 + 2 * k)                                   # the live pair: mate in the group
        groups.append(at)
        at += 11
    for g in groups:
        L.single(g + 2)                                                    # the interloper's slot
    L.fill()
    t = L.table(13)
    edges = set()
    for (kind, flag), g in zip(INTERLOPERS, groups):
        t.qname[g + 2] = t.qname[g + 1]
        t.flag[g + 2] = flag
        t.mtid[g + 2], t.mpos[g + 2], t.tlen[g + 2] = t.mtid[g + 1], t.mpos[g + 1], t.tlen[g + 1]
        edges.add(("interloper", kind))
    g = groups[-1]
    t.qname[g + 2] = "nodelimiter"
    t.mtid[g + 2], t.mpos[g + 2] = t.mtid[g + 1], t.mpos[g + 1]
    edges.add(("interloper", "no_delimiter"))
    bad1 = Case("E-filters-bad1-T%d" % T, t, edges, badread=1, ran=("k_pair_coord",), not_ran=("sort_qname",))
    # without a bad-read file every entry pairs: the searcher finds its qname twice in the target group,
    # so all three are residual, and a residual qname seen three times takes the residual's sort
    bad0 = Case("E-filters-bad0-T%d" % T, t, edges, badread=0, ran=("k_pair_coord", "sort_qname_resid"),
                not_ran=("sort_qname",), pipeline=False)
    return [bad1, bad0]


def class_e(T):
    return e_streams(T) + e_filters(T)


# ---- F. qname bytes ---------------------------------------------------------------------------------------
def qname_of_length(n, k):
    """A qname of n bytes with the delimiter and a barcode where they fit, distinct per k."""
    if n == 1:
        return "|"
    tail = "|" + barcode(k)[:max(0, min(5, n - 2))]
    head = ("%dx" % k) * n
    return head[:n - len(tail)] + tail


def class_f():
    L = Layout(1500)
    edges = set()
    at = 10
    for k, n in enumerate(QNAME_LENS):                       # each length: a near pair and a halo-distance pair
        L.link(at, at + 2)
        L.names[at] = L.names[at + 2] = qname_of_length(n, k)
        if n > 1:                                            # (one byte: the delimiter alone, one qname)
            L.link(at + 1, at + 1 + PC_HALO + 40)
            L.names[at + 1] = L.names[at + 1 + PC_HALO + 40] = qname_of_length(n, k + 50)
        edges.add(("qname_len", n))
        at += 5
    # one target group of near-identical qnames, their mates searching it from later records
    g = 100
    near = ["x" * 32 + "1|AC.GT", "x" * 32 + "2|AC.GT", "y" * 31 + "|AC.GT", "y" * 31 + "|AC.GTA", "abc|AC.GT",
            "abc|AC.GTA", "abc|AC.G", "y" * 30 + "|AC.GT"]
    L.group(g, len(near))
    for k, q in enumerate(near):
        s = g + 200 + 3 * k
        L.link(g + k, s)
        L.names[g + k] = L.names[s] = q
    edges |= {("equal_first_32",), ("equal_but_length",)}
    L.fill()
    base = Case("F-qnames", L.table(14), edges, ran=("k_pair_coord",), not_ran=("sort_qname",))
    # 10 digest bits: 1,500 qnames share 1,024 keys, so two found pairs with one key are certain, and the
    # check for a qname in two found pairs (which knows keys, not bytes) sends the pass to the sort path
    # before k_pair_mark's qname compare raises the collision: sort_qname runs here by design
    return [base, base.with_("-qdig10", env={"CC_QDIG_BITS": "10"}, ran=("k_pair_coord", "sort_qname"), not_ran=())]


# ---- all ----------------------------------------------------------------------------------------------------
def all_cases():
    out = []
    for T in TILES:
        env = {} if T == TILES[0] else {"CC_PC_TILE": str(T)}
        for c in class_a(T) + class_b(T):
            if not c.ran:
                c.ran, c.not_ran = ("k_pair_coord",), ("sort_qname",)
            else:
                c.ran, c.not_ran = c.ran + ("k_pair_coord",), ("sort_qname",)
            c.tile = T
            c.env = dict(env)
            out.append(c)
    for c in class_c() + class_d() + class_e(TILES[0]) + class_f():
        c.tile = TILES[0]
        out.append(c)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
