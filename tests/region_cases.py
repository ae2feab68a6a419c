"""The cases of tests/test_gpu_region_edges.py (the bed-region loops' entries, emission order and
KeyErrors against tests/region_refs.py) and of tests/test_region_refs.py (their edges, and the oracle's
verdict on each): tiny motifs tiled along one long contig.

A motif is the at most 20 records and 2-3 bed lines of one oracle/fuzz_csn_tiny.py seed (qnames seen
three and four times, overlapping regions, records fetched twice).  Copy k is shifted by k * PITCH bases
and gets its own qnames and its own bed line names, so copies share no read-end key, no qname and no
region: a clean motif stays clean and a raising one raises in its own copy only.  What a copy adds to
the entry and family counts is its motif's, so a chosen entry or family is placed on a 256-thread
block's edge by the counts of the copies before it.

The bed lines come in two orders: "blocked" (copy 0's lines, then copy 1's, ...) and "interleaved" (every
copy's first line, then every copy's second, ...), which puts an entry's creating and completing regions
a whole pass over the contig apart, so the emission order moves entries across the whole array.  A third,
"grouped", interleaves inside runs of GROUP copies: entries completed in a later region than created,
which the full interleave creates in its first pass only, then lie in every block of entries.

Families are indexed by the engine in (position, seeded hash) order: a copy's families are a contiguous
index range, and inside it only a family alone at its position has an index of its own.  The DCS
KeyError motif is one whose deleted family is such a family."""
import collections
import os
import tempfile

import group_refs as G
import pair_refs as PR
import region_refs as RR

BLOCK = 256          # threads per block of k_csn_entries, k_emit_keys, k_overlap_keyerror, k_deleted_late
PITCH = 1000         # bases between two copies (a motif lies in 0 .. 400)
GROUP = 16           # copies per run of the "grouped" bed order
CONTIG = ("chr1", 1 << 28)

_motifs = {}


HAND = {
    # duplex names, no record streamed twice.  Two records of one qname at one position pair in the first
    # region and create the family there; the DCS loop deletes it at that region's end; a second molecule
    # of the same barcode whose end at that position waited in pair_dict completes in the second region
    # and reads the deleted list.  "late-first": the deleted family is the motif's first by position,
    # "late-last": its last (the regions the other way round).
    "late-first": ([("AC.GT_q0", 99, 100, 300), ("AC.GT_q0", 99, 100, 300), ("AC.GT_q1", 99, 100, 300),
                    ("AC.GT_q0", 147, 300, 100), ("AC.GT_q1", 147, 300, 100)], [(0, 250), (250, 400)]),
    "late-last": ([("AC.GT_q0", 99, 100, 300), ("AC.GT_q1", 99, 100, 300), ("AC.GT_q0", 147, 300, 100),
                   ("AC.GT_q0", 147, 300, 100), ("AC.GT_q1", 147, 300, 100)], [(250, 400), (0, 250)]),
}
HAND_SEQ = ("ACGTACGTAC", "ACGTACGTAA", "ACGTTCGTAC", "TCGTACGTAC", "ACGTACCTAC")


class Motif(object):
    """One seed's records (as the pysam stand-in reads them back) and bed regions, or a hand-made motif's:
    (qname, flag, pos, mpos, tlen, cigar, sequence, qualities) per record."""

    def __init__(self, seed, duplex):
        self.seed, self.duplex = seed, duplex
        if seed in HAND:
            assert duplex
            rows, self.beds = HAND[seed]
            self.recs = [(q, flag, pos, mpos, 210 if mpos > pos else -210, ((0, 10),), HAND_SEQ[k], [35] * 10)
                         for k, (q, flag, pos, mpos) in enumerate(rows)]
            return
        import fuzz_csn_tiny
        import pysam
        with tempfile.TemporaryDirectory() as tmp:
            bam, bed = os.path.join(tmp, "m.bam"), os.path.join(tmp, "m.bed")
            fuzz_csn_tiny.build(seed, bam, bed, duplex=duplex)
            self.recs = [(r.query_name, r.flag, r.reference_start, r.next_reference_start, r.template_length,
                          tuple(r.cigartuples), r.query_sequence, list(r.query_qualities))
                         for r in pysam.AlignmentFile(bam, "rb").fetch(until_eof=True)]
            self.beds = [tuple(int(x) for x in line.split("\t")[1:3]) for line in open(bed)]


def motif(seed, duplex=False):
    if (seed, duplex) not in _motifs:
        _motifs[seed, duplex] = Motif(seed, duplex)
    return _motifs[seed, duplex]


class Tiled(object):
    """Copies of motifs along the contig with their bed lines blocked, interleaved, or "grouped":
    interleaved inside each run of GROUP copies, one run after the other."""

    def __init__(self, name, seeds, order="blocked", duplex=False, kind="clean", sscs=None):
        assert order in ("blocked", "interleaved", "grouped")
        self.name, self.seeds, self.order, self.duplex, self.kind = name, list(seeds), order, duplex, kind
        self.mode = "per_region" if duplex else "sscs"
        self.sscs = sscs          # singleton correction: the SSCS side's table (this one is the singletons')
        self.reads, self.extra, self.copy_of = [], [], []
        lines = []
        for k, seed in enumerate(self.seeds):
            m = motif(seed, duplex)
            for q, flag, pos, mpos, tlen, cigar, seq, quals in m.recs:
                q = q.replace("_q", "_c%dq" % k) if duplex else "c%d" % k + q
                self.reads.append(G.Read(q, flag, 0, pos + k * PITCH, 0, mpos + k * PITCH, tlen, cigar, seq))
                self.extra.append(quals)
                self.copy_of.append(k)
            lines += [(j, k, s + k * PITCH, e + k * PITCH) for j, (s, e) in enumerate(m.beds)]
        if order == "interleaved":
            lines.sort()
        elif order == "grouped":
            lines.sort(key=lambda x: (x[1] // GROUP, x[0], x[1]))
        self.regions = [(s, e, "c%dr%d" % (k, j)) for j, k, s, e in lines]
        self._result = None

    def __len__(self):
        return len(self.reads)

    # -- files
    def header(self):
        import pysam
        return pysam.AlignmentHeader("@HD\tVN:1.4\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n@RG\tID:A\n" % CONTIG, [CONTIG])

    def write(self, bam, bed):
        import pysam
        header = self.header()
        segs = []
        for rd, quals in zip(self.reads, self.extra):
            r = pysam.AlignedSegment(header)
            r.query_name, r.flag, r.reference_id, r.reference_start = rd.qname, rd.flag, rd.tid, rd.pos
            r.mapping_quality = 60
            r.cigartuples = list(rd.cigar)
            r.next_reference_id, r.next_reference_start, r.template_length = rd.mtid, rd.mpos, rd.tlen
            r.query_sequence = rd.seq
            r.query_qualities = quals
            r.set_tag("RG", "A")
            segs.append(r)
        pysam.write_bam_file(bam, header, segs, 1)
        with open(bed, "w") as f:
            for s, e, name in self.regions:
                f.write("%s\t%d\t%d\t%s\tgneg\n" % (CONTIG[0], s, e, name))

    # -- the stream and the restatement over it
    def stream(self):
        """(record, region) per stream entry: each bed line's records in file order, start <= pos < end."""
        by_copy = collections.defaultdict(list)
        for i, k in enumerate(self.copy_of):
            by_copy[k].append(i)
        rec, reg = [], []
        for n, (s, e, _) in enumerate(self.regions):
            for i in by_copy[s // PITCH]:
                if s <= self.reads[i].pos < e:
                    rec.append(i)
                    reg.append(n)
        return rec, reg

    def pairs(self):
        rec, reg = self.stream()
        return PR.pairs(rec, reg, [self.reads[i].qname for i in rec], [True] * len(rec))[0]

    def result(self):
        if self._result is None:
            pairs = self.pairs()
            self._result = (pairs, RR.region_loop(pairs, lambda i: self.reads[i], self.mode))
        return self._result


def profile(seed, duplex=False):
    """One copy of a motif under the restatement: its entries E, the first raising pair (error) and that
    pair's way: "twice" (a record of it streamed before: fetched by two overlapping regions) or "waited"
    (its first end waited in pair_dict since an earlier region)."""
    t = Tiled("m%s" % seed, [seed], duplex=duplex)
    pairs, g = t.result()
    out = dict(E=len(g.names), error=g.error, way=None)
    if g.error is not None:
        rec, reg = t.stream()
        pending, at_of = {}, []
        for at, i in enumerate(rec):
            q = t.reads[i].qname
            if q in pending:
                at_of.append((pending.pop(q), at))
            else:
                pending[q] = at
        x, y = at_of[g.error]
        assert (rec[x], rec[y]) == pairs[g.error][:2]
        twice = rec[:x].count(rec[x]) > 0 or rec[:y].count(rec[y]) > 0
        assert twice or reg[x] < reg[y]
        out["way"] = "twice" if twice else "waited"
    return out


# ---- the motifs in use (tests/test_region_refs.py pins every one of them to the oracle) ------------------------
# The SSCS-named clean motifs are those whose SSCS output also passes the DCS, SC and DCS-SC stages (most
# seeds' outputs raise there: their consensus reads share tags across regions in their own ways), so a
# clean case runs the whole pipeline.
SPLIT = (974, 467, 3530)          # clean: an entry completed in a later region than the one that created it
RESTART = (584, 2367)             # clean: a name's entry deleted, then started anew by a later region
PLAIN = (1, 4, 234)               # clean: no consensus tag with events in two regions (234: two orphan tags)
ONE = 79                          # clean: one entry
UNSHARED = 167                    # clean: no consensus tag shared by two pairs (twelve entries)
P_RESTART = (193, 859, 1341, 1953, 2092, 3251)   # duplex names, clean: a name's entries split by region
P_PLAIN = (1, 6)
P_FILL = ((58, 10), (24, 4), (231, 1))   # duplex names, clean, no record streamed twice: (seed, families)
# raising, one deleted family read once: the offending entry is the motif's first / its last
K_TWICE_FIRST, K_WAITED_FIRST, K_WAITED_FIRST_B, K_TWICE_LAST = 61, 52, 220, 1876
EXTRA_SEEDS = (K_TWICE_LAST, 2092, 3251, 467, 3530, 2367)     # beyond the fuzz range that tests/test_region_refs.py pins anyway
HAND_SEEDS = tuple(sorted(HAND))


def entries_of(seed, duplex=False):
    return profile(seed, duplex)["E"]


def fill_entries(n, seeds=SPLIT + PLAIN):
    """Clean motifs of exactly n entries in all: the given ones in turn while they fit, then one-entry motifs."""
    out, k = [], 0
    while n >= max(entries_of(s) for s in seeds):
        out.append(seeds[k % len(seeds)])
        n -= entries_of(out[-1])
        k += 1
    return out + [ONE] * n


def fill_families(n):
    out = []
    for seed, f in P_FILL:
        out += [seed] * (n // f)
        n %= f
    assert n == 0
    return out


def clean_sscs(name, order, lead, reps):
    return Tiled(name, list(lead) + list(SPLIT + PLAIN + RESTART) * reps, order)


# motifs in front shift every later entry: chosen (test_every_edge_is_present checks the outcome) so that
# entries completed in a later region sit at 256 j - 1 and at 256 j.  Under the interleaved bed every
# such entry is created by the first pass over the contig, so they fill the first blocks only.
# The grouped bed keeps them GROUP copies' lines apart and puts some in every block.
LEAD = {"blocked": [ONE], "interleaved": [], "grouped": [ONE] * 7}
REPS = 32
SMALL = tuple((e, order) for e in (255, 256, 257) for order in ("blocked", "interleaved"))


def all_cases():
    out = [clean_sscs("S-%s" % order, order, LEAD[order], REPS) for order in ("blocked", "interleaved", "grouped")]
    for e, order in SMALL:
        out.append(Tiled("S-small-%d-%s" % (e, order), fill_entries(e), order))
    for order in ("blocked", "interleaved"):
        out.append(Tiled("P-%s" % order, list(P_RESTART + P_PLAIN) * 14, order, duplex=True))
    out.append(Tiled("S-fast", [UNSHARED] * 228, "blocked", kind="fast"))
    tail = fill_entries(40)
    out.append(Tiled("K-entry-0", [K_WAITED_FIRST] + fill_entries(300), kind="keyerror"))
    out.append(Tiled("K-entry-255", fill_entries(255) + [K_TWICE_FIRST] + tail, kind="keyerror"))
    out.append(Tiled("K-entry-256", fill_entries(256) + [K_WAITED_FIRST_B] + tail, kind="keyerror"))
    out.append(Tiled("K-entry-last", fill_entries(300) + [K_TWICE_LAST], kind="keyerror"))
    ptail = fill_families(40)
    out.append(Tiled("D-family-0", ["late-first"] + fill_families(300), duplex=True, kind="keyerror"))
    out.append(Tiled("D-family-255", fill_families(255) + ["late-first"] + ptail, duplex=True, kind="keyerror"))
    out.append(Tiled("D-family-256", fill_families(256) + ["late-first"] + ptail, duplex=True, kind="keyerror"))
    out.append(Tiled("D-family-last", fill_families(300) + ["late-last"], duplex=True, kind="keyerror"))
    # singleton correction: the same singletons' table (no tag here has its duplex partner anywhere, so the
    # SC loop deletes the family as uncorrected at its region's end, as the DCS loop does as a singleton),
    # the deleted family past family 256, beside an SSCS table of a few of the same motifs
    seeds = fill_families(300) + ["late-first"] + ptail
    out.append(Tiled("C-family-300", seeds, duplex=True, kind="keyerror",
                     sscs=Tiled("C-family-300-sscs", seeds[:6], duplex=True)))
    out.append(Tiled("S-tiny", [SPLIT[0], ONE, RESTART[0]], "interleaved"))
    out.append(Tiled("P-tiny", [P_RESTART[0], P_PLAIN[0]], "interleaved", duplex=True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def split_entries(g):
    """The entries completed in a later region than the one that created them."""
    return [e for e in g.names if g.entry_done[e] is not None and g.entry_done[e] != g.entry_region[e]]


def restarted_entries(g):
    """The entries whose name has more than one entry (deleted at a region's end, started anew later)."""
    n = collections.Counter(g.entry_name)
    return [e for e in g.names if n[g.entry_name[e]] > 1]


def late_family_rank(case):
    """The engine's index of the one family read after its deletion, on a table whose stream holds every
    record once: families in position order, this one alone at its position."""
    pairs, g = case.result()
    rec, _ = case.stream()
    fams = sorted({f for _, f in g.late})
    assert len(fams) == 1 and len(set(rec)) == len(rec)
    where = lambda f: case.reads[pairs[g.families[f].first >> 1][g.families[f].first & 1]].pos
    at = [where(f) for f in range(len(g.families))]
    assert at.count(at[fams[0]]) == 1
    return sum(1 for x in at if x < at[fams[0]])
