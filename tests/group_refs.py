"""read_dict / tag_dict / csn_pair_dict (consensus_helper.py:455-500) restated in plain Python, the
reference of tests/test_gpu_group_edges.py (pinned to the oracle's FamilyBuilder.feed by
tests/test_group_refs.py): walk the completed pairs in completion order; each of a pair's two reads
takes its read-end key; a new key starts a family and enters the pair's molecule name's entry while that
holds fewer than two keys (a third is an orphan); a known key takes the read unless the pair's first read
is already a member of that family, by record equality ("line read twice").  Read end e = 2 * p + side
is read `side` of completed pair p.  Everything is dicts, lists and string and integer equality."""

CIGAR_OPS = "MIDNSHP=X"
R1_FLAGS = (99, 83, 67, 115, 81, 97, 65, 113)
R2_FLAGS = (147, 163, 131, 179, 161, 145, 129, 177)
POS_FLAGS = (99, 147, 67, 131)
NEG_FLAGS = (83, 163, 115, 179)
BY_COORD_FLAGS = (65, 129, 113, 177, 81, 161, 97, 145)


class Read(object):
    """One record's fields, by name."""

    def __init__(self, qname, flag, tid, pos, mtid, mpos, tlen, cigar, seq):
        self.qname, self.flag, self.tid, self.pos = qname, flag, tid, pos
        self.mtid, self.mpos, self.tlen, self.cigar, self.seq = mtid, mpos, tlen, cigar, seq

    def content(self):
        """What record equality compares (mapping quality and base qualities are one value here)."""
        return (self.qname, self.flag, self.tid, self.pos, self.mtid, self.mpos, self.tlen, self.cigar, self.seq)


def read_of(table, i):
    return Read(table.qname[i], int(table.flag[i]), int(table.tid[i]), int(table.pos[i]), int(table.mtid[i]),
                int(table.mpos[i]), int(table.tlen[i]), tuple(table.cigar_of(i)), table.seq[i].tobytes())


def cigar_string(cigar):
    return "".join("%d%s" % (ln, CIGAR_OPS[op]) for op, ln in cigar)


def read_number(flag):
    return "R1" if flag in R1_FLAGS else "R2" if flag in R2_FLAGS else None


def strand(r):
    """The strand a read's pair is named for: by the flag where it says, else by the read number and
    which of the two coordinates is lower."""
    if r.flag in POS_FLAGS:
        return "pos"
    if r.flag in NEG_FLAGS:
        return "neg"
    if r.flag in BY_COORD_FLAGS:
        own, mate = (r.tid, r.pos), (r.mtid, r.mpos)
        if read_number(r.flag) == "R1":
            return "pos" if own < mate else "neg"
        return "pos" if own > mate else "neg"
    return None


def pair_cigars(first, second):
    """Both cigars, the first read's own one in front when it is R1 of a pos pair or R2 of a neg pair."""
    s, num = strand(first), read_number(first.flag)
    if (s == "pos" and num == "R1") or (s == "neg" and num == "R2"):
        a, b = first, second
    else:
        a, b = second, first
    return "%s_%s" % (cigar_string(a.cigar), cigar_string(b.cigar))


def end_tag(r, barcode, cigars):
    """unique_tag: a read end's family key."""
    return "_".join(str(x) for x in (barcode, r.tid, r.pos, r.mtid, r.mpos, cigars, "rev" if r.flag & 0x10 else "fwd",
                                      read_number(r.flag)))


def pair_name(first, second, barcode, cigars):
    """sscs_qname: the molecule's name, the lower coordinate first."""
    lo, hi = sorted(((first.tid, first.pos), (second.tid, second.pos)))
    return "_".join(str(x) for x in (barcode, lo[0], lo[1], hi[0], hi[1], cigars, strand(first), abs(first.tlen)))


class Family(object):
    def __init__(self, tag, name, first, region):
        self.tag, self.name, self.first, self.region = tag, name, first, region   # name: its creating pair's
        self.members = []     # read ends kept, in completion order (read_dict[tag]); size = len(members)
        self.slots = []       # and with the dropped ones
        self.held = set()     # the members' records, as record equality sees them


class Grouping(object):
    def __init__(self):
        self.families = []    # in tag_dict insertion order
        self.by_tag = {}
        self.family_of = []   # per read end its family's index (a dropped end: the family that refused it)
        self.dropped = set()
        self.names = []       # molecule names in csn_pair_dict insertion order
        self.entries = {}     # name -> the one or two creating families' indices
        self.orphans = 0


def group(pairs, read, delim="|"):
    """pairs: [(rec_first, rec_second, region)] in completion order (pair_refs.pairs); read(i): the Read
    of record i."""
    g = Grouping()
    for p, (a, b, region) in enumerate(pairs):
        first, second = read(a), read(b)
        barcode = first.qname.split(delim)[1]
        cigars = pair_cigars(first, second)
        name = pair_name(first, second, barcode, cigars)
        for side, r in enumerate((first, second)):
            e = 2 * p + side
            tag = end_tag(r, barcode, cigars)
            if tag not in g.by_tag:
                g.by_tag[tag] = len(g.families)
                fam = Family(tag, name, e, region)
                g.families.append(fam)
                fam.members.append(e)
                fam.held.add(r.content())
                if name not in g.entries:
                    g.entries[name] = []
                    g.names.append(name)
                if len(g.entries[name]) < 2:
                    g.entries[name].append(g.by_tag[tag])
                else:
                    g.orphans += 1
            else:
                fam = g.families[g.by_tag[tag]]
                if first.content() not in fam.held:
                    fam.members.append(e)
                    fam.held.add(r.content())
                else:
                    g.dropped.add(e)
            fam.slots.append(e)
            g.family_of.append(g.by_tag[tag])
    return g
