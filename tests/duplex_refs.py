"""Plain references for the two in-pipeline duplex joins (tests/test_gpu_duplex_edges.py compares
cc_duplex_consensus and cc_singleton_correction with them; tests/test_duplex_refs.py pins them to
the Python oracle without a GPU): read_bam's family building (consensus_helper.py:308-506) in duplex
mode, the DCS loop (DCS_maker.py:245-282) and the SC loop (singleton_correction.py:278-319), restated
as dictionaries and loops over a table's record indices.  There is no chain logic here: a tag's
decision is whatever the dictionaries hold when the loop reaches it.

Results are per entry slot q = 2 * entry + (0 | 1), entries numbered as their first pair completes in
the stream: dec, t_rec (the family's first member record) and p_rec (the partner family's first
record; for SC in whichever table it lives).  A slot without a family holds 3, -1, -1.
  DCS dec: 0 made, 1 SSCS singleton, 2 skipped (the partner made the DCS)
  SC dec:  0 corrected by the SSCS, 1 corrected by the singleton, 2 uncorrected
Where the reference raises, `error` names the exception and the arrays are not to be used."""
import numpy as np

R1_FLAGS = frozenset((99, 83, 67, 115, 81, 97, 65, 113))
R2_FLAGS = frozenset((147, 163, 131, 179, 161, 145, 129, 177))
EMPTY = (3, -1, -1)


def swap_barcode(bc):
    """duplex_tag's barcode (consensus_helper.py:639-683): the halves around '.', else rotated by half."""
    if "." in bc:
        k = bc.index(".")
        return bc[k + 1:] + "." + bc[:k]
    return bc[len(bc) // 2:] + bc[:len(bc) // 2]


def read_number(flag):
    return "R1" if flag in R1_FLAGS else "R2" if flag in R2_FLAGS else None


def strand(t, r):
    f = int(t.flag[r])
    if f in (99, 147, 67, 131):
        return "pos"
    if f in (83, 163, 115, 179):
        return "neg"
    here, mate = (int(t.tid[r]), int(t.pos[r])), (int(t.mtid[r]), int(t.mpos[r]))
    if read_number(f) == "R1":
        return "pos" if here < mate else "neg"
    return "pos" if here > mate else "neg"


def complement(key):
    return (swap_barcode(key[0]),) + key[1:7] + ("R2" if key[7] == "R1" else "R1",)


class Families(object):
    """read_bam's dictionaries over one table, fed region by region."""

    def __init__(self, table):
        self.t = table
        self.pending = {}       # qname -> first record
        self.members = {}       # tag -> records
        self.size = {}          # tag -> count (never deleted from)
        self.entries = {}       # molecule -> (entry number, tags)
        self.n_entries = 0
        self.slot = {}          # tag -> its entry slot
        self.molecule = {}      # tag -> its molecule's name
        self.region = {}        # tag -> the region that created it

    def tag(self, r, bc, cig):
        t = self.t
        return (bc, int(t.tid[r]), int(t.pos[r]), int(t.mtid[r]), int(t.mpos[r]), cig,
                "rev" if int(t.flag[r]) & 16 else "fwd", read_number(int(t.flag[r])))

    def feed(self, records, region=0):
        t = self.t
        for r in records:
            q = t.qname[r]
            if q not in self.pending:
                self.pending[q] = r
                continue
            a, b = self.pending.pop(q), r
            bc = q.split("_")[0]
            s, num = strand(t, a), read_number(int(t.flag[a]))
            x, y = (a, b) if (s == "pos" and num == "R1") or (s == "neg" and num == "R2") else (b, a)
            cig = "%s_%s" % (t.cigar(x), t.cigar(y))
            lo, hi = sorted([(int(t.tid[a]), int(t.pos[a])), (int(t.tid[b]), int(t.pos[b]))])
            mol = (bc, lo, hi, cig, s, abs(int(t.tlen[a])))
            for rec in (a, b):
                k = self.tag(rec, bc, cig)
                if k not in self.members and k not in self.size:
                    self.members[k] = [rec]
                    self.size[k] = 1
                    self.region[k] = region
                    if mol not in self.entries:
                        self.entries[mol] = (self.n_entries, [])
                        self.n_entries += 1
                    e, tags = self.entries[mol]
                    if len(tags) < 2:
                        self.slot[k] = 2 * e + len(tags)
                        self.molecule[k] = "%s_%d_%d_%d_%d_%s_%s_%d" % (bc, lo[0], lo[1], hi[0], hi[1], cig, s, mol[5])
                        tags.append(k)
                elif k not in self.members:
                    raise KeyError(k)                       # a family emitted by an earlier region
                elif a not in self.members[k]:
                    self.members[k].append(rec)
                    self.size[k] += 1


def region_records(table, regions):
    """Per region (tid, start, end) its records in file order: start <= pos < end on that contig; one
    list of every record without regions."""
    if regions is None:
        return [list(range(len(table)))]
    return [[i for i in range(len(table)) if table.tid[i] == tid and start <= table.pos[i] < end]
            for tid, start, end in regions]


def region_runs(regions):
    """The chromosome run of each region, from 1 (a run ends where the next region names another contig;
    the first region begins one)."""
    if regions is None:
        return [0]
    runs = []
    for k, (tid, _, _) in enumerate(regions):
        runs.append(1 if k == 0 else runs[-1] + (1 if tid != regions[k - 1][0] else 0))
    return runs


class Result(object):
    def __init__(self):
        self.rows = {}
        self.error = None
        self.lists = {}
        self.sscs_runs = []    # SC: the SSCS side's dictionaries, one per chromosome run
        self.names = {}        # SC: slot -> the molecule name its output record carries

    def arrays(self, n_entries):
        out = np.tile(np.array(EMPTY, np.int32), (2 * n_entries, 1))
        for q, row in self.rows.items():
            out[q] = row
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def dcs(table, regions=None):
    """DCS_maker.py:245-282 over the table's stream."""
    fb, used, res = Families(table), set(), Result()
    made, single = [], []
    res.lists = dict(made=made, single=single)
    for n, records in enumerate(region_records(table, regions)):
        fb.feed(records, n)
        for mol in list(fb.entries):
            for k in fb.entries[mol][1]:
                q, ds = fb.slot[k], complement(k)
                own = fb.members[k][0]
                if ds in used:
                    res.rows[q] = (2, own, -1)
                    continue
                if k in fb.size and ds in fb.size:
                    if ds not in fb.members:
                        res.error = "KeyError"
                        return res, fb
                    other = fb.members[ds][0]
                    res.rows[q] = (0, own, other)
                    made.append((own, other))
                    used.add(k)
                else:
                    res.rows[q] = (1, own, -1)
                    single.append(own)
                del fb.members[k]
            del fb.entries[mol]
    return res, fb


def sc(singles_table, sscs_table, regions=None):
    """singleton_correction.py:278-319 over the two tables' streams."""
    g, s, res = Families(singles_table), Families(sscs_table), Result()
    by_sscs, by_single, uncorrected = [], [], []
    res.lists = dict(by_sscs=by_sscs, by_single=by_single, uncorrected=uncorrected)
    resolved = {}
    res.sscs_runs.append(s)
    runs = region_runs(regions)
    for n, (grecs, srecs) in enumerate(zip(region_records(singles_table, regions),
                                           region_records(sscs_table, regions))):
        if regions is not None and (n == 0 or runs[n] != runs[n - 1]):
            g.size = {}
            s = Families(sscs_table)
            res.sscs_runs.append(s)
        g.feed(grecs, n)
        s.feed(srecs, n)
        for mol in list(g.entries):
            for k in g.entries[mol][1]:
                q, ds = g.slot[k], complement(k)
                own = g.members[k][0]
                res.names[q] = g.molecule[k] + ":1"
                if ds in s.members:
                    res.rows[q] = (0, own, s.members[ds][0])
                    by_sscs.append((own, s.members[ds][0], q))
                    del s.members[ds]
                    del g.members[k]
                elif ds in g.members:
                    res.rows[q] = (1, own, g.members[ds][0])
                    by_single.append((own, g.members[ds][0], q))
                    resolved[k] = ds
                    if ds in resolved:
                        del g.members[k]
                        del g.members[ds]
                        del resolved[k]
                        del resolved[ds]
                else:
                    res.rows[q] = (2, own, -1)
                    uncorrected.append(own)
                    del g.members[k]
            del g.entries[mol]
    return res, g, s
