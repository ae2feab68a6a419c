"""tests/group_refs.py pinned to the Python oracle (cc_oracle.FamilyBuilder.feed) on every case of
tests/test_gpu_group_edges.py of at most 10,000 records, the kernel constants those cases mirror checked
against csrc/cc_engine.hip, and every case's claimed edges derived again from its finished table: record
indices against the ranking tile, group and family sizes, the sub-round and bitmap arithmetic and the
creation entries.  No GPU: a wrong reference must not be able to agree with a wrong kernel by
construction, and a layout that misses its edge fails here."""
import collections
import os
import re

import numpy as np
import pytest

import cc_oracle
import group_cases as GC
import group_refs as R
import pair_refs as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN_LIMIT = 10000


@pytest.fixture(scope="module")
def cases():
    return [c for c in GC.all_cases() if c.switch is None]


@pytest.fixture(scope="module")
def grouped(cases):
    return {c.name: GC.grouping(c) for c in cases}


def test_kernel_constants_are_mirrored():
    with open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, pattern
        return m[0]

    assert int(one(r"constexpr int GRP_SMALL = (\d+);")) == GC.GRP_SMALL
    assert one(r"constexpr int GT = (\d+), GH = (\w+), GS = GT \+ 2 \* GH, GW = GS / 32;") == (str(GC.GT), "GRP_SMALL")
    assert GC.GH == GC.GRP_SMALL
    assert int(one(r"constexpr int GC_TILES = (\d+);")) == GC.GC_TILES
    assert one(r"constexpr int DF_T = (\d+), DF_SLOTS = (\d+), DF_FAMS = (\d+), DF_SORT = (\d+), DF_ST = (\d+);") == tuple(
        str(x) for x in (GC.DF_T, GC.DF_SLOTS, GC.DF_FAMS, GC.DF_SORT, GC.DF_ST))
    assert int(one(r"constexpr int U = (\d+); ")) == GC.DF_U
    assert int(one(r"constexpr int U3 = (\d+); ")) == GC.DF_U3
    assert int(one(r"#define CC_DF_GRID (\d+)")) == GC.DF_GRID
    assert int(one(r"constexpr int64_t CT = (\d+);")) == GC.CT
    assert one(r"constexpr int CW = (\d+) \* GRP_SMALL;") == str(GC.CW // GC.GRP_SMALL) and GC.CW % GC.GRP_SMALL == 0
    one(r"if \(r0 \+ 4 <= N\) \{")                                     # k_group_count's 16-byte path
    one(r"if \(c <= 64u\) items\[atomicAdd\(n_items, 1u\)\] = itm;")   # k_deep_emit up to a wave, else k_deep_sortfam
    one(r"for \(uint32_t j0 = 0; j0 < m; j0 \+= 4u \* DF_ST\) \{")
    # the edges as the issue that asked for them lists them
    assert GC.PLACE_SIZES == (1, 2, 63, 64, 65) and GC.STRADDLE_K == (1, 31, 32, 33, 63)
    assert GC.TABLE_SIZES == (2, 255, 256, 257, 1023, 1024, 1025, 1027)
    assert GC.DEEP_SIZES == (65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
    assert GC.FAMS_PER_GROUP == (1, 2, 511, 512, 513) and GC.EMIT_SIZES == (1, 2, 63, 64)
    assert GC.SORTFAM_SIZES == (65, 511, 512, 513, 2048, 2049, 8192, 8193)
    assert GC.E_FAMILIES == (2, 65, 300)


def reads_of(*rows):
    return [R.Read(*row) for row in rows]


def test_grouping_by_hand():
    m = ((0, 8),)
    rd = reads_of(("a|AC", 99, 0, 10, 0, 50, 48, m, b"x"), ("a|AC", 147, 0, 50, 0, 10, -48, m, b"y"),
                  ("b|AC", 99, 0, 10, 0, 50, 48, m, b"x"), ("b|AC", 147, 0, 50, 0, 10, -48, m, b"y"),
                  ("c|AC", 67, 0, 10, 0, 50, 48, m, b"x"), ("c|AC", 131, 0, 50, 0, 10, -48, m, b"y"),
                  ("d|AC", 99, 0, 10, 0, 10, 8, m, b"x"), ("d|AC", 99, 0, 10, 0, 10, -8, m, b"x"))
    g = R.group([(0, 1, 0), (2, 3, 0), (4, 5, 1), (6, 7, 1)], lambda i: rd[i])
    assert [f.tag for f in g.families] == ["AC_0_10_0_50_8M_8M_fwd_R1", "AC_0_50_0_10_8M_8M_rev_R2",
                                           "AC_0_50_0_10_8M_8M_fwd_R2", "AC_0_10_0_10_8M_8M_fwd_R1"]
    assert [f.members for f in g.families] == [[0, 2, 4], [1, 3], [5], [6]]
    assert [f.slots for f in g.families] == [[0, 2, 4], [1, 3], [5], [6, 7]] and g.dropped == {7}
    assert [f.first for f in g.families] == [0, 1, 5, 6] and [f.region for f in g.families] == [0, 0, 1, 1]
    assert g.family_of == [0, 1, 0, 1, 0, 2, 3, 3]
    assert g.names == ["AC_0_10_0_50_8M_8M_pos_48", "AC_0_10_0_10_8M_8M_pos_8"]
    assert g.entries == {g.names[0]: [0, 1], g.names[1]: [3]} and g.orphans == 1
    assert R.strand(R.Read("q", 65, 0, 5, 0, 9, 0, m, b"")) == "pos" and R.strand(R.Read("q", 129, 0, 5, 0, 9, 0, m, b"")) == "neg"
    assert R.cigar_string([(4, 4), (0, 4)]) == "4S4M"


# ---- the edges, from the finished table -------------------------------------------------------------------
def derive(case, pairs, g):
    """The edge set of a case: record indices, group and family sizes and creation entries alone."""
    t = case.table
    n = len(t)
    out = {("n", n)}
    ends = [pairs[e >> 1][e & 1] for e in range(2 * len(pairs))]         # read end -> record
    if len(set(case.region.tolist())) > 1:
        out.add(("regions", len({f.region for f in g.families})))
    if not t.is_sorted():
        out.add(("unsorted",))
        return out | {("family", len(f.slots)) for f in g.families}
    key = t.keys()
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    end = np.concatenate([start[1:], [n]])
    size = end - start
    gi = np.repeat(np.arange(len(start)), size)                          # record -> group
    has_end = np.zeros(n, bool)
    has_end[ends] = True
    n_ends = np.add.reduceat(has_end.astype(np.int64), start)
    fams_of_group = collections.defaultdict(list)
    for f in g.families:
        fams_of_group[int(gi[ends[f.first]])].append(f)
    for k, (a, b, sz, ne) in enumerate(zip(start.tolist(), end.tolist(), size.tolist(), n_ends.tolist())):
        if ne == 0:
            continue
        if b % GC.GT == 0:
            out.add(("place", sz, "end"))
        if a % GC.GT == 0:
            out.add(("place", sz, "start"))
        elif a // GC.GT != (b - 1) // GC.GT:
            out.add(("place", sz, "straddle", GC.GT - a % GC.GT))
        if a == 0:
            out.add(("first", sz))
        if b == n:
            out.add(("last", sz))
        out.add(("start_bit", (a % GC.GT + GC.GH) % 32, sz))             # its index among the staged records
        if ne < sz:
            out.add(("noends", sz, ne))
        if 0 < k < len(start) - 1 and size[k - 1] == size[k + 1] and n_ends[k - 1] and n_ends[k + 1]:
            out.add(("flank", sz, int(size[k - 1])))
        if k and t.tid[a] != t.tid[a - 1] and t.pos[a] == t.pos[a - 1] and n_ends[k - 1]:
            out.add(("tid_change_same_pos",))
        if sz > 1 and any(not PR.passes(t.qname[r], int(t.flag[r]), 1, 1) for r in range(a, b)):
            out.add(("badread_in_group",))
        fams = fams_of_group[k]
        deep = sz > GC.GRP_SMALL
        if deep:
            out |= {("deep_size", sz), ("nfam", len(fams))}
        elif ne == sz:
            if len(fams) == 1:
                out.add(("one_family", sz))
            if len(fams) == sz:
                out.add(("singletons", sz))
            by_rec = {ends[e]: j for j, f in enumerate(sorted(fams, key=lambda f: min(ends[e] for e in f.slots)))
                      for e in f.slots}
            if 1 < len(fams) < sz and all(by_rec[r] == (r - a) % len(fams) for r in range(a, b)):
                out.add(("interleaved", len(fams)))
        for f in fams:
            recs = [ends[e] for e in f.slots]
            s = len(recs)
            up = all(x < y for x, y in zip(recs, recs[1:]))
            down = s > 1 and all(x > y for x, y in zip(recs, recs[1:]))
            twice = [e for e in f.slots if e in g.dropped]
            if not deep:
                if down:
                    out.add(("reversed",))
                for e in twice:
                    prs = []
                    for x in f.slots:
                        if x >> 1 not in prs:
                            prs.append(x >> 1)
                    at = prs.index(e >> 1)
                    out.add(("lrt", "alone" if len(prs) == 1 else "first" if at == 0 else
                             "last" if at == len(prs) - 1 else "middle"))
                for h in fams:
                    x, y = f.tag.split("_"), h.tag.split("_")
                    assert len(x) == len(y) == len(GC.TAG_FIELDS)
                    diff = [name for name, p, q in zip(GC.TAG_FIELDS, x, y) if p != q]
                    if len(diff) == 1:
                        out.add(("differs", diff[0]))
                continue
            if up or down:
                out.add(("family_size", s, "ordered" if up else "reversed"))
            if s > GC.WAVE:
                if s == sz:
                    out.add(("sortfam", s, "dense"))
                if len(fams) == 4 and all(len(h.slots) == s for h in fams):
                    out.add(("sortfam", s, "sparse"))
                lo = min(f.slots)
                for e in twice:
                    assert e & 1 and e - 1 in f.slots
                    if e - 1 == lo:
                        out.add(("lrt_lowest",))
                    if (e - 1 - lo) % 32 == 31:
                        out.add(("lrt_word_cross",))
            off = sorted(r - a for r in recs)
            if s == GC.DF_T and off[0] % GC.DF_T == 0 and off == list(range(off[0], off[0] + s)):
                out.add(("whole_subround",))
            waves = [x // GC.WAVE for x in off]
            if s == GC.DF_T // GC.WAVE and waves[0] % s == 0 and waves == list(range(waves[0], waves[0] + s)):
                out.add(("one_per_wave",))
            if len({x // GC.DF_T for x in off}) >= 3 and len(fams) > 1:
                out.add(("three_subrounds",))
    with_ends = [int(s) > GC.GRP_SMALL for s, ne in zip(size, n_ends) if ne]
    if True in with_ends and with_ends.index(True) > 0 and False in with_ends[with_ends.index(True):]:
        out.add(("mixed",))
    if any(not has_end[a:a + GC.GT].any() for a in range(0, n, GC.GT)):
        out.add(("empty_tile",))
    # molecule names whose families more than one pair created: the pairs' first creation entries
    by_name = collections.defaultdict(list)
    for k, f in enumerate(g.families):
        by_name[f.name].append(k)
    for name, ks in by_name.items():
        first_of_pair = {}
        for k in ks:
            first_of_pair.setdefault(g.families[k].first >> 1, k)
        if len(first_of_pair) < 2:
            continue
        ent = g.entries[name]
        if len(ent) == 2 and g.families[ent[0]].first >> 1 != g.families[ent[1]].first >> 1:
            out.add(("entry_of_two_pairs",))
        recs = [r for p in first_of_pair for r in pairs[p][:2]]
        kind = "deep" if any(size[gi[r]] > GC.GRP_SMALL for r in recs) else "small"
        lo, hi = min(first_of_pair.values()), max(first_of_pair.values())
        out.add(("shared_name", kind, len(first_of_pair), hi - lo, lo // GC.CT != hi // GC.CT))
    return out


def test_cases_hold_their_edges(cases, grouped):
    for c in cases:
        pairs, g = grouped[c.name]
        missing = c.edges - derive(c, pairs, g)
        assert not missing, (c.name, sorted(missing, key=str))
        assert pairs and len(g.family_of) == 2 * len(pairs)
        assert len(c.table) <= 20000
    by_class = {k: set().union(*(c.edges for c in cases if c.name[0] == k)) for k in "ABCDE"}
    a, b, c_, d, e = (by_class[k] for k in "ABCDE")
    for sz in GC.PLACE_SIZES:
        assert {("place", sz, "end"), ("place", sz, "start")} <= a
        assert {("place", sz, "straddle", k) for k in GC.STRADDLE_K if k < sz} <= a
    assert {("first", 64), ("last", 64), ("flank", 64, 65), ("flank", 65, 64), ("tid_change_same_pos",)} <= a
    assert {("start_bit", s, sz) for s, sz in ((31, 64), (0, 64), (1, 64))} <= a
    assert {("noends", 66, 60), ("noends", 64, 2), ("badread_in_group",), ("empty_tile",)} <= a
    assert {("n", n) for n in GC.TABLE_SIZES} <= a
    assert {("one_family", 64), ("singletons", 64), ("interleaved", 2), ("interleaved", 3), ("reversed",)} <= b
    assert {("differs", f) for f in GC.DIFFER} | {("lrt", w) for w in GC.LRT_PLACES} <= b
    assert {("deep_size", s) for s in GC.DEEP_SIZES} | {("nfam", k) for k in GC.FAMS_PER_GROUP} <= c_
    assert {("whole_subround",), ("one_per_wave",), ("three_subrounds",), ("mixed",)} <= c_
    assert {("family_size", s, o) for s in (2, 63, 64, 65) for o in ("ordered", "reversed")} | {("family_size", 1, "ordered")} <= c_
    assert {("sortfam", s, "dense") for s in GC.SORTFAM_SIZES} | {("sortfam", 65, "sparse"), ("sortfam", 513, "sparse")} <= c_
    assert {("lrt_word_cross",), ("lrt_lowest",)} <= c_
    span = 2 * (GC.GRP_SMALL - 1)
    assert {("shared_name", "small", 2, span, True), ("shared_name", "deep", 2, span, True),
            ("shared_name", "small", 3, span, True), ("entry_of_two_pairs",), ("regions", 2)} <= d
    assert {("unsorted",)} | {("family", s) for s in GC.E_FAMILIES} <= e
    assert grouped["D-three-pairs"][1].orphans == 3 and grouped["D-shared-small"][1].orphans == 1
    assert grouped["D-lrt-entry"][1].orphans == 0 and len(grouped["B-families"][1].dropped) == len(GC.LRT_PLACES)


# ---- the reference against the oracle -------------------------------------------------------------------------
PINNED = [c.name for c in GC.all_cases() if c.switch is None and len(c.table) <= PIN_LIMIT]


def test_the_pin_leaves_out_only_large_tables(cases):
    assert {c.name for c in cases} - set(PINNED) == {"C-sortfam", "C-sortfam-max", "C-sortfam-over"}


@pytest.mark.parametrize("name", PINNED)
def test_grouping_matches_oracle(cases, grouped, name):
    case = {c.name: c for c in cases}[name]
    t = case.table
    header = t.header()
    segs = [t.segment(i, header) for i in range(len(t))]
    index = {id(s): i for i, s in enumerate(segs)}
    fb = cc_oracle.FamilyBuilder()
    for reg in sorted(set(case.region.tolist())):            # one feed per region, as read_bam's region loop
        fb.feed([segs[r] for r, x in zip(case.stream, case.region) if x == reg], delim="|", bad_sink=[])
    pairs, g = grouped[name]
    ends = [pairs[e >> 1][e & 1] for e in range(2 * len(pairs))]
    assert list(fb.members) == [f.tag for f in g.families]
    for f in g.families:
        assert [index[id(s)] for s in fb.members[f.tag]] == [ends[e] for e in f.members], f.tag
        assert fb.size[f.tag] == len(f.members)
    assert list(fb.entries) == g.names
    for nm in g.names:
        assert fb.entries[nm] == [g.families[k].tag for k in g.entries[nm]], nm
    # every end is a member of one family, or the second end of a pair whose first end is in that family
    slots = sorted(e for f in g.families for e in f.slots)
    assert slots == list(range(2 * len(pairs)))
    assert all(e & 1 and g.family_of[e - 1] == g.family_of[e] for e in g.dropped)
