"""tests/pair_refs.py pinned to the Python oracle (cc_oracle.FamilyBuilder.feed) on a reduced draw of
the cases of tests/test_gpu_pair_edges.py, the kernel constants those cases mirror checked against
csrc/cc_engine.hip, and every case's claimed edges derived again from its finished table: record
indices against the tile, halo and staging-window arithmetic.  No GPU: a wrong reference must not be
able to agree with a wrong kernel by construction, and a layout that misses its edge fails here."""
import collections
import os
import re

import numpy as np
import pytest

import cc_oracle
import pair_cases as PC
import pair_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return PC.all_cases()


def test_kernel_constants_are_mirrored():
    with open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, pattern
        return m[0]

    assert int(one(r"constexpr int GRP_SMALL = (\d+);")) == PC.GRP_SMALL
    assert int(one(r"constexpr int DEEP_MIN = (\d+);")) == PC.DEEP_MIN == PC.GRP_SMALL + 1
    assert int(one(r"constexpr int PC_HALO = (\d+);")) == PC.PC_HALO
    assert int(one(r"constexpr int32_t PD_W = (\d+);")) == PC.PD_W
    assert int(one(r"constexpr int64_t PD_TILE = (\d+);")) == PC.PD_TILE
    assert int(one(r"constexpr int DQ_CAP = (\d+), DQ_T = CC_DQ_T;")) == PC.DQ_CAP
    assert int(one(r"#define CC_DQ_T (\d+)")) == PC.DQ_T
    assert int(one(r"#define CC_DQ_GRID (\d+)")) == PC.DQ_GRID
    assert one(r"k_pair_coord_tile<(\d+)> : k_pair_coord_tile<(\d+)>") == tuple(str(t) for t in PC.TILES)
    assert one(r"for \(int64_t step = (\d+);; step <<= (\d+)\)") == (str(PC.GALLOP0), "2")
    one(r"const int64_t x = g0 \+ 16 \* \(int64_t\)\(t \+ 1\);")       # deep_group_end: DQ_T probes 16 apart
    one(r"const int64_t w1 = min\(N, t1 \+ GRP_SMALL \+ 2\);")
    one(r"const bool many = NR > S / 4;")
    # the edges as the issue that asked for them lists them
    assert PC.HALO_D == (1, 2, 511, 512, 513)
    assert PC.GALLOP_D == (255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385)
    assert PC.GALLOP_PROBES == (256, 1280, 5376, 21760) and PC.GALLOP_AT_PROBES == (1279, 1280, 1281, 5375, 5376, 5377)
    assert PC.DEEP_SIZES == (65, 66, 8191, 8192, 8193, 16384, 16385)
    assert PC.tile_offsets(512) == (0, 1, 255, 256, 511) and PC.tile_offsets(1024) == (0, 1, 255, 256, 1023)
    assert PC.QNAME_LENS == (1, 7, 8, 9, 31, 32, 33, 40, 200)
    assert [len(PC.qname_of_length(n, 3)) for n in PC.QNAME_LENS] == list(PC.QNAME_LENS)


def test_pair_dict_by_hand():
    q = ["a", "b", "a", "a", "c", "a", "b", "a"]
    got, pending = R.pairs(list(range(10, 18)), [0, 0, 0, 1, 1, 1, 2, 2], q, [True] * 8)
    assert got == [(10, 12, 0), (13, 15, 1), (11, 16, 2)] and pending == 2       # c, and the fifth a
    got, pending = R.pairs(list(range(8)), [0] * 8, q, [True, True, False, True, True, True, True, False])
    assert got == [(0, 3, 0), (1, 6, 0)] and pending == 2
    assert R.passes("x|AC", 99, 1, 1) and not R.passes("x", 99, 1, 1) and R.passes("x", 99, 0, 1)
    assert not R.passes("x|AC", 103, 1, 1) and not R.passes("x|AC", 73, 1, 1) and R.passes("x|AC", 105, 1, 1)
    assert not R.passes("x|AC", 355, 1, 1) and not R.passes("x|AC", 2147, 1, 1)
    assert all(R.passes(q_, f, 1, 0) for q_ in ("x", "x|AC") for f in (99, 103, 73, 355, 2147))


# ---- the edges, from the finished table -------------------------------------------------------------
def derive(case):
    """The edge set of a case, from record indices alone."""
    t, T = case.table, case.tile
    n = len(t)
    out = {("n", n)}
    ident = len(case.stream) == n and np.array_equal(case.stream, np.arange(n))
    if not ident:
        seen = collections.Counter(case.stream.tolist())
        twice = sum(1 for v in seen.values() if v > 1)
        if twice:
            out.add(("entered_twice", twice))
        else:
            out.add(("subset", len(case.stream)))
        if len(set(case.region.tolist())) > 1:
            out.add(("regions", len(set(case.region.tolist()))))
        # what a subset leaves out, against the table: one end of a pair that the coordinates find (the
        # mate, and the searching end), and both records on either side of a tile's first record
        gone = np.ones(n, bool)
        gone[case.stream] = False
        names = collections.defaultdict(list)
        for i, q in enumerate(t.qname):
            names[q].append(i)
        tkey = t.keys()
        for recs in names.values():
            if len(recs) != 2 or gone[recs[0]] == gone[recs[1]]:
                continue
            m, s = recs
            if (int(t.mtid[s]) << 32) + int(t.mpos[s]) == tkey[m] and tkey[m] <= tkey[s]:
                out.add(("left_out_found_mate",) if gone[m] else ("left_out_searcher",))
        if any(gone[k - 1] and gone[k] for k in range(T, n, T)):
            out.add(("left_out_tile_edge",))
    if not t.is_sorted():
        out.add(("unsorted",))
        return out
    key = t.keys()
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if n else np.zeros(0, np.int64)
    end = np.concatenate([start[1:], [n]]) if n else start
    gs = np.repeat(start, end - start)
    gsize = np.repeat(end - start, end - start)
    first_of = {int(key[a]): (int(a), int(b - a)) for a, b in zip(start, end)}
    by_name = collections.defaultdict(list)
    for i, q in enumerate(t.qname):
        by_name[q].append(i)
    ndeep = int(np.sum(end - start > PC.GRP_SMALL))
    if ndeep:
        out.add(("deep_groups", ndeep))
        if end[0] - start[0] > PC.GRP_SMALL:
            out.add(("deep_first",))
        if end[-1] - start[-1] > PC.GRP_SMALL:
            out.add(("deep_last",))
    for a, b in zip(start, end):                        # groups beginning at a tile's end
        g = int(b - a)
        sizes = collections.Counter(t.qname[i] for i in range(a, b)) if g <= PC.GRP_SMALL + 2 else {}
        if g > PC.GRP_SMALL and sizes and max(sizes.values()) == 2:
            t1 = (int(a) + T - 1) // T * T
            for edge in (t1, t1 + T):
                if 0 <= edge - a <= PC.GRP_SMALL + 2 and edge < n:
                    out.add(("past_end", g, int(edge - a)))
    resid = wrong = 0
    for q, recs in by_name.items():
        found = []                                       # (searcher, mate) by coordinates
        for r in recs:
            target = (int(t.mtid[r]) << 32) + int(t.mpos[r])
            if t.mtid[r] < 0:
                out.add(("no_mtid",))
                continue
            if target > key[r]:
                continue
            cand = [m for m in recs if m != r and key[m] == target]
            if len(cand) != 1 or (target == key[r] and cand[0] > r):
                continue
            s, m = r, cand[0]
            found.append((s, m))
            a, g = first_of[target]
            t0, t1, w0, w1 = PC.window(s, T, n)
            out.add(("place", s - m, s % T))
            if s == n - 1:
                out.add(("last_record",))
            if t.tid[s] != t.tid[m]:
                out.add(("other_contig",))
            if target == key[s]:
                out.add(("same_pos", g))
            if w0 > 0 and a < w0 < a + g:
                out.add(("w0_split", g, w0 - a, "before" if m < w0 else "after"))
            if g > PC.GRP_SMALL:
                rel = "same" if gs[s] == a else "deep" if gsize[s] > PC.GRP_SMALL else "small"
                out.add(("deep", g, rel))
            elif w0 > 0 and a <= w0:
                out |= {("route", "global"), ("gallop", w0 - a)}
                if a == 0:
                    out.add(("gallop_to_first",))
            else:
                out.add(("route", "own" if m >= t0 else "halo"))
            if len(recs) == 2 and s - m in (PC.PD_W, PC.PD_W + 1):
                out.add(("span", s - m))
                if s // PC.PD_TILE != m // PC.PD_TILE:
                    out.add(("span_over_pd_tile",))
        in_pair = {x for p in found for x in p}
        resid += sum(1 for r in recs if r not in in_pair)
        if len(recs) == 2 and not found:
            wrong += 1
        if len(recs) == 3 and len(found) == 1 and recs[0] in found[0] and recs[2] in found[0]:
            out.add(("triple", recs[2] - recs[0]))
        if len(recs) == 3 and len(found) == 1 and recs[2] not in found[0]:
            out.add(("found_and_resid",))
        if len(recs) == 3 and not found:
            out.add(("resid_triple",))
        if len(recs) == 4 and len(found) == 2:
            a, b, c, d = recs
            if sorted(found) == [(c, a), (d, b)]:
                out.add(("quad", c - a, d - b, d - c))
                if c // PC.PD_TILE != d // PC.PD_TILE:
                    out.add(("pd_tile_boundary", d - c))
            elif sorted(found) == [(b, a), (d, c)]:
                out.add(("apart", d - b))
        # qname bytes
        if len(recs) == 2 and found:
            out.add(("qname_len", len(q)))
    singles = sum(1 for recs in by_name.values() if len(recs) == 1)
    out |= {("wrong_mpos", wrong), ("absent", singles), ("resid", resid, n)}
    out.add(("resid_many",) if resid > n // 4 else ("resid_few",))
    for a, b in zip(start, end):
        names = sorted({t.qname[i] for i in range(a, b)}) if b - a <= PC.GRP_SMALL else []
        for x in names:
            for y in names:
                if x != y and len(x) > 32 and x[:32] == y[:32]:
                    out.add(("equal_first_32",))
                if x != y and y.startswith(x):
                    out.add(("equal_but_length",))
    # filtered records with a live qname (or none) inside a searched target group
    kinds = dict((f, k) for k, f in PC.INTERLOPERS)
    for i in range(n):
        f = int(t.flag[i])
        kind = kinds.get(f) or ("no_delimiter" if "|" not in t.qname[i] else None)
        if kind is None:
            continue
        live = [r for r in by_name[t.qname[i]] if r != i]
        mates = [r for r in range(int(gs[i]), int(gs[i] + gsize[i])) if r != i and len(by_name[t.qname[r]]) >= 2]
        if (kind == "no_delimiter" or len(live) == 2) and mates:
            out.add(("interloper", kind))
    return out


def test_cases_hold_their_edges(cases):
    for c in cases:
        missing = c.edges - derive(c)
        assert not missing, (c.name, sorted(missing, key=str))
        pairs, _ = c.expected()
        assert pairs or len(c.table) == 1, c.name
    every = set().union(*(c.edges for c in cases))
    for T in PC.TILES:
        a = set().union(*(c.edges for c in cases if c.name[0] == "A" and c.tile == T))
        assert {("place", d, off) for d in PC.HALO_D for off in PC.tile_offsets(T)} <= a
        assert {("route", k) for k in ("own", "halo", "global")} <= a
        assert {("gallop", d) for d in PC.GALLOP_D + PC.GALLOP_AT_PROBES} | {("gallop_to_first",)} <= a
        assert {("w0_split", g, k, side) for g in (2, 64, 65, 66) for k in (1, g - 1) for side in ("before", "after")} <= a
        assert {("past_end", g, back) for g in (65, 66) for back in (66, 1, 0)} <= a
        assert {("same_pos", g) for g in (2, 3, 64, 65, 66)} <= a
        assert {("n", n) for n in (1, 2, 255, 256, 257, 2 * T, 4 * T + 37)} <= a
        b = set().union(*(c.edges for c in cases if c.name[0] == "B" and c.tile == T))
        assert {("deep", g, "same") for g in PC.DEEP_SIZES} <= b and ("deep_groups", PC.DQ_GRID + 1) in b
        assert {("deep_first",), ("deep_last",)} <= b
    assert {("span", PC.PD_W), ("span", PC.PD_W + 1), ("apart", PC.PD_W), ("apart", PC.PD_W + 1)} <= every
    assert {("pd_tile_boundary", 1), ("triple", PC.PD_W), ("triple", PC.PD_W + 1)} <= every
    assert {("left_out_found_mate",), ("left_out_searcher",), ("left_out_tile_edge",)} <= every
    assert {("resid_few",), ("resid_many",), ("resid_triple",), ("found_and_resid",), ("unsorted",)} <= every
    assert {("interloper", k) for k in ("unmapped", "mate_unmapped", "secondary", "supplementary", "no_delimiter")} <= every
    assert {("qname_len", n) for n in PC.QNAME_LENS} | {("equal_first_32",), ("equal_but_length",)} <= every
    quads = {e for e in every if e[0] == "quad"}
    long_spans = {(e[1] > PC.PD_W) + (e[2] > PC.PD_W) for e in quads}
    assert long_spans == {0, 1, 2} and {e[3] for e in quads} >= {PC.PD_W, PC.PD_W + 1}


# ---- the reference against the oracle -----------------------------------------------------------------
REDUCED = ("A-size-1-T512", "A-size-257-T512", "A-one-position-T512", "A-contigs-T512", "A-window-start-T512",
           "B-deep-T512", "C-multi", "C-apart", "D-triple", "D-found-and-resid", "E-subset-2regions-T512",
           "E-overlap-T512", "E-shuffled-T512", "E-filters-bad1-T512", "E-filters-bad0-T512", "F-qnames")


@pytest.mark.parametrize("name", REDUCED)
def test_pairs_match_oracle(cases, name, monkeypatch):
    case = {c.name: c for c in cases}[name]
    t = case.table
    header = t.header()
    limit = 6000                                     # a reduced draw: the stream's first entries
    stream, region = case.stream[:limit], case.region[:limit]
    segs = {}
    records = []
    for r in stream:
        if r not in segs:
            segs[r] = t.segment(int(r), header)
            segs[r].table_index = int(r)
        records.append(segs[r])
    calls = []
    real = cc_oracle.molecule_name

    def spy(first, second, barcode, cigars):
        calls.append((first.table_index, second.table_index))
        return real(first, second, barcode, cigars)

    monkeypatch.setattr(cc_oracle, "molecule_name", spy)
    fb = cc_oracle.FamilyBuilder()
    got = []
    for reg in sorted(set(region.tolist())):        # one feed per region, as read_bam's region loop
        before = len(calls)
        fb.feed([x for x, g in zip(records, region) if g == reg], delim="|" if case.delim_filter else None,
                bad_sink=[] if case.badread else None)
        got += [(a, b, reg) for a, b in calls[before:]]
    qn = [t.qname[r] for r in stream]
    ps = [R.passes(t.qname[r], int(t.flag[r]), case.delim_filter, case.badread) for r in stream]
    want, pending = R.pairs(stream, region, qn, ps)
    assert got == want
    assert len(fb.pending) == pending
    assert want or len(t) == 1
