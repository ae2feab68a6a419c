"""tests/duplex_refs.py pinned to the Python oracle (cc_oracle.dcs_stage / sc_stage) on every case of
tests/test_gpu_duplex_edges.py: the refs' decisions, turned into the stage's record lists, must be the
oracle's output files record for record, and a case the oracle raises on must raise the same error in
the refs.  The kernel constants the cases mirror are checked against csrc/cc_engine.hip, and every
case's claimed edges are derived again from its finished tables: family indices against the 256-family
blocks, bucket indices from a mirror of k_bucket_geom and bucket_of.  No GPU."""
import os
import re

import numpy as np
import pytest

import cc_oracle
import duplex_cases as DC
import duplex_refs as R
import pysam
import vote_refs as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return DC.all_cases()


def test_kernel_constants_are_mirrored():
    with open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, pattern
        return m[0]

    assert one(r"constexpr int DD_T = (\d+), DD_H = (\d+);") == (str(DC.DD_T), str(DC.DD_H))
    assert int(one(r"constexpr int DEEP_MIN = (\d+);")) == DC.DEEP_MIN == DC.DD_H + 1
    assert int(one(r"constexpr int DUPLEX_CHAIN = (\d+);")) == DC.DUPLEX_CHAIN
    assert int(one(r"uint64_t size = (\d+);\n    while \(size < \(uint64_t\)\(2 \* g\.F\)\) size <<= 1;")) == DC.HT_FLOOR
    assert DC.HT_FACTOR == 2
    one(r"const int64_t w0 = f0 > DD_H \? f0 - DD_H : 0;")
    one(r"const int64_t w1 = min\(F, f0 \+ DD_T \+ DD_H\);")
    one(r"if \(block_sum64\(part, s_w\) <= 2 \* N \+ ntid\) \{ bs = s; break; \}")
    one(r"return b < tbase\[t \+ 1\] \? b : tbase\[t \+ 1\];")
    # the edges as the issue that asked for them lists them
    assert DC.GROUPS == (2, 3, 63, 64) and DC.offsets(3) == (-64, -63, -2, -1, 0, 1)
    assert DC.offsets(64) == (-64, -63, -1, 0, 1) and DC.offsets(2) == (-64, -63, -1, 0, 1)
    assert DC.CHAIN_HOPS == (1, 2, 3, 4, 5, 31, 32) and DC.HASHED_F == (511, 512, 513)
    assert [DC.ht_size(F) for F in DC.HASHED_F] == [1024, 1024, 2048]


def test_refs_by_hand():
    assert R.swap_barcode("AC.GT") == "GT.AC" and R.swap_barcode("ACGTA") == "GTAAC"
    k = ("AC.GT", 0, 5, 1, 9, "8M_8M", "fwd", "R1")
    assert R.complement(k) == ("GT.AC", 0, 5, 1, 9, "8M_8M", "fwd", "R2") and R.complement(R.complement(k)) == k
    assert R.region_runs([(0, 0, 5), (0, 5, 9), (1, 0, 9), (0, 9, 12)]) == [1, 1, 2, 3]
    assert DC.bucket_geometry(4, [100, 100]) == (5, [0, 4, 8]) and DC.bucket_of(5, [0, 4, 8], 0, 500) == 4
    assert DC.bucket_of(5, [0, 4, 8], 2, 0) == 8 and DC.bucket_of(5, [0, 4, 8], 1, 99) == 7


# ---- the refs against the oracle -------------------------------------------------------------------------
def duplex_name(tag_name, ds_name):
    bc, dbc = tag_name.split("_")[0], ds_name.split("_")[0]
    coords = tag_name.split("_", 1)[1].rsplit("_", 1)[0]
    n_tag, n_ds = tag_name.split(":")[1], ds_name.split(":")[1]
    return "%s_%s_%s:%s_%s" % ((bc, dbc, coords, n_tag, n_ds) if "pos" in tag_name else (dbc, bc, coords, n_ds, n_tag))


def voted_line(header, t, own, tb, other, gate, name):
    """The consensus record of own (table t) with other (table tb) as the stage writes it."""
    codes, quals = V.pair_vote(t.codes[own], t.quals[own], tb.codes[other], tb.quals[other], gate)
    r = t.segment(own, header)
    r.query_name = name
    r.query_sequence = "".join(DC.PC.NT16[c] for c in codes)
    r.query_qualities = [int(q) for q in quals]
    if not gate:
        r.mapping_quality = V.most_common_first([int(t.mapq[own]), int(tb.mapq[other])])
        r.template_length = V.most_common_first([int(t.tlen[own]), int(tb.tlen[other])])
        r.flag = V.pick_flag([int(t.flag[own]), int(tb.flag[other])])
    return pysam.canonical_sam_line(r)


def raw_lines(header, t, recs):
    return [pysam.canonical_sam_line(t.segment(r, header)) for r in recs]


def run_case(case, tmp):
    """(the refs' record lists, the oracle's), or the two errors."""
    t = case.table
    header = t.header()
    bed = None
    if case.regions:
        bed = os.path.join(tmp, "regions.bed")
        with open(bed, "w") as f:
            f.write(DC.bed_text(case.regions))
    if case.kind == "dcs":
        bam = os.path.join(tmp, "x.sscs.sorted.bam")
        t.write(bam)
        res, _ = R.dcs(t, case.regions)
        try:
            cc_oracle.dcs_stage(bam, os.path.join(tmp, "x.dcs.bam"), bed)
        except cc_oracle.OracleError as e:
            return res.error, str(e).split(":")[0]
        if res.error:
            return res.error, None
        ours = [[voted_line(header, t, a, t, b, False, duplex_name(t.qname[a], t.qname[b])) for a, b in res.lists["made"]],
                raw_lines(header, t, res.lists["single"])]
        ref = [pysam.sam_lines(os.path.join(tmp, "x.dcs.bam")), pysam.sam_lines(os.path.join(tmp, "x.sscs.singleton.bam"))]
        return ours, ref
    sbam, xbam = os.path.join(tmp, "x.singleton.sorted.bam"), os.path.join(tmp, "x.sscs.sorted.bam")
    t.write(sbam)
    case.sscs.write(xbam)
    res, _, _ = R.sc(t, case.sscs, case.regions)
    cc_oracle.sc_stage(sbam, bed)
    ours = [[voted_line(header, t, a, case.sscs, b, True, res.names[q]) for a, b, q in res.lists["by_sscs"]],
            [voted_line(header, t, a, t, b, True, res.names[q]) for a, b, q in res.lists["by_single"]],
            raw_lines(header, t, res.lists["uncorrected"])]
    ref = [pysam.sam_lines(os.path.join(tmp, "x.%s.bam" % k)) for k in ("sscs.correction", "singleton.correction",
                                                                         "uncorrected")]
    return ours, ref


def test_refs_match_oracle(cases, tmp_path):
    made = corrected = most_made = most_b_in_a = 0
    for n, case in enumerate(cases):
        tmp = str(tmp_path / str(n))
        os.makedirs(tmp)
        ours, ref = run_case(case, tmp)
        if case.error:
            assert (ours, ref) == (case.error, case.error), case.name
            continue
        assert not isinstance(ours, str) and ours is not None, (case.name, ours, ref)
        for k, (a, b) in enumerate(zip(ours, ref)):
            assert a == b, (case.name, k, len(a), len(b), [x for x in zip(a, b) if x[0] != x[1]][:2])
        if case.kind == "dcs":
            made += len(ours[0])
            most_made = max(most_made, len(ours[0]))
            assert ours[0] and ours[1], case.name           # every case makes a DCS and leaves a singleton
        else:
            corrected += len(ours[0]) + len(ours[1])
            most_b_in_a = max(most_b_in_a, len(ours[1]))
    assert made > 1000 and corrected > 100
    # the rows the GPU test votes and compares: at least 20 in one case, of each duplex vote and of its b_in_a branch
    assert most_made >= 20 and most_b_in_a >= 20


# ---- the edges, from the finished tables --------------------------------------------------------------
def family_groups(fb):
    """The position groups of a coordinate grouping: (index of the first family, families)."""
    at = sorted((k[1], k[2]) for k in fb.size)
    out, i = [], 0
    while i < len(at):
        j = i
        while j < len(at) and at[j] == at[i]:
            j += 1
        out.append((i, j - i))
        i = j
    return out, len(at)


def derive(case):
    t = case.table
    out = set()
    if case.kind == "dcs":
        res, fb = R.dcs(t, case.regions)
        groups, F = family_groups(fb)
        Q = 2 * fb.n_entries
        out |= {("F", F), ("F_hashed", F, DC.ht_size(F))}
        last = (F - 1) // DC.DD_T * DC.DD_T
        for start, g in groups:
            if start + g == F:
                out.add(("group_ends_at_F", g))
            for b in (start // DC.DD_T * DC.DD_T, start // DC.DD_T * DC.DD_T + DC.DD_T):
                for k in [b // DC.DD_T] + (["last"] if b == last else []):
                    out.add(("grp", g, start - b, k))
        slots = set(fb.slot.values())
        if any(q + 1 not in slots for q in slots if q % 2 == 0):
            out.add(("one_tag",))
        if Q - 1 not in slots and Q - 1 >= F:
            out.add(("empty_slot_at_F",))
        orphans = [k for k in fb.size if k not in fb.slot]
        for k in orphans:
            out.add(("orphan", "partner" if R.complement(k) in fb.slot else "alone"))
        if case.regions:
            if res.error:
                out.add(("bed", "dcs", "keyerror"))
            for k, q in fb.slot.items():
                ds = R.complement(k)
                if ds in fb.region and q in res.rows:
                    if res.rows[q][0] == 0 and fb.region[ds] < fb.region[k]:
                        out.add(("bed", "dcs", "partner_earlier"))
                    if res.rows[q][0] == 1 and fb.region[ds] > fb.region[k]:
                        out.add(("bed", "dcs", "partner_later"))
    else:
        res, g, s = R.sc(t, case.sscs, case.regions)
        groups, F = family_groups(g)
        sizes = {n for _, n in groups}
        out |= {("g_group", n) for n in sizes}
        if groups and groups[0][1] == 2:
            out.add(("g_group", 2, "first"))
        if groups and groups[-1][1] == 2:
            out.add(("g_group", 2, "last"))
        out.add(("sscs_families", len(s.size)))
        if case.s_hashed:
            out.add(("s_hashed",))
        x = case.sscs
        if len(x) and not case.s_hashed:
            shift, tbase = DC.table_geometry(x)
            if shift == DC.BUCKET_SHIFT:
                W, nb, ntid = 1 << shift, tbase[-1], len(tbase) - 1
                spos = {}
                for i in range(len(x)):
                    spos.setdefault(DC.bucket_of(shift, tbase, int(x.tid[i]), int(x.pos[i])), set()).add(
                        (int(x.tid[i]), int(x.pos[i])))
                for q, (dec, own, other) in res.rows.items():
                    tid, pos = int(t.tid[own]), int(t.pos[own])
                    b = DC.bucket_of(shift, tbase, tid, pos)
                    here = sorted(spos.get(b, ()))
                    if dec == 0:
                        if pos % W == 0:
                            out.add(("bucket", "first"))
                        if pos % W == W - 1:
                            out.add(("bucket", "last"))
                        if len(here) >= 5:
                            k = here.index((tid, pos))
                            out.add(("bucket", "dense_first" if k == 0 else "dense_last" if k == len(here) - 1
                                     else "dense_middle"))
                        if b == nb - 1 and (tid, pos) == here[-1]:
                            out.add(("bucket", "last_bucket"))
                    elif tid >= ntid:
                        out.add(("bucket", "no_contig"))
                    elif pos > max(p for tt, p in set().union(*spos.values()) if tt == tid):
                        assert b == tbase[tid + 1]
                        out.add(("bucket", "beyond"))
                    elif not here and b - 1 in spos and b + 1 in spos:
                        out.add(("bucket", "empty"))
                    elif len(here) >= 5 and here[0] < (tid, pos) < here[-1] and (tid, pos) not in here:
                        out.add(("bucket", "dense_absent"))
        if case.regions:
            runs = R.region_runs(case.regions)
            for k, q in g.slot.items():
                ds, dec, rk = R.complement(k), res.rows[q][0], g.region[k]
                sr = [x.region[ds] for x in res.sscs_runs if ds in x.region]
                if dec == 2 and sr and min(sr) > rk and runs[min(sr)] == runs[rk]:
                    out.add(("bed", "sc", "sscs_later"))
                if dec == 0 and sr and min(sr) < rk:
                    out.add(("bed", "sc", "sscs_earlier"))
                if dec == 0 and runs[rk] > runs[0]:
                    out.add(("bed", "sc", "second_run"))
                if dec == 2 and ds in g.region and g.region[ds] != rk:
                    out.add(("bed", "sc", "single_later" if g.region[ds] > rk else "single_earlier"))
        # decisions: the singleton y of a pair (x, y) whose tag is an SSCS family too; mutual corrections; chains
        for q, (dec, own, other) in res.rows.items():
            if dec == 0:
                k = next((k for k, v in g.slot.items() if v == q))
                if R.complement(k) in g.size:
                    y = g.slot[R.complement(k)]
                    out.add(("sscs_wins", "x" if q < y else "y"))
    # chains and mutual pairs, from the barcodes: a tag's partners processed before it; the two mutual pairs of
    # one position group of four families, the forward first end processed first in one and second in the other
    fb = R.dcs(t, case.regions)[1] if case.kind == "dcs" else R.sc(t, case.sscs, case.regions)[1]
    sites = {}
    for k, q in fb.slot.items():
        sites.setdefault(k[1:3], []).append(k)
        ds = R.complement(k)
        if ds in fb.slot and R.complement(ds) == k:
            continue
        hops, x = 0, k
        while R.complement(x) in fb.slot and fb.slot[R.complement(x)] < fb.slot[x]:
            x, hops = R.complement(x), hops + 1
        if hops:
            out.add(("chain", hops, "present" if R.complement(x) in fb.size else "absent"))
    for tags in sites.values():
        r1 = [k for k in tags if k[7] == "R1" and R.complement(k) in tags and R.complement(R.complement(k)) == k]
        if len(tags) == 4 and len(r1) == 2 and {fb.slot[k] < fb.slot[R.complement(k)] for k in r1} == {True, False}:
            out.add(("mutual", 2))
    return out


def test_cases_hold_their_edges(cases):
    for c in cases:
        claimed = c.edges
        if c.hashed and c.kind == "dcs" and not c.name.startswith("H-"):
            # (a deep group appended: the block geometry is not in use and the last entries are the deep group's)
            claimed = {e for e in c.edges if e[0] not in ("grp", "F", "group_ends_at_F", "empty_slot_at_F")}
        missing = claimed - derive(c)
        assert not missing, (c.name, sorted(missing, key=str))
    every = set().union(*(c.edges for c in cases if not c.hashed))
    want = {("grp", g, s, k) for g in DC.GROUPS for s in DC.offsets(g) for k in DC.BLOCKS if k != 0 or s >= 0}
    assert want <= every and len(want) == 2 * 22 + 8
    assert {("F", F) for F in (511, 512, 513)} | {("group_ends_at_F", 64), ("one_tag",), ("empty_slot_at_F",)} <= every
    assert {("orphan", "partner"), ("orphan", "alone")} <= every
    assert {("chain", h, f) for h in DC.CHAIN_HOPS for f in DC.FAR} | {("chain", 33, "present")} <= every
    hashed = set().union(*(c.edges for c in cases if c.hashed))
    assert {("F_hashed", 511, 1024), ("F_hashed", 512, 1024), ("F_hashed", 513, 2048)} <= hashed
    sc = set().union(*(c.edges for c in cases if c.kind == "sc"))
    assert {("bucket", k) for k in ("first", "last", "empty", "dense_first", "dense_middle", "dense_last", "dense_absent",
                                    "beyond", "no_contig", "last_bucket")} <= sc
    assert {("sscs_wins", "x"), ("sscs_wins", "y"), ("mutual", 2), ("sscs_families", 0), ("sscs_families", 2)} <= sc
    assert {("chain", h, f) for h in (1, 2, 3, 4) for f in DC.FAR} | {("chain", 32, "present"), ("chain", 33, "present")} <= sc
    assert {("bed", "dcs", k) for k in ("partner_earlier", "partner_later", "keyerror")} <= every
    assert {("bed", "sc", k) for k in ("sscs_later", "sscs_earlier", "single_later", "single_earlier", "second_run")} <= sc
    for c in cases:
        if c.regions:
            assert len(c.regions) == 3 and {r[0] for r in c.regions} == {0, 1}
            assert all(a[0] != b[0] or a[2] <= b[1] or b[2] <= a[1] for a in c.regions for b in c.regions if a is not b)
    # the groupings are what the paths need: local unless a deep group was appended
    for c in cases:
        t = c.table
        key = t.keys()
        deep = int(np.max(np.unique(key, return_counts=True)[1])) >= DC.DEEP_MIN
        assert deep == bool(c.hashed), c.name
        if c.sscs is not None and len(c.sscs):
            deep = int(np.max(np.unique(c.sscs.keys(), return_counts=True)[1])) >= DC.DEEP_MIN
            assert deep == bool(c.s_hashed), c.name
