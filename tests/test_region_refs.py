"""tests/region_refs.py pinned to the Python oracle's region loops (cc_oracle.sscs_stage / dcs_stage with
FamilyBuilder.feed wrapped as oracle/fuzz_csn_tiny.py wraps it) on every tiny input of fuzz_csn_tiny.py
seeds 0..400, the eight hits of tests/test_gpu_csn_regions.py and the motifs tests/region_cases.py adds, in
both naming modes; and every edge tests/test_gpu_region_edges.py relies on derived again from the
restatement over the finished cases, with the oracle's verdict (raises / does not) on each.  No GPU: a
wrong reference must not be able to agree with a wrong kernel by construction."""
import os

import pytest

import cc_oracle
import region_cases as RC

HITS = [193, 584, 859, 958, 974, 1124, 1341, 1953]
SEEDS = list(range(0, 401)) + [s for s in HITS + list(RC.EXTRA_SEEDS) if s > 400]
RAISES = (cc_oracle.OracleError, KeyError, IndexError, ValueError, ZeroDivisionError)
_feed = cc_oracle.FamilyBuilder.feed


def content(s):
    return (s.query_name, s.flag, s.reference_start, s.next_reference_start, s.query_sequence)


def oracle_run(case, tmp):
    """The stage over the case's files with feed wrapped: what the dictionaries held after each region's
    feed.  -> dict(raised, region of the raise, tags in tag_dict order, sizes, members, entries
    [name, tags, region], emitted entries in order)."""
    bam, bed = os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.bed")
    case.write(bam, bed)
    st = dict(region=-1, entries=[], live={}, emitted=[], members={}, size={}, raised=False, ok_regions=0)

    def feed(self, records, region=None, **kw):
        st["region"] += 1
        # what the loop at the end of the region before deleted
        gone = [m for m in st["live"] if m not in self.entries]
        want_gone = st.pop("expect_gone", [])
        assert gone == want_gone, (case.name, st["region"], gone, want_gone)
        for m in gone:
            del st["live"][m]
        out = _feed(self, records, region, **kw)
        for m, keys in self.entries.items():                   # dict order: the survivors, then the new ones
            if m not in st["live"]:
                st["live"][m] = len(st["entries"])
                st["entries"].append([m, [], st["region"]])
            st["entries"][st["live"][m]][1] = list(keys)
        for k, v in self.members.items():
            st["members"][k] = [content(s) for s in v]
        st["size"] = dict(self.size)
        st["tags"] = list(self.size)
        if case.mode == "sscs":
            done = [m for m in st["live"] if len(self.entries[m]) == 2]
            st["emitted"] += [st["live"][m] for m in done]
        else:
            done = list(st["live"])
        st["expect_gone"] = done
        st["ok_regions"] += 1
        return out

    cc_oracle.FamilyBuilder.feed = feed
    try:
        if case.mode == "sscs":
            cc_oracle.sscs_stage(bam, os.path.join(tmp, "o.sscs.bam"), 0.7, bed)
        else:
            cc_oracle.dcs_stage(bam, os.path.join(tmp, "o.dcs.bam"), bed)
    except RAISES as e:
        # read_dict[tag] of a deleted family; anything else (an empty family table after the loops, a
        # vote's IndexError) is none of the region loops' doing
        st["raised"] = "KeyError" in "%s: %s" % (type(e).__name__, e)
        st["other"] = None if st["raised"] else str(e)
    finally:
        cc_oracle.FamilyBuilder.feed = _feed
    return st


def compare(case, st):
    """The restatement against what the oracle did; -> "raising" | "two_regions" | "plain"."""
    pairs, g = case.result()
    tag = (case.name, case.mode)
    raised = g.error is not None or bool(g.loop_errors)
    if st.get("other"):
        assert "empty family table" in st["other"] and not pairs and not raised, tag + (st["other"],)
        return "empty"
    assert st["raised"] == raised, tag
    if raised:
        # the raise is the first one's: in feed, in the region of the raising pair (the regions before it
        # fed and looped completely); or in the DCS loop at the end of a fed region
        feed_region = pairs[g.error][2] if g.error is not None else None
        loop_region = g.loop_errors[0] if g.loop_errors else None
        if feed_region is not None and (loop_region is None or feed_region <= loop_region):
            assert st["region"] == feed_region and st["ok_regions"] == feed_region, tag
        else:
            assert st["region"] == loop_region and st["ok_regions"] == loop_region + 1, tag
        # everything before it: the emissions of the completed regions
        if case.mode == "sscs":
            before = [e for e in g.emitted if g.entry_done[e] < st["ok_regions"]]
            assert st["emitted"] == before, tag
            assert [st["entries"][e][0] for e in before] == [g.entry_name[e] for e in before], tag
        return "raising"
    ends = [pairs[e >> 1][e & 1] for e in range(2 * len(pairs))]
    assert st["tags"] == [f.tag for f in g.families], tag
    for f in g.families:
        assert st["size"][f.tag] == len(f.members), tag + (f.tag,)
        r = [case.reads[ends[e]] for e in f.members]
        assert st["members"][f.tag] == [(x.qname, x.flag, x.pos, x.mpos, x.seq) for x in r], tag + (f.tag,)
    assert [(m, keys, reg) for m, keys, reg in st["entries"]] == [
        (g.entry_name[e], [g.families[f].tag for f in g.entries[e]], g.entry_region[e]) for e in g.names], tag
    assert len(st["tags"]) - sum(len(keys) for _, keys, _ in st["entries"]) == g.orphans, tag
    if case.mode == "sscs":
        assert st["emitted"] == g.emitted, tag
        assert all(g.entry_done[e] is not None for e in g.emitted), tag
        done = [g.entry_done[e] for e in g.emitted]
        assert done == sorted(done), tag
    return "two_regions" if RC.split_entries(g) or RC.restarted_entries(g) else "plain"


@pytest.mark.parametrize("duplex", [False, True], ids=["sscs", "per_region"])
def test_region_loop_matches_oracle(tmp_path, duplex):
    kinds = {"raising": [], "two_regions": [], "plain": [], "empty": []}
    for seed in SEEDS + (list(RC.HAND_SEEDS) if duplex else []):
        case = RC.Tiled("seed-%s" % seed, [seed], duplex=duplex)
        d = tmp_path / ("s%s" % seed)
        d.mkdir()
        kinds[compare(case, oracle_run(case, str(d)))].append(seed)
    print("REGIONPIN %s: %s" % ("per_region" if duplex else "sscs", {k: len(v) for k, v in kinds.items()}))
    # a run that degenerates (all seeds raising, say) pins nothing
    assert len(kinds["two_regions"]) >= 5, kinds["two_regions"]
    assert len(kinds["raising"]) >= 5 and len(kinds["plain"]) >= 5
    # the motifs the cases are built from are what they are used as
    use = [kinds["two_regions"], kinds["plain"], kinds["raising"]]
    if duplex:
        want = [RC.P_RESTART, RC.P_PLAIN + tuple(s for s, _ in RC.P_FILL), RC.HAND_SEEDS]
    else:
        want = [RC.SPLIT + RC.RESTART, RC.PLAIN + (RC.ONE, RC.UNSHARED),
                (RC.K_TWICE_FIRST, RC.K_WAITED_FIRST, RC.K_WAITED_FIRST_B, RC.K_TWICE_LAST)]
    for have, seeds in zip(use, want):
        assert set(seeds) <= set(have), (seeds, have)


def test_the_two_deletion_rules_by_hand():
    """One name with events in three regions: SSCS keeps a one-tag entry until a later region completes it
    and emits it there; the per-region loop deletes it each time, so each region starts an entry anew."""
    import group_refs as G
    import region_refs as RR
    m = ((0, 8),)
    rd = [G.Read("a|AC", 99, 0, 10, 0, 10, 8, m, "x"), G.Read("a|AC", 99, 0, 10, 0, 10, 8, m, "x"),      # one tag
          G.Read("b|AC", 147, 0, 10, 0, 10, 8, m, "y"), G.Read("b|AC", 147, 0, 10, 0, 10, 8, m, "y"),    # a second
          G.Read("c|AC", 131, 0, 10, 0, 10, 8, m, "z"), G.Read("c|AC", 131, 0, 10, 0, 10, 8, m, "z"),    # a third
          G.Read("d|AC", 99, 0, 10, 0, 10, 8, m, "w"), G.Read("d|AC", 99, 0, 10, 0, 10, 8, m, "w")]      # the first again
    pairs = [(0, 1, 0), (2, 3, 2), (4, 5, 2), (6, 7, 3)]
    g = RR.region_loop(pairs, lambda i: rd[i], "sscs")
    assert len(set(g.entry_name)) == 1 and g.entries == {0: [0, 1]} and g.orphans == 1
    assert (g.entry_region, g.entry_done, g.emitted) == ([0], [2], [0]) and g.error == 3 and g.late == [(3, 0)]
    for r in rd:
        r.qname = "AC_" + r.qname[0]
    g = RR.region_loop(pairs, lambda i: rd[i], "per_region")
    assert g.entries == {0: [0], 1: [1, 2]} and g.orphans == 0 and g.entry_region == [0, 2] and g.entry_done == [None, 2]
    assert g.error == 3 and g.late == [(3, 0)] and not g.loop_errors
    assert RR.complement("AC.GT_0_10_0_50_8M_8M_fwd_R1") == "GT.AC_0_10_0_50_8M_8M_fwd_R2"
    assert RR.complement("ACGT_0_10_0_50_8M_8M_rev_R2") == "GTAC_0_10_0_50_8M_8M_rev_R1"


# ---- the cases' edges, from the restatement alone --------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in RC.all_cases()}


def blocks(n):
    return range((n + RC.BLOCK - 1) // RC.BLOCK)


def test_every_edge_is_present(cases, tmp_path):
    B = RC.BLOCK
    for c in cases.values():
        assert len(c) < 10000, (c.name, len(c))
    # clean SSCS cases: entries completed in a later region than created, in every block and on a block's edge
    for order in ("blocked", "interleaved", "grouped"):
        _, g = cases["S-%s" % order].result()
        split = set(RC.split_entries(g))
        E = len(g.names)
        assert g.error is None and E >= 4 * B + 1, (order, E)
        # (interleaved: the last pass over the contig creates the last block's entries, and nothing
        # completes those later; the grouped bed has them in every block)
        with_split = {e // B for e in split}
        assert with_split >= set(blocks(E)[:-1] if order == "interleaved" else blocks(E)), (order, with_split)
        assert any(j * B - 1 in split for j in range(1, E // B + 1)), (order, sorted(split)[:40])
        assert any(j * B in split for j in range(1, E // B + 1)), (order, sorted(split)[:40])
        assert len({s for s in cases["S-%s" % order].seeds if s in RC.SPLIT}) >= 3
        assert RC.restarted_entries(g) and g.orphans > 0
        # the emission order is no identity: entries move by more than a block under the interleaved bed
        two = [e for e in g.names if len(g.entries[e]) == 2]
        assert g.emitted != two and sorted(g.emitted) == two
        moved = max(abs(x - two.index(e)) for x, e in enumerate(g.emitted))
        assert moved >= (B if order == "interleaved" else 1), (order, moved)
    sizes = set()
    assert len(RC.SMALL) == 6
    for e, order in RC.SMALL:
        _, g = cases["S-small-%d-%s" % (e, order)].result()
        assert g.error is None and len(g.names) == e and RC.split_entries(g)
        two = [x for x in g.names if len(g.entries[x]) == 2]
        assert g.emitted != two
        sizes.add((e, order))
    assert sizes == {(e, o) for e in (B - 1, B, B + 1) for o in ("blocked", "interleaved")}
    # clean per-region cases: a name's entries split by region in every block of entries
    for order in ("blocked", "interleaved"):
        _, g = cases["P-%s" % order].result()
        again = set(RC.restarted_entries(g))
        E, F = len(g.names), len(g.families)
        assert g.error is None and not g.loop_errors and F >= 4 * B + 1, (order, F)
        assert all(any(e in again for e in range(b * B, min(E, (b + 1) * B))) for b in blocks(E)), order
        assert not RC.split_entries(g)
    # the fast path's case: several regions, no consensus tag shared by two pairs
    c = cases["S-fast"]
    pairs, g = c.result()
    assert g.error is None and len(g.names) >= 8 * B + 1 and len(c.regions) > 1
    assert len({f.name for f in g.families}) == len({f.first >> 1 for f in g.families})
    assert g.emitted == [e for e in g.names if len(g.entries[e]) == 2] and g.orphans == 0
    # SSCS KeyErrors: one family read after its deletion, its entry at 0, 255, 256 and E - 1, both ways
    ways = set()
    for name, at in (("K-entry-0", 0), ("K-entry-255", B - 1), ("K-entry-256", B), ("K-entry-last", -1)):
        c = cases[name]
        pairs, g = c.result()
        E = len(g.names)
        assert g.error is not None and len({f for _, f in g.late}) == 1 and E >= B + 1, name
        assert g.entry_of[g.late[0][1]] == (at if at >= 0 else E - 1), (name, g.entry_of[g.late[0][1]], E)
        assert sum(1 for s in c.seeds if RC.profile(s)["error"] is not None) == 1, name
        ways.add(RC.profile([s for s in c.seeds if RC.profile(s)["error"] is not None][0])["way"])
    assert ways == {"twice", "waited"}
    # DCS KeyErrors: the one deleted family at family 0, 255, 256 and F - 1 (position order: no record twice)
    for name, at in (("D-family-0", 0), ("D-family-255", B - 1), ("D-family-256", B), ("D-family-last", -1)):
        c = cases[name]
        pairs, g = c.result()
        F = len(g.families)
        assert g.error is not None and not g.loop_errors and F >= B + 1, name
        assert RC.late_family_rank(c) == (at if at >= 0 else F - 1), (name, RC.late_family_rank(c), F)
    # singleton correction: the deleted singleton family past family 256
    c = cases["C-family-300"]
    _, g = c.result()
    assert g.error is not None and not g.loop_errors and c.sscs is not None and len(c.sscs) > 0
    assert RC.late_family_rank(c) == 300 > B and len(g.families) > 300
    # the oracle's verdict on every case: the stage's, and the whole pipeline's on the SSCS-named ones (a
    # clean case passes every stage; a KeyError case raises read_dict[tag] in the SSCS stage)
    for c in cases.values():
        d = tmp_path / c.name
        d.mkdir()
        _, g = c.result()
        st = oracle_run(c, str(d))
        assert st["raised"] == (c.kind == "keyerror") == (g.error is not None), c.name
        if not st["raised"] and c.mode == "sscs":
            assert st["emitted"] == g.emitted, c.name
        if c.mode == "sscs":
            bam, bed = str(d / "sample.bam"), str(d / "regions.bed")
            c.write(bam, bed)
            try:
                out = cc_oracle.consensus_pipeline(bam, str(d / "oracle"), bedfile=bed)
                err = None
            except RAISES as e:
                out, err = None, "%s: %s" % (type(e).__name__, e)
            assert (err is not None) == (c.kind == "keyerror"), (c.name, err)
            if err is None:
                assert all(os.path.exists(out[k]) for k in ("stats", "read_families", "all_unique", "dcs_sc")), c.name
            else:
                assert "consensus_helper.py:490" in err and not os.path.exists(str(d / "oracle" / "sample" / "dcs" / "sample.dcs.bam"))
        elif c.sscs is not None:
            sbam, xbam = str(d / "x.singleton.sorted.bam"), str(d / "x.sscs.sorted.bam")
            c.write(sbam, str(d / "regions.bed"))
            c.sscs.write(xbam, str(d / "unused.bed"))
            with pytest.raises(cc_oracle.OracleError, match="consensus_helper.py:490"):
                cc_oracle.sc_stage(sbam, str(d / "regions.bed"))
