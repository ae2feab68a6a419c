"""The bed-region loops past one 256-thread block: csn entries split per the stage's loop (k_csn_entries,
per_region 0 and 1), SSCS emission slots by completing region (k_emit_keys, sort_emit, k_emit_rank, then
k_sscs_emit's scatter through hx) and the KeyErrors of families read after their deletion
(k_overlap_keyerror; k_dcs_deleted + k_deleted_late), through Engine.read_bam / consensus_maker /
duplex_consensus on the tiled cases of tests/region_cases.py, against tests/region_refs.py (pinned to the
oracle's stages by tests/test_region_refs.py, which also derives every edge the cases claim).

Clean cases: every array test_gpu_group_edges.check_grouping compares (ent_f, has2, ent_pair, fam_region and
the ENTRIES / FAMILIES / ORPHAN_TAGS counters among them), for SSCS emit_rec / emit_n in the restatement's
emission order and emit_ckey through the formatted names, the kernel scopes that say which path ran, two
planned re-runs, and the whole pipeline (SSCS names) or the DCS stage (duplex names, which the SSCS stage
would file under bad spacers) against the oracle's in file order, stats and read_families as text (the
SSCS-named clean motifs are chosen so that every later stage passes too).  KeyError cases: CC_E_KEYERROR
from the call that holds the check (read_bam; duplex_consensus; singleton_correction on the case with an
SSCS-side table, where the SC decision's fam_del feeds k_deleted_late), from the pipeline or stage too,
and a small clean case on the same engine afterwards.  read_bam's raise leaves no arrays to fetch, so an
SSCS KeyError case's entry index is the restatement's; the DCS and SC cases check the deleted family's
index on the device through fam_first.  Everything compared is an integer, a byte string or a text, for equality."""
import os
import shutil

import numpy as np
import pytest

import region_cases as RC
from parity import PARTIAL, assert_same_in_order
from test_gpu_group_edges import check_grouping, same

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in RC.all_cases()}
_broken = []     # an engine error ends the module: nothing more is started on a device that may have faulted


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def check_emission(engine, it, g, case, pairs, ref, tag):
    """emit_rec / emit_n / emit_ckey: both families of each emitted entry in the region loop's order."""
    from consensuscruncher_amd.engine import csn_names
    ends = [p[k] for p in pairs for k in (0, 1)]
    fams = ref.emitted_families()
    emit_rec, emit_n = engine.fetch(g, "emit_rec", np.int32), engine.fetch(g, "emit_n", np.int32)
    ckey = engine.fetch(g, "emit_ckey", np.int32)
    assert len(emit_rec) >= len(fams) and len(emit_n) >= len(fams) and len(ckey) >= 9 * len(ref.emitted), tag
    at = lambda i: dict(slot=i, entry=ref.emitted[i >> 1])
    same(emit_rec[:len(fams)], [ends[ref.families[f].members[0]] for f in fams], tag + ("emit_rec",), at)
    same(emit_n[:len(fams)], [len(ref.families[f].members) for f in fams], tag + ("emit_n",), at)
    blob, off = csn_names(it, np.repeat(ckey[:9 * len(ref.emitted)].reshape(-1, 9), 2, axis=0).reshape(-1),
                          emit_n[:len(fams)])
    got = [blob[off[i]:off[i + 1]].tobytes().decode() for i in range(len(fams))]
    want = ["%s:%d" % (ref.entry_name[e], len(ref.families[f].members)) for e in ref.emitted for f in ref.entries[e]]
    bad = [i for i in range(len(fams)) if got[i] != want[i]][:1]
    assert not bad, tag + ("emit_ckey", at(bad[0]), got[bad[0]], want[bad[0]])


def arrays(engine, case, d, check=True):
    """read_bam (and the stage's call) on the case's files against the restatement; a KeyError case's
    defined error from the call that holds its check."""
    from consensuscruncher_amd import native as N
    from consensuscruncher_amd.engine import MODE_DUPLEX, MODE_SSCS, Bam, Interner, bed_stream
    sscs = case.mode == "sscs"
    pairs, ref = case.result()
    bam, bed = str(d / "sample.bam"), str(d / "regions.bed")
    case.write(bam, bed)
    it = Interner()
    b = Bam(bam)
    rec = b.decode(it, MODE_SSCS if sscs else MODE_DUPLEX, "|")
    assert rec.n == len(case)
    stream = bed_stream(rec, b.refs, bed)
    srec, sreg = case.stream()
    assert stream.rec.tolist() == srec and stream.region.tolist() == sreg
    tid = g = xtid = xg = None
    try:
        if case.sscs is not None:       # singleton correction: the SSCS side's table under the same bed file
            xbam = str(d / "sscs_side.bam")
            case.sscs.write(xbam, str(d / "unused.bed"))
            xb = Bam(xbam)
            xrec = xb.decode(it, MODE_DUPLEX, "|")
            xtid = engine.upload(xrec)
            xg = engine.read_bam(xtid, bed_stream(xrec, xb.refs, bed), 0, 0, 1)
        tid = engine.upload(rec)
        engine.set_profiling(True)
        engine.profile_only(())
        if sscs and case.kind == "keyerror":
            with pytest.raises(N.CCError) as e:
                engine.read_bam(tid, stream, 1, 1, 0)
            assert e.value.code == N.CC_E_KEYERROR, str(e.value)
            return bam, bed
        g = engine.read_bam(tid, stream, 1 if sscs else 0, 1 if sscs else 0, 0)
        check_grouping(engine, g, pairs, ref, (case.name, "exact"))
        swap = None if sscs else it.swap_table()
        if case.kind == "keyerror":      # DCS: the one deleted family where the case put it, then the raise
            first = engine.fetch(g, "fam_first", np.int32)[:len(ref.families)].tolist()
            late = sorted({f for _, f in ref.late})
            want = RC.late_family_rank(case)
            assert [first.index(ref.families[f].first) for f in late] == [want], (case.name, want)
            for seed in (None, 0xabcdef, 0x1234567):
                if seed is not None:
                    engine.rerun(g, seed)
                    if xg is not None:
                        engine.rerun(xg, seed)
                with pytest.raises(N.CCError) as e:
                    if xg is not None:
                        engine.singleton_correction(g, xg, swap)
                    else:
                        engine.duplex_consensus(g, swap)
                assert e.value.code == N.CC_E_KEYERROR, (seed, str(e.value))
            return bam, bed
        if sscs:
            engine.consensus_maker(g, 0.7)
            check_emission(engine, it, g, case, pairs, ref, (case.name, "exact"))
        else:
            engine.duplex_consensus(g, swap)
        kt = engine.kernel_times()
        engine.set_profiling(False)
        print("REGIONCASE %s records %d regions %d pairs %d families %d entries %d emitted %d orphans %d scopes %s" % (
            case.name, len(case), len(case.regions), len(pairs), len(ref.families), len(ref.names), len(ref.emitted),
            ref.orphans, ",".join(k for k in sorted(kt) if k.startswith(("k_csn", "sort_", "k_emit", "k_sscs")))))
        if check:
            if case.kind == "fast":
                assert "k_csn_fast" in kt and "sort_csn" not in kt and "k_csn" not in kt and "sort_emit" not in kt, sorted(kt)
            else:
                assert "sort_csn" in kt and "k_csn" in kt, sorted(kt)
                assert ("sort_emit" in kt) == sscs, sorted(kt)
        for seed in (0xabcdef, 0x1234567):      # planned passes
            engine.rerun(g, seed)
            check_grouping(engine, g, pairs, ref, (case.name, "planned", seed))
            if sscs:
                engine.consensus_maker(g, 0.7)
                check_emission(engine, it, g, case, pairs, ref, (case.name, "planned", seed))
            else:
                engine.duplex_consensus(g, swap)
        return bam, bed
    except N.CCError as e:
        _broken.append("%s: %s" % (case.name, e))
        raise
    finally:
        if not _broken:
            engine.set_profiling(False)
            for x in (g, xg):
                if x is not None:
                    engine.free_group(x)
            for x in (tid, xtid):
                if x is not None:
                    engine.free_table(x)


def pipeline(engine, case, d, bam, bed):
    """The whole pipeline (SSCS names) or the DCS stage (duplex names) against the oracle's, in file order."""
    import cc_oracle
    from consensuscruncher_amd import native as N
    from consensuscruncher_amd import stages
    from consensuscruncher_amd.pipeline import consensus_pipeline
    if case.sscs is not None:          # the SC stage on both tables' files
        ours, ref = d / "ours", d / "ref"
        for x in (ours, ref):
            os.makedirs(str(x))
            shutil.copy(bam, str(x / "x.singleton.sorted.bam"))
            shutil.copy(str(d / "sscs_side.bam"), str(x / "x.sscs.sorted.bam"))
        with pytest.raises(cc_oracle.OracleError, match="consensus_helper.py:490"):
            cc_oracle.sc_stage(str(ref / "x.singleton.sorted.bam"), bed)
        with pytest.raises(N.CCError) as e:
            run = stages.SCRun(engine, str(ours / "x.singleton.sorted.bam"), bed)
            try:
                run.emit(verbose=False)
            finally:
                run.close()
        assert e.value.code == N.CC_E_KEYERROR, str(e.value)
        return
    if case.mode != "sscs":
        ours, ref = d / "ours", d / "ref"
        for x in (ours, ref):
            os.makedirs(str(x))
            shutil.copy(bam, str(x / "x.sscs.sorted.bam"))
        ref_err = our_err = None
        try:
            cc_oracle.dcs_stage(str(ref / "x.sscs.sorted.bam"), str(ref / "x.dcs.bam"), bed)
        except cc_oracle.OracleError as e:
            ref_err = str(e)
        try:
            stages.run_dcs(str(ours / "x.sscs.sorted.bam"), str(ours / "x.dcs.bam"), bed, engine=engine, verbose=False)
        except N.CCError as e:
            our_err = e
        assert (ref_err is not None) == (case.kind == "keyerror") == (our_err is not None), (case.name, ref_err, our_err)
        if ref_err is not None:
            assert ref_err.startswith("KeyError") and our_err.code == N.CC_E_KEYERROR, (ref_err, our_err)
            return
        for k in ("x.dcs.bam", "x.sscs.singleton.bam"):
            assert_same_in_order(str(ours / k), str(ref / k), "%s/%s" % (case.name, k))
        return
    ref_err = our_err = ours = None
    try:
        ref = cc_oracle.consensus_pipeline(bam, str(d / "oracle"), bedfile=bed)
    except cc_oracle.OracleError as e:
        ref_err = str(e)
    try:
        ours = consensus_pipeline(bam, str(d / "gpu"), bedfile=bed, engine=engine, level=1)
    except N.CCError as e:
        our_err = e
    # a clean case passes every stage of the oracle's pipeline (tests/test_region_refs.py checks that too)
    assert (ref_err is not None) == (case.kind == "keyerror") == (our_err is not None), (case.name, ref_err, our_err)
    if ref_err is not None:
        # read_dict[tag] in the SSCS stage's feed; whatever the oracle left before it must match
        assert "consensus_helper.py:490" in ref_err and our_err.code == N.CC_E_KEYERROR, (case.name, ref_err, our_err)
        for k, rel in PARTIAL.items():
            exp = os.path.join(str(d / "oracle"), "sample", rel.replace("ID", "sample"))
            got = os.path.join(str(d / "gpu"), "sample", rel.replace("ID", "sample"))
            if os.path.exists(exp):
                assert_same_in_order(got, exp, "%s %s" % (case.name, k))
        return
    n = 0
    for k, path in ref.items():
        if path.endswith(".bam"):
            assert_same_in_order(ours[k], path, "%s %s" % (case.name, k))
            n += 1
    assert n >= 5
    for k in ("stats", "read_families"):
        assert open(ours[k]).read() == open(ref[k]).read(), (case.name, k)


@pytest.mark.parametrize("name", [n for n in CASES if not n.endswith("-tiny")])
def test_region_loops_match_reference(engine, tmp_path, name):
    assert not _broken, "an earlier case ended in an engine error: %s" % _broken[0]
    case = CASES[name]
    d = tmp_path / "case"
    d.mkdir()
    bam, bed = arrays(engine, case, d)
    pipeline(engine, case, d, bam, bed)
    if case.kind == "keyerror":       # the engine goes on after the error
        tiny = CASES["S-tiny" if case.mode == "sscs" else "P-tiny"]
        d = tmp_path / "after"
        d.mkdir()
        arrays(engine, tiny, d, check=False)
