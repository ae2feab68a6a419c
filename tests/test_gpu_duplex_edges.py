"""The two in-pipeline duplex joins, cc_duplex_consensus (k_dcs_decide_fam, k_dcs_decide) and
cc_singleton_correction (k_sc_decide with k_ht_insert / lookup_ht, k_bucket_geom / k_fam_bucket /
lookup_fam_bucket, k_q_pairs, k_ckey_out) and the vote that follows them (k_duplex_vote_swar, its
b_in_a branch included), at the edges of their geometry: through Engine.read_bam, duplex_consensus and
singleton_correction as DCSRun / SCRun call them, on tables written by the pysam stand-in, against the
dictionaries and loops of tests/duplex_refs.py (pinned to the oracle by tests/test_duplex_refs.py).
dec, t_rec and p_rec are compared per entry slot; every made or corrected slot's consensus row and
five meta fields against tests/vote_refs.py; the kernel scopes say which lookup path ran; two planned
re-runs (another hash seed: another family order inside every position group, another hash layout)
must give the same arrays; and the whole stage is compared with the oracle's, record for record.
Everything compared is an integer, compared for equality.

The cases are tests/duplex_cases.py's: A k_dcs_decide_fam's blocks and halo, F edges, one-tag entries
and orphan tags, B decisions and chains, H the hash table's sizes, C singleton correction, D (and
C-bed) partners of other regions under a bed file of three regions.  Every A
and B case runs per family (default), per entry (CC_DCS_PER_ENTRY) and, with a deep position group
appended, hashed."""
import os
import shutil

import numpy as np
import pytest

import duplex_cases as DC
import duplex_refs as R
import vote_refs as V
from parity import assert_same_records

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in DC.all_cases()}
RUNS = []
for _c in CASES.values():
    if _c.kind == "dcs" and not _c.hashed:
        RUNS += [(_c.name, "default"), (_c.name, "per_entry")]
    else:
        RUNS.append((_c.name, "hashed" if _c.kind == "dcs" else "sc"))
_broken = []     # an engine error ends the module: nothing more is started on a device that may have faulted


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def first_difference(got, want):
    n = min(len(got), len(want))
    bad = np.flatnonzero(np.asarray(got[:n]) != np.asarray(want[:n]))
    return (len(got), len(want)) + ((int(bad[0]), got[bad[0]:bad[0] + 4].tolist(), want[bad[0]:bad[0] + 4].tolist())
                                     if len(bad) else ())


def compare_rows(engine, g, case, dec, t_rec, p_rec, qstride):
    """Every made / corrected slot's consensus row and meta against the duplex restatement."""
    from consensuscruncher_amd.engine import unpack_nibbles
    t = case.table
    sc = case.kind == "sc"
    vslot = engine.fetch(g, "vslot", np.int32)
    meta = engine.fetch(g, "vote_meta", np.int32).reshape(-1, 5)
    rows = lambda a, k: a[:len(a) // k * k].reshape(-1, k)
    seq = unpack_nibbles(rows(engine.fetch(g, "cons_seq", np.uint8), qstride // 2), qstride)
    qual = rows(engine.fetch(g, "cons_qual", np.uint8), qstride)
    n = 0
    for q in np.flatnonzero((dec == 0) | ((dec == 1) if sc else False)):
        a, b = int(t_rec[q]), int(p_rec[q])
        tb = case.sscs if sc and dec[q] == 0 else t
        codes, quals = V.pair_vote(t.codes[a], t.quals[a], tb.codes[b], tb.quals[b], sc)
        w, L = int(vslot[q]), len(codes)
        where = (case.name, int(q), int(dec[q]), a, b, w)
        assert w >= 0 and meta[w][0] == L, where
        bad = np.flatnonzero((seq[w][:L] != codes) | (qual[w][:L] != quals))
        assert len(bad) == 0, where + (bad[:8].tolist(), seq[w][bad[:8]].tolist(), codes[bad[:8]].tolist())
        if sc:
            want = [int(t.mapq[a]), int(t.tlen[a]), int(t.flag[a])]
        else:
            want = [V.most_common_first([int(t.mapq[a]), int(t.mapq[b])]), V.most_common_first([int(t.tlen[a]), int(t.tlen[b])]),
                    V.pick_flag([int(t.flag[a]), int(t.flag[b])])]
        assert meta[w][1:4].tolist() == want and meta[w][4] == -1, where
        n += 1
    return n


@pytest.mark.parametrize("name, path", RUNS)
def test_decisions_match_the_loops(engine, tmp_path, name, path):
    from consensuscruncher_amd.engine import MODE_DUPLEX, Bam, Interner, bed_stream, whole_file_stream
    from consensuscruncher_amd import native as N
    from consensuscruncher_amd import stages
    import cc_oracle
    assert not _broken, "an earlier case ended in an engine error: %s" % _broken[0]
    case = CASES[name]
    t, sc = case.table, case.kind == "sc"
    bed = None
    if case.regions:
        bed = str(tmp_path / "regions.bed")
        with open(bed, "w") as f:
            f.write(DC.bed_text(case.regions))
    if sc:
        res, fam, sfam = R.sc(t, case.sscs, case.regions)
        bam, xbam = str(tmp_path / "x.singleton.sorted.bam"), str(tmp_path / "x.sscs.sorted.bam")
        case.sscs.write(xbam)
    else:
        res, fam = R.dcs(t, case.regions)
        bam, xbam = str(tmp_path / "x.sscs.sorted.bam"), None
    t.write(bam)
    want = res.arrays(fam.n_entries)
    env = {"CC_DCS_PER_ENTRY": "1"} if path == "per_entry" else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    it = Interner()
    tables, groups = [], []
    try:
        bams = [Bam(p) for p in ((bam, xbam) if sc else (bam,))]
        recs = [b.decode(it, MODE_DUPLEX) for b in bams]
        assert recs[0].n == len(t)
        for k, rec in enumerate(recs):
            tables.append(engine.upload(rec))
            stream = bed_stream(rec, bams[k].refs, bed) if bed else whole_file_stream(rec)
            if bed:       # the stream is the one the refs read: each region's records in file order
                want_s = R.region_records(case.sscs if k else t, case.regions)
                assert stream.rec.tolist() == [r for recs_ in want_s for r in recs_]
                assert stream.region.tolist() == [n for n, recs_ in enumerate(want_s) for _ in recs_]
                assert stream.region_run.tolist() == R.region_runs(case.regions)
            groups.append(engine.read_bam(tables[k], stream, 0, 0, scope_by_run=k))
        swap = it.swap_table()
        g = groups[0]
        qstride = (max(r.max_len for r in recs) + 15) & ~15
        join = (lambda: engine.singleton_correction(g, groups[1], swap)) if sc else (lambda: engine.duplex_consensus(g, swap))
        expect = case.engine_error or ("CC_E_KEYERROR" if case.error else None)
        if expect:
            with pytest.raises(N.CCError) as e:
                join()
            assert e.value.code == {v: k for k, v in N.CC_E.items()}[expect], (name, str(e.value))
            print("DUPLEXCASE %s path %s records %d error %s" % (name, path, len(t), expect))
            return
        engine.set_profiling(True)
        engine.profile_only(())
        join()
        kt = engine.kernel_times()
        engine.set_profiling(False)
        got = [engine.fetch(g, k, np.int32) for k in ("dec", "t_rec", "p_rec")]
        F = len(fam.region)
        print("DUPLEXCASE %s path %s records %d F %d Q %d dec %s scopes %s" % (
            name, path, len(t), F, len(want[0]), np.bincount(want[0], minlength=4).tolist(),
            ",".join(k for k in sorted(kt) if k.startswith(("k_dcs", "k_sc", "k_ht", "k_bucket")))))
        for k, field in enumerate(("dec", "t_rec", "p_rec")):
            assert np.array_equal(got[k], want[k]), (field,) + first_difference(got[k], want[k])
        compare_rows(engine, g, case, *got, qstride)
        # which lookups ran
        if bed:       # as observed: a later change of path is noticed
            assert case.ran or case.not_ran
            for scope in case.ran:
                assert scope in kt, (scope, sorted(kt))
            for scope in case.not_ran:
                assert scope not in kt, (scope, sorted(kt))
        elif sc:
            # (an empty SSCS file has no grouping to bucket: the hashed lookups over a table nothing is inserted in)
            assert ("k_ht_insert" in kt) == bool(case.hashed or case.s_hashed), sorted(kt)
            assert ("k_bucket_geom" in kt) == (not case.s_hashed and len(case.sscs) > 0), sorted(kt)
        else:
            assert ("k_ht_insert" in kt) == (path == "hashed"), sorted(kt)
            assert "k_bucket_geom" not in kt
        for seed in (0xabcdef, 0x1234567):      # planned passes
            for x in groups:
                engine.rerun(x, seed)
            join()
            again = [engine.fetch(g, k, np.int32) for k in ("dec", "t_rec", "p_rec")]
            for k in range(3):
                assert np.array_equal(again[k], want[k]), (seed, k) + first_difference(again[k], want[k])
            compare_rows(engine, g, case, *again, qstride)
        for x in groups:
            engine.free_group(x)
        for x in tables:
            engine.free_table(x)
        groups, tables = [], []
        if path == "per_entry":
            return
        # the whole stage against the oracle's, record for record
        ours, ref = tmp_path / "ours", tmp_path / "ref"
        for d in (ours, ref):
            os.makedirs(str(d))
            for p in (bam, xbam):
                if p:
                    shutil.copy(p, str(d))
        if sc:
            run = stages.SCRun(engine, str(ours / "x.singleton.sorted.bam"), bed)
            try:
                run.emit(verbose=False)
            finally:
                run.close()
            cc_oracle.sc_stage(str(ref / "x.singleton.sorted.bam"), bed)
            outs = ("x.sscs.correction.bam", "x.singleton.correction.bam", "x.uncorrected.bam")
        else:
            stages.run_dcs(str(ours / "x.sscs.sorted.bam"), str(ours / "x.dcs.bam"), bed, engine=engine, verbose=False)
            cc_oracle.dcs_stage(str(ref / "x.sscs.sorted.bam"), str(ref / "x.dcs.bam"), bed)
            outs = ("x.dcs.bam", "x.sscs.singleton.bam")
        for k in outs:
            assert_same_records(str(ours / k), str(ref / k), "%s/%s" % (name, k))
    except N.CCError as e:
        _broken.append("%s: %s" % (name, e))
        raise
    finally:
        if not _broken:
            engine.set_profiling(False)
            for x in groups:
                engine.free_group(x)
            for x in tables:
                engine.free_table(x)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_every_class_is_present():
    assert {n[0] for n in CASES} == set("ABCDH")
    base = [c for c in CASES.values() if c.kind == "dcs" and not c.hashed and not c.regions]
    neg = sum(1 for g in DC.GROUPS for s in DC.offsets(g) if s < 0)
    assert sum(1 for c in base if c.name.startswith("A-g")) == neg == 14
    assert sum(1 for c in base if c.name.startswith("B-chain")) == len(DC.CHAIN_HOPS) * len(DC.FAR) + 1
    assert sum(1 for c in CASES.values() if c.name.endswith("+deep")) == len(base)
    assert sum(1 for c in CASES.values() if c.name.startswith("H-F")) == len(DC.HASHED_F)
    assert len(RUNS) == 3 * len(base) + len(DC.HASHED_F) + sum(1 for c in CASES.values() if c.kind == "sc") + 2 * 2
    assert sum(1 for c in CASES.values() if c.regions) == 3
