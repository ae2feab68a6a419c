"""read_bam's mate search (k_scatter_stream, k_deep_qsort / deep_find, k_pair_coord_tile<512 | 1024> with
mate_search_global and mate_record, k_pair_resid, k_lp_hist / k_lp_scatter / k_lp_dups, k_resid_insert /
k_resid_probe / k_resid_probe_sorted / k_resid_pair, and the exact fallback k_pair_mark behind
sort_qname / sort_qname_resid) at the edges of its geometry, through Engine.read_bam on tables written
by the pysam stand-in, against pair_dict restated in tests/pair_refs.py (pinned to the oracle by
tests/test_pair_refs.py).  The completed pairs' records and regions, in the order of the completing
stream entries, and the pair and leftover counts are compared for equality; the kernel scopes say
which path ran; two planned re-runs must give the same arrays; and for tables of at most 10,000
records the whole pipeline is compared with the oracle's, record for record.

The cases are tests/pair_cases.py's: A tile and halo, B deep groups, C stream-order semantics,
D residual paths, E streams and filters, F qname bytes.

Not reachable at these sizes, and left to the pipeline tests: k_lp_dups' over-full bucket (more than
12,288 keys in one of 4,096 hash buckets), and the automatic switch to the 1024 tile at 2^23 records
(the 1024 tile itself runs here under CC_PC_TILE=1024)."""
import os

import numpy as np
import pytest

import pair_cases as PC
from parity import assert_same_records

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in PC.all_cases()}
OUTS = ("sscs", "singleton", "badreads", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction",
        "uncorrected", "sscs_sc", "dcs_sc", "sscs_sc_singleton", "all_unique")
_broken = []     # an engine error ends the module: nothing more is started on a device that may have faulted
_oracle = {}     # table -> the oracle pipeline's outputs (cases that differ in their switches share them)


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def fetch_pairs(engine, g):
    return [engine.fetch(g, name, np.int32) for name in ("pr_rec1", "pr_rec2", "pr_region")]


def first_difference(got, want):
    n = min(len(got), len(want))
    bad = np.flatnonzero(np.asarray(got[:n]) != np.asarray(want[:n]))
    return (len(got), len(want)) + ((int(bad[0]), got[bad[0]:bad[0] + 4].tolist(), want[bad[0]:bad[0] + 4].tolist())
                                     if len(bad) else ())


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_match_pair_dict(engine, tmp_path, name):
    from consensuscruncher_amd.engine import MODE_SSCS, Bam, Interner, Stream
    from consensuscruncher_amd import native as N
    assert not _broken, "an earlier case ended in an engine error: %s" % _broken[0]
    case = CASES[name]
    table = case.table
    pairs, pending = case.expected()
    want = [np.array([p[k] for p in pairs], np.int32) for k in range(3)]
    bam = str(tmp_path / "sample.bam")
    table.write(bam)
    rec = Bam(bam).decode(Interner(), MODE_SSCS, "|")
    assert rec.n == len(table)
    stream = Stream(case.stream, case.region, np.zeros(case.n_regions, np.int32), None)
    old = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    tid = g = None
    try:
        tid = engine.upload(rec)
        engine.set_profiling(True)
        engine.profile_only(())
        g = engine.read_bam(tid, stream, case.delim_filter, case.badread, 0)
        kt = engine.kernel_times()
        engine.set_profiling(False)
        got = fetch_pairs(engine, g)
        cnt = engine.counters(g)
        print("PAIRCASE %s records %d entries %d pairs %d pending %d scopes %s" % (
            name, len(table), len(case.stream), len(pairs), pending,
            ",".join(k for k in sorted(kt) if k.startswith(("k_pair", "k_deep_q", "k_lp", "sort_q")))))
        for k, field in enumerate(("pr_rec1", "pr_rec2", "pr_region")):
            assert np.array_equal(got[k], want[k]), (field,) + first_difference(got[k], want[k])
        assert cnt["PAIRS"] == len(pairs) and cnt["UNPAIRED"] == pending, cnt
        for scope in case.ran:
            assert scope in kt, (scope, sorted(kt))
        for scope in case.not_ran:
            assert scope not in kt, (scope, sorted(kt))
        for seed in (0xabcdef, 0x1234567):      # planned passes
            engine.rerun(g, seed)
            again = fetch_pairs(engine, g)
            for k in range(3):
                assert np.array_equal(again[k], want[k]), (seed, k) + first_difference(again[k], want[k])
            cnt = engine.counters(g)
            assert cnt["PAIRS"] == len(pairs) and cnt["UNPAIRED"] == pending, (seed, cnt)
        engine.free_group(g)
        g = None
        engine.free_table(tid)
        tid = None
        if case.pipeline:
            import cc_oracle
            from consensuscruncher_amd.pipeline import consensus_pipeline
            if id(table) not in _oracle:
                try:
                    _oracle[id(table)] = cc_oracle.consensus_pipeline(bam, str(tmp_path / "oracle"))
                except cc_oracle.OracleError as e:      # (no pair at all: the reference's empty family table)
                    _oracle[id(table)] = e
            ref = _oracle[id(table)]
            if isinstance(ref, cc_oracle.OracleError):
                assert str(ref).startswith("IndexError") and not pairs
                with pytest.raises(IndexError):
                    consensus_pipeline(bam, str(tmp_path / "ours"), engine=engine)
                return
            ours = consensus_pipeline(bam, str(tmp_path / "ours"), engine=engine)
            n = 0
            for k in OUTS:
                if k in ref:
                    assert_same_records(ours[k], ref[k], "%s/%s" % (name, k))
                    n += 1
            assert n >= 5
    except N.CCError as e:
        _broken.append("%s: %s" % (name, e))
        raise
    finally:
        if not _broken:
            engine.set_profiling(False)
            if g is not None:
                engine.free_group(g)
            if tid is not None:
                engine.free_table(tid)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_every_class_is_present():
    assert {n[0] for n in CASES} == set("ABCDEF")
    for T in PC.TILES:
        assert sum(1 for c in CASES.values() if c.name[0] in "AB" and c.tile == T) == 15
    assert all(CASES[n].env.get("CC_PC_TILE") == "1024" for n in CASES if n.endswith("T1024"))
