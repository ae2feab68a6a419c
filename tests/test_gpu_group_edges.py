"""read_bam's read-end grouping at the edges of its geometry, through Engine.read_bam on tables written by
the pysam stand-in, against read_dict / tag_dict / csn_pair_dict restated in tests/group_refs.py (pinned to
the oracle by tests/test_group_refs.py).

Kernels covered: k_group_count / k_group_flags (CC_GROUP_STAGED), k_group_rank<true | false> (by record, or
by pair under CC_GR_BY_PAIR and wherever the plan says most ends are deep), k_deep_count, k_deep_fam,
k_deep_emit, k_deep_sortfam's bitmap rank, k_big_keys / sort_tags_big (a group of more than DF_FAMS
families, a family of more than DF_SORT ends, CC_DEEP_SORT), sort_tags / k_fam_mark / k_fam_dedup (an
unsorted table), the EmitFamStarts scan, k_fam_build, the EmitCreation scan, k_csn_fast and its exact
fallback k_csn_keys / sort_csn / k_csn_mark / k_csn_entries.

The cases are tests/group_cases.py's: A small position groups on the ranking tile's edges, B families
inside small groups, C deep groups, D creation order and csn_pair_dict, E an unsorted table.  Every array
is compared for equality in a form that does not depend on the seeded hash: families are named by their
first read end.  The kernel scopes say which path ran; two planned re-runs with other seeds must give the
same result (on mixed tables the planned pass ranks with the other k_group_rank variant); classes A-C
run again under CC_GR_BY_PAIR, a reduced draw under CC_GROUP_STAGED and CC_DEEP_SORT; and for tables of
at most 10,000 records on an identity stream the whole pipeline is compared with the oracle's, record
for record.

Left to the pipeline tests:
  * a 64-bit tag-hash collision (EB_COLLISION): no switch narrows the tag hash, and none is added here;
  * k_deep_sortfam's merge-sort branch: it needs a family's ends 32 * DF_SORT = 262,144 end indices
    apart.  A family's tag holds its own and its mate's position, so all its pairs complete inside one
    position group (the later of the two), one after the other in an identity stream; end indices are
    2 * pair + side, so the family's group would have to complete more than 131,072 pairs, and hold as
    many records.  Not reachable below the 20,000 records of a table here;
  * more deep groups than k_deep_fam's grid (CC_DF_GRID = 8192): 532,545 records."""
import os

import numpy as np
import pytest

import group_cases as GC
from parity import assert_same_records

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in GC.all_cases()}
OUTS = ("sscs", "singleton", "badreads", "dcs", "sscs_singleton", "sscs_correction", "singleton_correction",
        "uncorrected", "sscs_sc", "dcs_sc", "sscs_sc_singleton", "all_unique")
ARRAYS = (("rs_val", np.uint32), ("mem_rec", np.int32), ("segf", np.uint8), ("mem_valid", np.uint32),
          ("fam_beg", np.int32), ("fam_end", np.int32), ("fam_n", np.int32), ("fam_first", np.int32),
          ("fam_region", np.int32), ("fam_by_k", np.int32), ("fam_sizes_by_creation", np.int32),
          ("ent_f", np.int32), ("ent_pair", np.int32), ("has2", np.uint8), ("pr_rec1", np.int32), ("pr_rec2", np.int32))
_broken = []     # an engine error ends the module: nothing more is started on a device that may have faulted
_oracle = {}     # table -> the oracle pipeline's outputs (cases that differ in their switches share them)
_expected = {}   # table, stream -> (pairs, the reference's grouping)


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def expected(case):
    key = (id(case.table), id(case.stream))
    if key not in _expected:
        _expected[key] = GC.grouping(case)
    return _expected[key]


def same(got, want, what, at):
    """Array equality, the first difference reported with its place."""
    got, want = np.asarray(got), np.asarray(want)
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, at(int(bad[0])), got[bad[0]:bad[0] + 4].tolist(), want[bad[0]:bad[0] + 4].tolist())


def check_grouping(engine, g, pairs, ref, tag):
    cnt = engine.counters(g)
    P, R, F, E = len(pairs), 2 * len(pairs), len(ref.families), len(ref.names)
    want_cnt = dict(PAIRS=P, READ_ENDS=R, FAMILIES=F, ENTRIES=E, ORPHAN_TAGS=ref.orphans, DROPPED=len(ref.dropped))
    assert {k: cnt[k] for k in want_cnt} == want_cnt, tag
    a = {name: engine.fetch(g, name, dt) for name, dt in ARRAYS}
    for name in ("rs_val", "mem_rec", "segf", "mem_valid"):
        assert len(a[name]) >= R, (tag, name)
        a[name] = a[name][:R]
    for name in ("fam_beg", "fam_end", "fam_n", "fam_first", "fam_region", "fam_by_k", "fam_sizes_by_creation"):
        assert len(a[name]) >= F, (tag, name)
        a[name] = a[name][:F]
    ends = np.array([p[k] for p in pairs for k in (0, 1)], np.int32)           # read end -> record
    rs = a["rs_val"].astype(np.int64)

    def slot(j):      # a slot's place: its end, record and offset in the ranking tile
        e = int(rs[j]) if rs[j] < R else -1
        r = int(ends[e]) if e >= 0 else -1
        return dict(slot=j, end=e, record=r, tile_offset=r % GC.GT, family_start=bool(a["segf"][j]))

    def fam(f):
        return dict(family=f, **slot(int(a["fam_beg"][f])))

    same(a["pr_rec1"][:P], ends[0::2], tag + ("pr_rec1",), lambda i: i)
    same(a["pr_rec2"][:P], ends[1::2], tag + ("pr_rec2",), lambda i: i)
    # every end in exactly one slot, beside its record
    same(np.sort(rs), np.arange(R), tag + ("rs_val holds every end once",), lambda i: i)
    same(a["mem_rec"], ends[rs], tag + ("mem_rec",), slot)
    # family starts and ends
    same(np.flatnonzero(a["segf"]), a["fam_beg"], tag + ("segf against fam_beg",), lambda i: i)
    same(a["fam_end"], np.concatenate([a["fam_beg"][1:], [R]]), tag + ("fam_end",), fam)
    same(a["fam_first"], rs[a["fam_beg"]], tag + ("fam_first",), fam)
    # members in completion order, the families' slots the reference's, named by their first end
    inside = np.ones(R, bool)
    inside[a["fam_beg"]] = False
    rising = np.concatenate([[True], rs[1:] > rs[:-1]])
    same(rising | ~inside, np.ones(R, bool), tag + ("rs_val ascending inside a family",), slot)
    fam_of_slot = np.cumsum(a["segf"].astype(np.int64)) - 1
    by_first = {f.first: k for k, f in enumerate(ref.families)}
    missing = [fam(f) for f in range(F) if int(a["fam_first"][f]) not in by_first][:1]
    assert not missing, tag + ("a family the reference does not start",) + tuple(missing)
    ref_of = np.array([by_first[int(x)] for x in a["fam_first"]], np.int64)        # engine family -> reference family
    same(ref_of[fam_of_slot], np.asarray(ref.family_of, np.int64)[rs], tag + ("the family of each slot's end",), slot)
    dropped = np.zeros(R, bool)
    dropped[sorted(ref.dropped)] = True
    same(a["mem_valid"] == 0, dropped[rs], tag + ("mem_valid",), slot)
    sizes = np.array([len(f.members) for f in ref.families], np.int32)
    regions = np.array([f.region for f in ref.families], np.int32)
    same(a["fam_n"], sizes[ref_of], tag + ("fam_n",), fam)
    same(a["fam_region"], regions[ref_of], tag + ("fam_region",), fam)
    # tag_dict insertion order
    same(a["fam_first"][a["fam_by_k"]], [f.first for f in ref.families], tag + ("fam_first[fam_by_k]",), lambda i: i)
    same(a["fam_sizes_by_creation"], sizes, tag + ("fam_sizes_by_creation",), lambda i: i)
    # csn_pair_dict
    assert len(a["ent_f"]) >= 2 * E and len(a["ent_pair"]) >= E and len(a["has2"]) >= E, tag
    ent = a["ent_f"][:2 * E].reshape(E, 2)
    first = np.concatenate([a["fam_first"], [-1]])
    want = np.full((E, 2), -1, np.int64)
    for r, name in enumerate(ref.names):
        for k, f in enumerate(ref.entries[name]):
            want[r, k] = ref.families[f].first
    assert ent.min(initial=0) >= -1 and ent.max(initial=0) < F, tag
    same(first[ent[:, 0]], want[:, 0], tag + ("ent_f: the entries' first families",), lambda i: i)
    same(first[ent[:, 1]], want[:, 1], tag + ("ent_f: the entries' second families",), lambda i: i)
    same(a["has2"][:E], want[:, 1] >= 0, tag + ("has2",), lambda i: i)
    same(a["ent_pair"][:E], want[:, 0] >> 1, tag + ("ent_pair",), lambda i: i)


@pytest.mark.parametrize("name", list(CASES))
def test_grouping_matches_reference(engine, tmp_path, name):
    from consensuscruncher_amd.engine import MODE_SSCS, Bam, Interner, Stream
    from consensuscruncher_amd import native as N
    assert not _broken, "an earlier case ended in an engine error: %s" % _broken[0]
    case = CASES[name]
    table = case.table
    pairs, ref = expected(case)
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
        print("GROUPCASE %s records %d pairs %d families %d entries %d dropped %d orphans %d scopes %s" % (
            name, len(table), len(pairs), len(ref.families), len(ref.names), len(ref.dropped), ref.orphans,
            ",".join(k for k in sorted(kt) if k.startswith(("k_group", "k_deep", "k_fam", "k_csn", "sort_")))))
        check_grouping(engine, g, pairs, ref, (name, "exact"))
        for scope in case.ran:
            assert scope in kt, (scope, sorted(kt))
        for scope in case.not_ran:
            assert scope not in kt, (scope, sorted(kt))
        for seed in (0xabcdef, 0x1234567):      # planned passes
            engine.rerun(g, seed)
            check_grouping(engine, g, pairs, ref, (name, "planned", seed))
        engine.free_group(g)
        g = None
        engine.free_table(tid)
        tid = None
        if case.pipeline:
            import cc_oracle
            from consensuscruncher_amd.pipeline import consensus_pipeline
            if id(table) not in _oracle:
                _oracle[id(table)] = cc_oracle.consensus_pipeline(bam, str(tmp_path / "oracle"))
            ref_out = _oracle[id(table)]
            ours = consensus_pipeline(bam, str(tmp_path / "ours"), engine=engine)
            n = 0
            for k in OUTS:
                if k in ref_out:
                    assert_same_records(ours[k], ref_out[k], "%s/%s" % (name, k))
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
    base = [c for c in CASES.values() if c.switch is None]
    assert {k: sum(1 for c in base if c.name[0] == k) for k in "ABCDE"} == dict(A=14, B=1, C=10, D=5, E=1)
    by_switch = {s: [c for c in CASES.values() if c.switch == s] for s in ("CC_GR_BY_PAIR", "CC_GROUP_STAGED", "CC_DEEP_SORT")}
    assert sorted(c.name[0] for c in by_switch["CC_GR_BY_PAIR"]) == ["A"] * 14 + ["B"] + ["C"] * 10
    assert {c.name[0] for c in by_switch["CC_GROUP_STAGED"]} == set("ABCDE") and len(by_switch["CC_GROUP_STAGED"]) == 7
    deep_sort = by_switch["CC_DEEP_SORT"]
    assert {c.name[0] for c in deep_sort} == set("ABCDE") and sum(1 for c in deep_sort if c.name[0] == "C") == 10
    assert len(deep_sort) == 14 and len(CASES) == 31 + 25 + 7 + 14
    assert all(c.env == {c.switch: "1"} for s in by_switch.values() for c in s)
    assert sum(1 for c in base if c.pipeline) >= 20
