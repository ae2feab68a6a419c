"""The entry points that take a buffer's or a planned total's name (cc_fetch, cc_debug_poison,
cc_debug_skew_plan) and the profile scopes named after planned totals: the engine keeps buffers and
totals in tables indexed by id, and these resolve the name through the tables' name lists.  Every
array the stages fetch must resolve; an unknown name, and a known one the group never allocated or
recorded, must be refused with CC_E_INVALID and the message the callers know."""
import os

import pytest

pytestmark = pytest.mark.gpu

CC_E_INVALID = -1   # include/consensuscruncher_amd.h

# what stages.py fetches from each run's group (SSCSRun.emit, DCSRun.emit, SCRun.emit)
FETCHED = {
    "sscs": ("emit_n", "emit_rec", "emit_vslot", "emit_ckey", "vote_meta", "cons_seq", "cons_qual", "bad_rec",
             "fam_sizes_by_creation"),
    "dcs": ("dec", "t_rec", "p_rec", "vslot", "vote_meta", "cons_seq", "cons_qual"),
    "sc": ("dec", "t_rec", "vslot", "q_ckey", "vote_meta", "cons_seq", "cons_qual"),
}


@pytest.fixture(scope="module")
def stages(tmp_path_factory):
    import bench
    from consensuscruncher_amd import synth
    from consensuscruncher_amd.engine import Engine
    d = str(tmp_path_factory.mktemp("named"))
    batch = synth.generate(2000, seed=synth.SEED_BASE + 733, contigs=(("chr1", 200_000),))
    inp = os.path.join(d, "sample.bam")
    synth.write_bam_native(batch, inp, level=1)
    eng = Engine(0)
    runs, _ = bench.build_stages(eng, d, inp, 0.7)
    yield eng, dict(runs)
    for r in runs:
        r[1].close()
    eng.close()


def _group(runs, tag):
    return runs[tag].gs if tag == "sc" else runs[tag].g


def _err(eng):
    return eng.lib.cc_last_error(eng.h).decode()


def test_fetched_names_resolve(stages):
    eng, runs = stages
    for tag, names in FETCHED.items():
        g = _group(runs, tag)
        for name in names:
            first = eng.lib.cc_fetch(eng.h, g, name.encode(), None, 0)
            again = eng.lib.cc_fetch(eng.h, g, name.encode(), None, 0)
            assert first >= 0 and first == again, (tag, name, first, again, _err(eng))
    # results exist at this size: the byte counts above are not all zero
    assert eng.lib.cc_fetch(eng.h, _group(runs, "sscs"), b"cons_qual", None, 0) > 0


def test_fetch_refuses_unknown_and_unallocated(stages):
    eng, runs = stages
    g = _group(runs, "sscs")
    assert eng.lib.cc_fetch(eng.h, g, b"no_such_array", None, 0) == CC_E_INVALID
    assert "no_such_array" in _err(eng)
    # declared (singleton correction's output names), never allocated by a group that has only run SSCS
    assert eng.lib.cc_fetch(eng.h, g, b"q_ckey", None, 0) == CC_E_INVALID
    assert "no result array named" in _err(eng) and "q_ckey" in _err(eng)


def test_debug_hooks_refuse_unknown_names(stages):
    eng, runs = stages
    g = _group(runs, "sscs")
    assert eng.lib.cc_debug_poison(eng.h, g, b"no_such_array", 64, 0) == CC_E_INVALID
    assert "no_such_array" in _err(eng)
    assert eng.lib.cc_debug_skew_plan(eng.h, g, b"no_such_total", 1) == CC_E_INVALID
    assert "no_such_total" in _err(eng)
    # a known total this group has not recorded: singleton correction has not run on it
    assert eng.lib.cc_debug_skew_plan(eng.h, g, b"scan_sc", 1) == CC_E_INVALID
    assert "no planned total named" in _err(eng)
    # ... and one it has (a zero shift: the plan stays as it was)
    assert eng.lib.cc_debug_skew_plan(eng.h, g, b"scan_emit", 0) == 0


def test_profile_scopes_keep_their_names(stages):
    eng, runs = stages
    eng.set_profiling(True)
    try:
        runs["sscs"].step(0x51)
        runs["dcs"].step(0x51)
        times = eng.kernel_times()
    finally:
        eng.set_profiling(False)
    for scope in ("scan_pairs", "scan_fam", "scan_emit", "k_duplex_vote_dcs"):
        assert scope in times and times[scope][1] > 0, (scope, sorted(times))
