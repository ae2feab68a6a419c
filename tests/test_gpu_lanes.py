"""Stage passes on their own lanes (CC_LANES): groups are bound to one of up to four
streams, a pass waits for exactly the groups and tables it reads, and each group owns its error
word, counters and guard word.  Lanes must change no result: the chain bench.py builds
(build_stages) is run in fresh child processes with CC_LANES=1 and CC_LANES=4 -- without a bed
file and with a bed file of two regions -- and every array bench.py's stage_outputs fetches and
every counter is compared byte for byte, after the setup and after each step.

One child does, in this order (each snapshot is every stage's arrays and counters):
  setup        the first (exact) pass of build_stages
  step0..2     three deferred steps in bench order
  reversed     one deferred step with the stage calls enqueued last stage first (SC before DCS)
  interleaved  one deferred step as gs' pass, the DCS stage, then the join of gs with the DCS grouping
  replay       one deferred step with one group's plan skewed (cc_debug_skew_plan): the step replays
  freed        one deferred step in which the last stage's group and table are freed while the other
               lanes have work queued
The stages' results do not depend on the step's seed, so every snapshot of one child equals its
setup snapshot, and the two children's snapshots equal each other.  Because equal bytes alone would
not show a skipped wait, the child also records each group's re-run and lane-wait counts
(cc_group_reruns): under four lanes the join must have made its lane wait for the DCS grouping, and
the DCS group's next pass for the join; under one lane nothing waits.

Two more tests run in this process on one engine with the default lanes: a group that returns
CC_E_KEYERROR (the golden bed_overlap case) beside a clean group in one deferred step, and the
guards' test (stale slots, tests/test_gpu_deferred.py) applied to one group beside a second."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 20_000
ARRAYS = {
    "sscs": ("emit_n", "emit_vslot", "emit_rec", "emit_ckey", "fam_sizes_by_creation", "bad_rec", "vote_meta",
             "cons_qual", "cons_seq"),
    "dcs": ("dec", "vslot", "t_rec", "p_rec", "vote_meta", "cons_qual", "cons_seq"),
    "sc": ("dec", "vslot", "t_rec", "q_ckey", "vote_meta", "cons_qual", "cons_seq"),
    "dcs_sc": ("dec", "vslot", "t_rec", "p_rec", "vote_meta", "cons_qual", "cons_seq"),
}


def _reruns(eng, g):
    """(exact re-runs of planned passes, those after a guarded index, waits on other lanes' events) of group g"""
    a = np.zeros(3, np.int64)
    assert eng.lib.cc_group_reruns(eng.h, g, a.ctypes.data_as(N_i64p())) == 0
    return [int(x) for x in a]


def N_i64p():
    from consensuscruncher_amd import native as N
    return N.i64p


def _groups(runs):
    return {tag: (r.gs if tag == "sc" else r.g) for tag, r in runs}


def _snapshot(eng, runs):
    import hashlib
    out = {}
    for tag, r in runs:
        g = r.gs if tag == "sc" else r.g
        for a in ARRAYS[tag]:
            b = eng.fetch(g, a, np.uint8).tobytes()
            out["%s.%s" % (tag, a)] = "%d:%s" % (len(b), hashlib.sha256(b).hexdigest())
        out["%s.counters" % tag] = sorted(eng.counters(g).items())
    return out


def _child(work, bed, out_path):
    sys.path.insert(0, ROOT)
    import bench
    from consensuscruncher_amd import synth
    from consensuscruncher_amd.engine import Engine
    batch = synth.generate(PAIRS, seed=synth.SEED_BASE + 4111, contigs=(("chr1", 600_000),))
    inp = os.path.join(work, "sample.bam")
    synth.write_bam_native(batch, inp, level=1)
    eng = Engine(0)
    runs, _ = bench.build_stages(eng, work, inp, 0.7, bed or None)
    r = dict(runs)
    res = {"setup": _snapshot(eng, runs)}
    for i in range(3):
        eng.deferred(lambda: [x.step(0x5eed + 7919 * i) for _, x in runs])
        res["step%d" % i] = _snapshot(eng, runs)
    eng.deferred(lambda: [x.step(0x101) for _, x in reversed(runs)])
    res["reversed"] = _snapshot(eng, runs)

    sc = r["sc"]
    gids = _groups(runs)
    w0 = {t: _reruns(eng, g)[2] for t, g in gids.items()}

    def interleaved():
        eng.derive(sc.ts)
        eng.rerun(sc.gs, 0x202)
        r["dcs"].step(0x202)
        if not sc.x_shared:
            eng.derive(sc.tx)
            eng.rerun(sc.gx, 0x202)
        eng.singleton_correction(sc.gs, sc.gx, sc.swap)
        r["dcs_sc"].step(0x202)
        r["sscs"].step(0x202)
    eng.deferred(interleaved)
    res["interleaved"] = _snapshot(eng, runs)
    # the join waited for the grouping it reads; that grouping's next pass waits for the join
    w1 = {t: _reruns(eng, g)[2] for t, g in gids.items()}
    res["join_waits"] = w1["sc"] - w0["sc"]
    r["dcs"].step(0x203)
    res["dcs_waits_after_join"] = _reruns(eng, gids["dcs"])[2] - w1["dcs"]
    res["shared_x"] = bool(sc.x_shared)

    # one group's plan skewed (the csn sharing flag: a valid computation on either value, see
    # test_gpu_deferred.py): the commit asks for a replay, the replay re-runs that pass exactly
    n = []
    before = {t: _reruns(eng, g)[0] for t, g in gids.items()}
    assert eng.lib.cc_debug_skew_plan(eng.h, r["dcs"].g, b"csn_shared", 1) == 0

    def skewed():
        n.append(1)
        for _, x in runs:
            x.step(0x303)
    eng.deferred(skewed)
    res["replay_calls"] = len(n)
    res["replay_reruns"] = {t: _reruns(eng, g)[0] - before[t] for t, g in gids.items()}
    res["replay"] = _snapshot(eng, runs)

    # the last stage's group and table freed between the other stages' passes of one deferred step
    def freeing():
        r["sscs"].step(0x404)
        r["dcs"].step(0x404)
        r["dcs_sc"].close()
        sc.step(0x404)
    eng.deferred(freeing)
    res["freed"] = _snapshot(eng, runs[:3])
    for _, x in runs[:3]:
        x.close()
    eng.close()
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module", params=["nobed", "bed"])
def children(request, tmp_path_factory):
    """{lanes: the child's snapshots} for CC_LANES=1 and CC_LANES=4 on one input."""
    out = {}
    for lanes in (1, 4):
        d = str(tmp_path_factory.mktemp("lanes_%s_%d" % (request.param, lanes)))
        bed = ""
        if request.param == "bed":
            bed = os.path.join(d, "two.bed")
            with open(bed, "w") as f:
                f.write("chr1\t0\t300000\tp\nchr1\t300000\t600000\tq\n")
        env = dict(os.environ, CC_LANES=str(lanes))
        res = os.path.join(d, "result.json")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), d, bed, res], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
        with open(res) as f:
            out[lanes] = json.load(f)
    return out


def _diff(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def test_lanes_change_no_result(children):
    """Setup and three steps: CC_LANES=4 leaves what CC_LANES=1 leaves."""
    for name in ("setup", "step0", "step1", "step2"):
        assert _diff(children[1][name], children[4][name]) == [], name
        assert _diff(children[4]["setup"], children[4][name]) == [], name


@pytest.mark.parametrize("order", ["reversed", "interleaved"])
def test_enqueue_order_changes_no_result(children, order):
    """A pass waits for the groups and tables it reads, whatever the order the host enqueued them in."""
    for lanes in (1, 4):
        assert _diff(children[lanes]["setup"], children[lanes][order]) == [], (lanes, order)


def test_join_waits_for_the_grouping_it_reads(children):
    """The waits themselves (equal bytes would not show a skipped one): with four lanes the join of gs
    with the DCS run's grouping waited for it, and that group's next pass waited for the join."""
    assert children[1]["join_waits"] == 0 and children[1]["dcs_waits_after_join"] == 0
    if children[4]["shared_x"]:   # (with a bed file SC groups its SSCS side itself: gx is not the DCS group)
        assert children[4]["join_waits"] >= 1
        assert children[4]["dcs_waits_after_join"] >= 1


def test_deferred_replay_under_lanes(children):
    for lanes in (1, 4):
        assert children[lanes]["replay_calls"] == 2
        # only the skewed group counts a re-run
        assert children[lanes]["replay_reruns"] == {"sscs": 0, "dcs": 1, "sc": 0, "dcs_sc": 0}, lanes
        assert _diff(children[lanes]["setup"], children[lanes]["replay"]) == [], lanes


def test_free_while_other_lanes_have_work(children):
    for lanes in (1, 4):
        ref = {k: v for k, v in children[lanes]["setup"].items() if not k.startswith("dcs_sc.")}
        assert _diff(ref, children[lanes]["freed"]) == [], lanes


# ---- one engine, default lanes: what is per group stays with its group

@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_error_stays_with_its_group(engine, tmp_path):
    """One group returns CC_E_KEYERROR (tests/golden/bed_overlap: a record fetched by two overlapping bed
    regions, consensus_helper.py:490) while a clean group runs in the same deferred step: the clean
    group returns 0 with its outputs unchanged, the other its own code and message, as alone."""
    import ctypes as C
    from consensuscruncher_amd import native as N, synth
    from consensuscruncher_amd.engine import MODE_SSCS, Bam, Interner, bed_stream
    from consensuscruncher_amd.stages import SSCSRun
    eng = engine
    inp = str(tmp_path / "good.bam")
    synth.write_bam_native(synth.generate(2_000, seed=synth.SEED_BASE + 4112, contigs=(("chr1", 200_000),)), inp, level=1)
    good = SSCSRun(eng, inp, 0.7)
    runs = [("sscs", good)]
    ref = _snapshot(eng, runs)

    d = os.path.join(ROOT, "tests", "golden", "bed_overlap")
    bam = Bam(os.path.join(d, "input.bam"))
    rec = bam.decode(Interner(), MODE_SSCS, "|")
    stream = bed_stream(rec, bam.refs, os.path.join(d, "regions.bed"))
    table = eng.upload(rec)
    prm = N.cc_read_bam_params(1, 1, 0, 0, 0x5eed)
    gid = C.c_int32(0)
    rc = eng.lib.cc_read_bam(eng.h, table, stream.n, N.ptr(stream.rec), N.ptr(stream.region), len(stream.region_run),
                             N.ptr(stream.region_run), C.byref(prm), C.byref(gid))
    alone = (rc, eng.lib.cc_last_error(eng.h))
    assert rc == N.CC_E_KEYERROR, alone
    try:
        for order in (0, 1):
            got = []

            def calls():
                if order == 0:
                    got.append((eng.lib.cc_read_bam_rerun(eng.h, gid.value, 0x5eed), eng.lib.cc_last_error(eng.h)))
                good.step(0x600 + order)
                if order == 1:
                    got.append((eng.lib.cc_read_bam_rerun(eng.h, gid.value, 0x5eed), eng.lib.cc_last_error(eng.h)))
            eng.deferred(calls)   # (raises if the clean group's pass or the commit returned a code)
            assert got == [alone], order
            assert _diff(ref, _snapshot(eng, runs)) == [], order
            assert _reruns(eng, good.g)[:2] == [0, 0]
    finally:
        eng.lib.cc_group_free(eng.h, gid.value)
        eng.free_table(table)
        good.close()


def test_guard_stays_with_its_group(engine, tmp_path):
    """tests/test_gpu_deferred.py::test_guarded_stale_slots_rerun_exactly's setup on the SSCS group, with the
    DCS group's step enqueued beside it: the SSCS group's guards fire and its pass re-runs exactly,
    the DCS group counts no re-run, and every result is the exact run's."""
    import bench
    from consensuscruncher_amd import synth
    eng = engine
    d = str(tmp_path)
    inp = os.path.join(d, "sample.bam")
    synth.write_bam_native(synth.generate(PAIRS, seed=synth.SEED_BASE + 4113, contigs=(("chr1", 600_000),)), inp, level=1)
    runs, _ = bench.build_stages(eng, d, inp, 0.7)
    try:
        r = dict(runs)
        eng.deferred(lambda: [x.step(0x700) for _, x in runs])   # (every group has run planned once)
        ref = _snapshot(eng, runs)
        g, other = r["sscs"].g, r["dcs"].g
        b_g, b_o = _reruns(eng, g), _reruns(eng, other)
        for name in ("needv", "emit_span", "emit_fam"):
            used = eng.lib.cc_fetch(eng.h, g, name.encode(), None, 0)
            assert used > 0
            assert eng.lib.cc_debug_poison(eng.h, g, name.encode(), used + (1 << 16), 0x7f) == 0
        assert eng.lib.cc_debug_skew_plan(eng.h, g, b"scan_emit", 256) == 0

        def calls():
            eng.consensus_maker(g, 0.7)
            r["dcs"].step(0x701)
        eng.deferred(calls)
        a_g, a_o = _reruns(eng, g), _reruns(eng, other)
        assert a_g[1] > b_g[1] and a_g[0] > b_g[0]
        assert a_o[:2] == b_o[:2]
        assert _diff(ref, _snapshot(eng, runs)) == []
    finally:
        for _, x in runs:
            x.close()


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3])
