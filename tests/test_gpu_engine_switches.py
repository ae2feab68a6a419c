"""The engine's measurement switches (INTEGRATION.md "Engine switches") change no output: the whole
pipeline with each switch set, record for record against the default run on the same input."""
import os

import pytest

pytestmark = pytest.mark.gpu

# CC_QDIG_BITS=10 keeps 10 bits of the tables' qname digests: the seeded keys collide everywhere.  Two
# found pairs with one key first send the pass to the sort path (EB_NEEDSORT); k_pair_mark's qname
# compare meets EB_COLLISION there, and the pass re-runs on the full qname hash (read_bam_run)
SWITCHES = [("CC_PC_TILE", "1024"), ("CC_PC_TILE", "512"), ("CC_RESID_SORT", "1"), ("CC_SCAN1", "1"),
            ("CC_SCAN1", "0"), ("CC_QDIG", "0"), ("CC_QDIG_BITS", "10"), ("CC_DCS_PER_ENTRY", "1"),
            ("CC_LP_MIN", "0"), ("CC_GROUP_STAGED", "1"),
            ("CC_RESID_SCAN", "1"), ("CC_META_SCALAR", "1"), ("CC_DERIVE_SEPARATE", "1"),
            ("CC_GR_BY_PAIR", "1")]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from consensuscruncher_amd import synth
    from consensuscruncher_amd.engine import Engine
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = tmp_path_factory.mktemp("switches")
    batch = synth.generate(40_000, seed=synth.SEED_BASE + 931)
    bam = str(d / "s.bam")
    synth.write_bam_native(batch, bam)
    e = Engine(0)
    base = consensus_pipeline(bam, str(d / "base"), engine=e)
    yield e, bam, d, base
    e.close()


@pytest.mark.parametrize("name,value", SWITCHES)
def test_switch_changes_no_output(case, name, value):
    from parity import assert_same_records
    from consensuscruncher_amd.pipeline import consensus_pipeline
    e, bam, d, base = case
    os.environ[name] = value
    try:
        got = consensus_pipeline(bam, str(d / ("%s_%s" % (name, value))), engine=e)
    finally:
        os.environ.pop(name, None)
    assert sorted(got) == sorted(base)
    n = 0
    for k in base:
        if not (isinstance(base[k], str) and os.path.isfile(base[k])):
            continue
        if base[k].endswith(".bam"):
            assert_same_records(got[k], base[k], "%s=%s/%s" % (name, value, k))
        else:
            assert open(got[k], "rb").read() == open(base[k], "rb").read(), k
        n += 1
    assert n >= 5


@pytest.mark.parametrize("kind", ["deep", "dupq"])
def test_partitioned_pair_check_equals_table(kind, tmp_path):
    """The partitioned check for a qname in two found pairs (k_lp_hist / k_lp_scatter / k_lp_dups,
    CC_LP_MIN=0: every pass) against the long-pair table (CC_LTAB_CAS=1), record for record: deep
    position groups whose pairs are all long, and qnames seen three and four times (the check must
    send those passes to the sort path exactly as the table does)."""
    from parity import assert_same_records
    from consensuscruncher_amd import synth
    from consensuscruncher_amd.engine import Engine
    from consensuscruncher_amd.pipeline import consensus_pipeline
    kw = dict(loci=12, zipf_s=1.2, max_fam=400) if kind == "deep" else dict(dupq_frac=0.02)
    batch = synth.generate(30_000, seed=synth.SEED_BASE + 977, contigs=(("chr1", 400_000),), **kw)
    bam = str(tmp_path / "s.bam")
    synth.write_bam_native(batch, bam)
    e = Engine(0)
    outs = {}
    try:
        for name, env in (("table", {"CC_LTAB_CAS": "1"}), ("part", {"CC_LP_MIN": "0"})):
            os.environ.update(env)
            try:
                outs[name] = consensus_pipeline(bam, str(tmp_path / name), engine=e)
            finally:
                for k in env:
                    os.environ.pop(k, None)
    finally:
        e.close()
    a, b = outs["table"], outs["part"]
    n = 0
    for k in a:
        if isinstance(a[k], str) and a[k].endswith(".bam") and os.path.isfile(a[k]):
            assert_same_records(b[k], a[k], "%s/%s" % (kind, k))
            n += 1
    assert n >= 5
