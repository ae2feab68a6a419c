"""tests/vote_refs.py pinned to the Python oracle (cc_oracle.single_strand_vote, pair_vote,
most_common_first, pick_flag; the oracle itself is pinned to the reference by tests/golden) on a
reduced draw of the generators of tests/test_gpu_vote_edges.py, and the kernel constants those
generators mirror checked against csrc/cc_engine.hip.  No GPU: a wrong reference must not be able to
agree with a wrong kernel by construction."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import cc_oracle
import vote_cases as VC
import vote_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_KIND = {"IndexError: read shorter": R.SHORT_READ, "ValueError: base": R.BAD_BASE,
               "IndexError: N with quality": R.N_HIGHQ, "IndexError: complement shorter": R.SHORT_READ}


def oracle_kind(exc):
    for head, kind in ORACLE_KIND.items():
        if str(exc).startswith(head):
            return kind
    raise AssertionError("unexpected oracle error %s" % exc)


def codes_of(s):
    return np.array([VC.NT16.index(c) for c in s], np.uint8)


def test_kernel_constants_are_mirrored():
    with open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")) as f:
        src = f.read()
    for name in ("VOTE_BIGN", "BIG_CH", "BIG_STAGE", "SV_POS", "MODE_K", "MODE_SLOTS"):
        m = re.findall(r"constexpr int %s = (\d+);" % name, src)
        assert len(m) == 1, name
        assert int(m[0]) == getattr(VC, name), name
    # the edges the GPU matrix is laid on, as the issue that asked for it lists them
    assert VC.TABLE_LENS == (1, 16, 17, 144, 145, 520, 1024, 1025)
    assert [VC.fams_per_wave(m) for m in VC.TABLE_LENS] == [64, 64, 32, 7, 6, 1, 1, 1]
    assert VC.SIZES == (1, 2, 3, 62, 63, 64, 65, 126, 127, 189, 190, 300)
    assert VC.LONG_SIZES == (1, 2, 63, 64, 127)
    assert VC.PAIR_LENS == (1, 15, 16, 17, 150, 1024, 1025, 1040)
    assert VC.DISTINCT == (1, 4, 5, 256, 257)
    assert VC.family_lengths(145) == [145, 91, 144, 1] and VC.family_lengths(1) == [1]
    assert VC.family_lengths(16) == [16, 11, 15, 1]


def test_worked_example():
    """SSCS_maker.py:27-35: cutoff 0.7 over the four reads gives ACTGATACNT."""
    reads = ["ACTGATACTT", "ACTGAAACCT", "ACTGATACCT", "ACTGATACTT"]
    codes, quals = R.sscs_vote([codes_of(s) for s in reads], [np.full(10, 40)] * 4, 0.7)
    assert "".join(VC.NT16[c] for c in codes) == "ACTGATACNT"
    assert quals.tolist() == [60] * 10
    # position 8 is a 2 : 2 tie: C (the first maximum) at any cutoff up to one half
    codes, _ = R.sscs_vote([codes_of(s) for s in reads], [np.full(10, 40)] * 4, 0.5)
    assert "".join(VC.NT16[c] for c in codes) == "ACTGATACCT"


def test_cutoff_is_python_division():
    assert R.passes_cutoff([7, 49, 6, 2, 1, 0], [10, 70, 10, 3, 3, 0], 0.7).tolist() == [True, True, False, False, False, False]
    assert not R.passes_cutoff([7, 49], [10, 70], VC.CUTOFFS[1]).any()
    assert R.passes_cutoff([2, 1, 1], [3, 3, 2], 2.0 / 3.0).tolist() == [True, False, False]
    assert R.passes_cutoff([1, 21], [3, 63], 1.0 / 3.0).all()
    assert R.passes_cutoff([5], [5], 1.0).all() and not R.passes_cutoff([5], [5], VC.CUTOFFS[6]).any()
    assert R.passes_cutoff([1], [9], 0.0).all() and not R.passes_cutoff([0], [0], 0.0).any()
    assert [VC.min_count(10, c) for c in VC.CUTOFFS] == [7, 8, 5, 7, 4, 10, 11, 0]


def check_family(table, fam, cutoff):
    members = [table.segment(j) for j in fam]
    try:
        want = cc_oracle.single_strand_vote(members, cutoff)
    except cc_oracle.OracleError as e:
        with pytest.raises(R.VoteError) as got:
            VC.expect_family(table, fam, cutoff)
        assert got.value.kind == oracle_kind(e)
        return
    codes, quals, meta, rg = VC.expect_family(table, fam, cutoff)
    assert "".join(VC.NT16[c] for c in codes) == want[0]
    assert quals.tolist() == list(want[1])
    assert meta == [members[0].infer_query_length(), cc_oracle.most_common_first([m.mapping_quality for m in members]),
                    cc_oracle.most_common_first([m.template_length for m in members]), cc_oracle.pick_flag(members)]
    made = cc_oracle.new_record(members, want[0], want[1], "x")
    assert rg == (made.get_tag("RG") if made.has_tag("RG") else None)


@pytest.mark.parametrize("max_len, sizes, families", [(17, (1, 2, 3, 63, 64, 127), 225), (145, (3, 64, 127), 43)])
def test_sscs_vote_matches_oracle(max_len, sizes, families):
    table, calls = VC.sscs_matrix(max_len, seed=100 + max_len, sizes=sizes, rounds=1, min_calls=4)
    n = 0
    for cutoff, fams in calls:
        for fam in fams:
            check_family(table, fam, cutoff)
            n += 1
    assert n == families
    # the draw holds what it is for: lengths past member 0's, every pattern's outcome, both qualities' ends
    assert any(len(table.codes[j]) > len(table.codes[f[0]]) for _, fams in calls for f in fams for j in f)
    out = [VC.expect_family(table, f, c) for c, fams in calls[:4] for f in fams]
    quals = np.concatenate([o[1] for o in out])
    codes = np.concatenate([o[0] for o in out])
    assert set(np.unique(quals).tolist()) >= {0, 30, 31, 59, 60} and (codes == R.N).any() and (codes != R.N).any()


def test_sscs_errors_match_oracle():
    table, clean, cases = VC.error_matrix(40, seed=7)
    check_family(table, clean, 0.7)
    kinds = []
    for kind, fam in cases:
        with pytest.raises(R.VoteError) as e:
            VC.expect_family(table, fam, 0.7)
        assert e.value.kind == kind
        check_family(table, fam, 0.7)
        kinds.append(kind)
    assert len(kinds) == 21 and set(kinds) == {R.SHORT_READ, R.N_HIGHQ, R.BAD_BASE}


def test_first_raise_wins():
    """Positions outside, members inside: the kind is that of the first step that raises."""
    a = codes_of("ACGT")
    q = np.full(4, 40)
    short, n_hi, bad = codes_of("AC"), codes_of("ANGT"), codes_of("ACGM")
    for fam, kind in (([a, short, n_hi], R.N_HIGHQ), ([a, short, bad], R.SHORT_READ), ([a, bad, n_hi], R.N_HIGHQ),
                      ([a, codes_of("ACMT"), short], R.BAD_BASE), ([a, short, codes_of("ACMT")], R.SHORT_READ),
                      ([a, codes_of("ACNT"), short], R.N_HIGHQ)):
        with pytest.raises(R.VoteError) as e:
            R.sscs_vote(fam, [q[:len(c)] for c in fam], 0.7)
        assert e.value.kind == kind
    # below Q30 an N only fails; a base outside ACGTN raises at any quality; neither matters past member 0's length
    codes, quals = R.sscs_vote([a, n_hi], [q, np.array([40, 29, 40, 40])], 0.7)
    assert codes.tolist() == [1, 2, 4, 8] and quals.tolist() == [60, 40, 60, 60]
    with pytest.raises(R.VoteError):
        R.sscs_vote([a, bad], [q, np.array([40, 40, 40, 2])], 0.7)
    codes, _ = R.sscs_vote([a[:3], bad, n_hi[:3] + 0, codes_of("ACGN")], [q[:3], q, np.array([40, 2, 40]), q], 0.7)
    assert codes.tolist() == [1, 2, 4]


@pytest.mark.parametrize("len1, a_longer, pairs", [(17, False, 2 * (20 * 20 + 20 * 21)), (150, True, 2 * (20 * 20 + 20 * 22))])
def test_pair_vote_matches_oracle(len1, a_longer, pairs):
    a, b, r1, r2, long_a, short_b = VC.pair_matrix(len1, a_longer, seed=len1)
    sa = [a.segment(i) for i in range(len(a))]
    sb = [b.segment(i) for i in range(len(b))]
    n = 0
    sums, both = set(), set()
    for gate in (False, True):
        for t2, s2, second in ((b, sb, r2), (a, sa, r1 + long_a)):
            for i in r1:
                for j in second:
                    want = cc_oracle.pair_vote(sa[i], s2[j], gate=gate)
                    codes, quals = R.pair_vote(a.codes[i], a.quals[i], t2.codes[j], t2.quals[j], gate)
                    assert "".join(VC.NT16[c] for c in codes) == want[0] and quals.tolist() == list(want[1])
                    same = a.codes[i] == t2.codes[j][:len1]
                    sums |= set((a.quals[i].astype(int) + t2.quals[j][:len1])[same].tolist())
                    both |= set(zip(a.codes[i][same].tolist(), a.quals[i][same].tolist(), t2.quals[j][:len1][same].tolist()))
                    n += 1
        for j in short_b:
            with pytest.raises(cc_oracle.OracleError) as e:
                cc_oracle.pair_vote(sa[r1[0]], sb[j], gate=gate)
            assert oracle_kind(e.value) == R.SHORT_READ
            with pytest.raises(R.VoteError):
                R.pair_vote(a.codes[r1[0]], a.quals[r1[0]], b.codes[j], b.quals[j], gate)
    assert n == pairs
    # the draw crosses 60 and 255, has 29 / 30 on either side of equal bases, and N equal to N
    assert min(sums) < 60 < max(sums) and max(sums) > 255 and {59, 60, 61} <= sums
    assert any(x == R.N for x, _, _ in both)
    assert any(q1 == 29 and q2 >= 30 for _, q1, q2 in both) and any(q1 >= 30 and q2 == 29 for _, q1, q2 in both)
    assert any(q1 == 30 and q2 == 30 for _, q1, q2 in both)


def test_modes_match_oracle():
    n = 0
    for table, fams in (VC.mode_matrix(1), VC.flag_tie_matrix(2), VC.rg_matrix(3)):
        for fam in fams:
            assert R.most_common_first([table.mapq[j] for j in fam]) == cc_oracle.most_common_first([table.mapq[j] for j in fam])
            assert R.most_common_first([table.tlen[j] for j in fam]) == cc_oracle.most_common_first([table.tlen[j] for j in fam])
            flags = [table.flag[j] for j in fam]
            assert R.pick_flag(flags) == cc_oracle.pick_flag([SimpleNamespace(flag=f) for f in flags])
            rgs = [table.rg[j] for j in fam]
            assert R.family_rg(rgs) == (None if None in rgs else cc_oracle.most_common_first(rgs))
            n += 1
    assert n == 46 + 116 + 21
    # every first-seen order of the four proper-pair flags gives 99; without 99, 83; and so on
    assert R.pick_flag([163, 147, 83, 99]) == 99 and R.pick_flag([163, 147, 83]) == 83 and R.pick_flag([163, 147]) == 147
    assert R.pick_flag([1024, 163, 163, 1024]) == 163 and R.pick_flag([97, 145]) == 97 and R.pick_flag([97, 99, 97]) == 97
    assert R.most_common_first([5, 7, 7, 5, 9]) == 5 and R.family_rg(["a", None, "a"]) is None
