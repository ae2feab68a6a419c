"""The vote kernels (k_vote_plan, k_sscs_vote_swar, k_big_items, k_big_swar, k_big_final,
k_duplex_vote_swar) at every edge of their launch geometry, through Engine.sscs_vote and
Engine.pair_vote on tables written by the pysam stand-in, against the numpy restatement of
consensus_maker and duplex_consensus in tests/vote_refs.py (pinned to the oracle by
tests/test_vote_refs.py).  Every consensus base, every quality up to the consensus length and the
five meta fields are compared for equality: everything is integer.

The cases are tests/vote_cases.py's: the table's longest read at each families-per-wave step and on
both sides of the LDS staging and all-slow thresholds, family sizes around the 63-member items,
partly filled waves and blocks, per-position patterns at and below the cutoff's smallest passing
count, the mode routines on both sides of their table sizes, the three defined errors on each vote
path, and pairs across tables of different longest read.

Not reachable through these two calls: members dropped as a line read twice (the member record's
valid bit clear), left to the pipeline tests, and singleton-correction pairs whose complement lies in
the singleton table (b_in_a), covered by tests/test_gpu_duplex_edges.py."""
import os
import re

import numpy as np
import pytest

import vote_cases as VC
import vote_refs as R
from consensuscruncher_amd import native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def error_codes():
    with open(os.path.join(ROOT, "include", "consensuscruncher_amd.h")) as f:
        src = f.read()
    code = lambda name: int(re.search(r"#define %s (-?\d+)" % name, src).group(1))
    return {R.SHORT_READ: code("CC_E_SHORT_READ"), R.N_HIGHQ: code("CC_E_N_HIGHQ"), R.BAD_BASE: code("CC_E_BAD_BASE")}


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def upload(engine, table, path, interner=None):
    from consensuscruncher_amd.engine import MODE_SSCS, Bam, Interner
    table.write(path)
    it = interner or Interner()
    rec = Bam(path).decode(it, MODE_SSCS, "|")
    assert rec.n == len(table) and rec.max_len == table.max_len
    return engine.upload(rec), it, rec


def vote(engine, tid, fams, cutoff):
    off = np.concatenate([[0], np.cumsum([len(f) for f in fams])]).astype(np.int64)
    return engine.sscs_vote(tid, np.concatenate(fams).astype(np.int32), off, cutoff)


def compare_families(table, it, fams, cutoff, got):
    seq, qual, meta = got
    assert len(seq) == len(qual) == len(meta) == len(fams)
    for k, fam in enumerate(fams):
        codes, quals, want, rg = VC.expect_family(table, fam, cutoff)
        L = want[0]
        where = (cutoff, k, len(fam), L)
        assert meta[k][0] == L, where
        bad = np.flatnonzero((seq[k][:L] != codes) | (qual[k][:L] != quals))
        assert len(bad) == 0, where + (bad[:8].tolist(), seq[k][bad[:8]].tolist(), codes[bad[:8]].tolist(),
                                       qual[k][bad[:8]].tolist(), quals[bad[:8]].tolist())
        assert meta[k][1:4].tolist() == want[1:], where
        assert (it.get(2, meta[k][4]) if meta[k][4] >= 0 else None) == rg, where
    return len(fams)


# (the table's longest read, the families its calls vote): 8 calls of fpw - 1, fpw, fpw + 1 and
# 4 fpw + 1 families twice over; with fpw = 1, 9 calls of 1, 2 and 5 families to reach all 20
@pytest.mark.parametrize("max_len, families", [
    (1, 2 * (63 + 64 + 65 + 257)), (16, 2 * (63 + 64 + 65 + 257)), (17, 2 * (31 + 32 + 33 + 129)),
    (144, 2 * (6 + 7 + 8 + 29)), (145, 2 * (5 + 6 + 7 + 25)), (520, 3 * (1 + 2 + 5)), (1024, 3 * (1 + 2 + 5)),
    (1025, 3 * (1 + 2 + 5))])
def test_sscs_vote_edges(engine, tmp_path, max_len, families):
    assert max_len in VC.TABLE_LENS
    table, calls = VC.sscs_matrix(max_len, seed=1000 + max_len)
    tid, it, _ = upload(engine, table, str(tmp_path / "t.bam"))
    n = 0
    for i, (cutoff, fams) in enumerate(calls):
        assert i == 0 or cutoff != calls[i - 1][0]   # the cached cutoff table never fits the next call
        n += compare_families(table, it, fams, cutoff, vote(engine, tid, fams, cutoff))
    engine.free_table(tid)
    assert n == families
    assert {c for c, _ in calls} == set(VC.CUTOFFS)
    sizes = {len(f) for _, fams in calls for f in fams}
    assert sizes >= set(VC.LONG_SIZES if max_len in VC.LONG_TABLES else VC.SIZES)
    assert {len(table.codes[f[0]]) for _, fams in calls for f in fams} == set(VC.family_lengths(max_len))


@pytest.mark.parametrize("max_len, members", [(VC.SV_POS, VC.VOTE_BIGN), (VC.SV_POS, 3 * VC.BIG_CH + 1),
                                              (VC.TABLE_LENS[3], 2 * VC.BIG_CH + 1), (VC.TABLE_LENS[4], 2 * VC.BIG_CH + 1)])
def test_sscs_vote_exact_ratios(engine, tmp_path, max_len, members):
    """count / pass equal to the cutoff exactly (7 of 10, 49 of 70, 2 of 3, 1 of 3, 1 of 2, all) and one
    count below, at every position of a family: below 64 members through thr[], above through
    k_big_final's division; each cutoff twice, never twice in a row."""
    rng = np.random.default_rng(max_len + members)
    ratios = [(7, 10), (2, 3), (1, 3), (1, 2), (1, 1), (49, 70), (42, 60), (21, 63), (40, 60)]
    ratios = [(c, p) for c, p in ratios if p <= members]
    table, fams = VC.Table(), []
    for below in (0, 1):
        b = np.zeros((members, max_len), np.uint8)
        q = np.zeros((members, max_len), np.uint8)
        for i in range(max_len):
            c, p = ratios[i % len(ratios)]
            c = max(1, c - below)
            order = rng.permutation(members)
            bases = rng.permutation(R.ACGT)
            b[:, i] = rng.choice(VC.ACGTN, members)
            q[:, i] = rng.choice(VC.FAIL_Q, members)
            b[order[:c], i] = bases[0]
            b[order[c:p], i] = np.resize(bases[1:], p - c) if p - c <= 3 * (c - 1) or c == 1 else bases[1]
            q[order[:p], i] = rng.choice(VC.PASS_Q, p)
        fams.append([table.add(b[j], q[j]) for j in range(members)])
    tid, it, _ = upload(engine, table, str(tmp_path / "t.bam"))
    n = 0
    for cutoff in VC.CUTOFFS + VC.CUTOFFS[3:] + VC.CUTOFFS[:3]:
        n += compare_families(table, it, fams, cutoff, vote(engine, tid, fams, cutoff))
    engine.free_table(tid)
    assert n == 2 * 2 * len(VC.CUTOFFS)
    # the draw is what it says: at cutoff 0.7 the 7 : 10 positions pass in the first family only
    at = [VC.expect_family(table, f, 0.7)[0][0] for f in fams]
    assert at[0] != R.N and at[1] == R.N


@pytest.mark.parametrize("matrix, families", [(VC.mode_matrix, 46), (VC.flag_tie_matrix, 116), (VC.rg_matrix, 21)])
def test_sscs_vote_modes(engine, tmp_path, matrix, families):
    table, fams = matrix(seed=5)
    tid, it, rec = upload(engine, table, str(tmp_path / "t.bam"))
    if matrix is VC.rg_matrix:       # the high read groups do take the member record's escape value
        ids = rec.rg_id[:rec.n]
        assert ids.max() >= 199 and all(ids[j] >= 126 for f in fams[1:] for j in f if table.rg[j] in ("g150", "g199"))
    n, call = 0, []
    for k, fam in enumerate(fams):   # a few thousand reads per call
        call.append(fam)
        if k + 1 == len(fams) or sum(len(f) for f in call) + len(fams[k + 1]) > 3000:
            n += compare_families(table, it, call, 0.7, vote(engine, tid, call, 0.7))
            call = []
    # and one family at a time: a family's modes must not depend on its neighbours in the wave
    for fam in fams[::7]:
        compare_families(table, it, [fam], 0.7, vote(engine, tid, [fam], 0.7))
    engine.free_table(tid)
    assert n == families
    assert any(len(f) <= VC.VOTE_BIGN for f in fams) and any(len(f) > VC.VOTE_BIGN for f in fams)


@pytest.mark.parametrize("max_len", [VC.TABLE_LENS[3], VC.TABLE_LENS[4], VC.TABLE_LENS[7]])
def test_sscs_vote_defined_errors(engine, tmp_path, max_len):
    """One offending member per call, so the engine's fixed error priority cannot hide a wrong kind:
    on the SWAR path (k_big_final's own count when every family is slow) and on the item path, the
    offender in the first, a middle and the last item and as the last member."""
    codes = error_codes()
    table, clean, cases = VC.error_matrix(max_len, seed=max_len)
    tid, it, _ = upload(engine, table, str(tmp_path / "t.bam"))
    sizes = sorted({len(f) for _, f in cases})
    assert sizes == [5, VC.VOTE_BIGN, 3 * VC.BIG_CH + 1]
    clean_fams = [clean[:s] for s in sizes]
    assert compare_families(table, it, clean_fams, 0.7, vote(engine, tid, clean_fams, 0.7)) == 3
    n = 0
    for kind, fam in cases:
        with pytest.raises(R.VoteError) as want:
            VC.expect_family(table, fam, 0.7)
        assert want.value.kind == kind
        with pytest.raises(N.CCError) as e:
            vote(engine, tid, [clean[:3], fam], 0.7)
        assert e.value.code == codes[kind], (kind, len(fam))
        n += 1
    # the engine goes on after an error
    assert compare_families(table, it, clean_fams, 0.7, vote(engine, tid, clean_fams, 0.7)) == 3
    engine.free_table(tid)
    assert n == 3 * 7


def compare_pairs(mode, ta, tb, it, a, b, got):
    seq, qual, meta = got
    assert len(seq) == len(a)
    for i, (x, y) in enumerate(zip(a, b)):
        codes, quals = R.pair_vote(ta.codes[x], ta.quals[x], tb.codes[y], tb.quals[y], bool(mode))
        L = len(codes)
        where = (mode, i, x, y, L, len(tb.codes[y]))
        assert meta[i][0] == L, where
        bad = np.flatnonzero((seq[i][:L] != codes) | (qual[i][:L] != quals))
        assert len(bad) == 0, where + (bad[:8].tolist(), seq[i][bad[:8]].tolist(), codes[bad[:8]].tolist(),
                                       qual[i][bad[:8]].tolist(), quals[bad[:8]].tolist())
        if mode == 0:    # create_aligned_segment over [read 1, read 2]
            want = [R.most_common_first([ta.mapq[x], tb.mapq[y]]), R.most_common_first([ta.tlen[x], tb.tlen[y]]),
                    R.pick_flag([ta.flag[x], tb.flag[y]])]
            rg = R.family_rg([ta.rg[x], tb.rg[y]])
        else:            # strand_correction: the singleton's own fields
            want, rg = [ta.mapq[x], ta.tlen[x], ta.flag[x]], ta.rg[x]
        assert meta[i][1:4].tolist() == want, where
        assert (it.get(2, meta[i][4]) if meta[i][4] >= 0 else None) == rg, where
    return len(a)


# per read-1 length and direction: both modes over reads 1 x reads 2 across the tables, and reads 1 x
# (reads 1 and A's longer reads) inside table A
@pytest.mark.parametrize("a_longer", [False, True])
@pytest.mark.parametrize("len1, n", [(1, 20), (15, 20), (16, 20), (17, 20), (150, 20), (1024, 6), (1025, 6), (1040, 6)])
def test_pair_vote_edges(engine, tmp_path, len1, n, a_longer):
    from consensuscruncher_amd.engine import Interner
    assert len1 in VC.PAIR_LENS
    codes = error_codes()
    ta, tb, r1, r2, long_a, short_b = VC.pair_matrix(len1, a_longer, seed=2000 + len1)
    it = Interner()
    ida, _, _ = upload(engine, ta, str(tmp_path / "a.bam"), it)
    idb, _, _ = upload(engine, tb, str(tmp_path / "b.bam"), it)
    second = r1 + long_a
    ab = [(x, y) for x in r1 for y in r2]
    aa = [(x, y) for x in r1 for y in second]
    pairs = 0
    for mode in (0, 1):
        a, b = [x for x, _ in ab], [y for _, y in ab]
        pairs += compare_pairs(mode, ta, tb, it, a, b, engine.pair_vote(mode, ida, idb, a, b))
        a, b = [x for x, _ in aa], [y for _, y in aa]
        pairs += compare_pairs(mode, ta, ta, it, a, b, engine.pair_vote(mode, ida, ida, a, b))
        for y in short_b:            # read 2 shorter than read 1
            with pytest.raises(N.CCError) as e:
                engine.pair_vote(mode, ida, idb, [r1[0], r1[1]], [r2[0], y])
            assert e.value.code == codes[R.SHORT_READ]
        for y in long_a[:1]:         # and the other way round it is read 1's length that counts
            pairs += compare_pairs(mode, tb, ta, it, [r2[0]], [y], engine.pair_vote(mode, idb, ida, [r2[0]], [y]))
    engine.free_table(ida)
    engine.free_table(idb)
    assert pairs == 2 * (n * n + n * (n + (2 if a_longer else 1)) + 1)
