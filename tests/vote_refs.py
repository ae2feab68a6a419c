"""numpy references for the engine's votes (tests/test_gpu_vote_edges.py compares the kernels with
them; tests/test_vote_refs.py pins them to the Python oracle without a GPU): consensus_maker
(SSCS_maker.py:81-168), the two duplex_consensus variants (DCS_maker.py:99-123,
singleton_correction.py:61-86) and the create_aligned_segment modes (consensus_helper.py:509-619),
restated on arrays.  Bases are BAM nibble codes, one per element; all arithmetic is int64."""
import numpy as np

A, C, G, T, N = 1, 2, 4, 8, 15          # BAM nibble codes of the bases a vote accepts
ACGT = (A, C, G, T)
PHRED_PASS = 30                         # a member counts at a position from this quality on
QUAL_CAP = 60                           # the consensus quality's cap
FLAG_PRIORITY = (99, 83, 147, 163)      # consensus_flag's order among tied flags

# what consensus_maker raises on, in the order one (position, member) step meets them
SHORT_READ, BAD_BASE, N_HIGHQ = "short_read", "bad_base", "n_highq"


class VoteError(Exception):
    def __init__(self, kind):
        Exception.__init__(self, kind)
        self.kind = kind


def passes_cutoff(count, passed, cutoff):
    """count / passed >= cutoff in Python floats (SSCS_maker.py:154-155), evaluated once per distinct
    (count, passed) pair; False where nothing passed."""
    count = np.asarray(count, np.int64)
    passed = np.asarray(passed, np.int64)
    out = np.zeros(count.shape, bool)
    pairs, inv = np.unique(np.stack([count.ravel(), passed.ravel()], axis=1), axis=0, return_inverse=True)
    ok = np.array([bool(p) and (int(c) / int(p) >= cutoff) for c, p in pairs], bool)
    out.ravel()[:] = ok[inv.ravel()]
    return out


def sscs_vote(codes, quals, cutoff, length=None):
    """consensus_maker over one family: codes[j], quals[j] the base codes and qualities of member j
    (members may be longer than member 0); length: member 0's query length (its array's by default).
    Returns (codes, quals) of `length` positions; raises VoteError with the kind of the first
    (position, member) that raises in the reference."""
    n = len(codes)
    L = len(codes[0]) if length is None else int(length)
    lens = np.array([min(len(c), len(q)) for c, q in zip(codes, quals)], np.int64)
    b = np.zeros((n, L), np.int64)
    q = np.zeros((n, L), np.int64)
    for j in range(n):
        k = min(L, int(lens[j]))
        b[j, :k] = np.asarray(codes[j][:k], np.int64)
        q[j, :k] = np.asarray(quals[j][:k], np.int64)
    pos = np.arange(L, dtype=np.int64)[None, :]
    short = pos >= lens[:, None]
    passing = (q >= PHRED_PASS) & ~short
    known = np.isin(b, ACGT + (N,))
    err = np.zeros((n, L), np.int64)                 # 0 none, else 1 + index into the kinds
    err[passing & (b == N)] = 3
    err[~known & ~short] = 2
    err[short] = 1
    # the reference walks positions outside, members inside, and stops at the first raise
    flat = err.T.ravel()
    hit = np.flatnonzero(flat)
    if len(hit):
        raise VoteError((SHORT_READ, BAD_BASE, N_HIGHQ)[int(flat[hit[0]]) - 1])
    cnt = np.stack([(passing & (b == x)).sum(axis=0, dtype=np.int64) for x in ACGT])          # (4, L)
    qsum = np.stack([np.where(passing & (b == x), q, 0).sum(axis=0, dtype=np.int64) for x in ACGT])
    best = np.argmax(cnt, axis=0)                    # first maximum in A, C, G, T order
    top = cnt[best, np.arange(L)]
    passed = passing.sum(axis=0, dtype=np.int64)
    ok = passes_cutoff(top, passed, cutoff)
    out_c = np.where(ok, np.array(ACGT, np.int64)[best], N).astype(np.uint8)
    out_q = np.minimum(QUAL_CAP, qsum[best, np.arange(L)]).astype(np.int64)
    return out_c, out_q


def pair_vote(codes1, quals1, codes2, quals2, gate):
    """duplex_consensus(read1, read2) over read 1's length: equal bases (gate: and both qualities
    above 29) give the base at min(60, q1 + q2), everything else N at 0.  A shorter read 2 raises
    VoteError(SHORT_READ)."""
    L = len(codes1)
    if len(codes2) < L:
        raise VoteError(SHORT_READ)
    b1 = np.asarray(codes1, np.int64)
    b2 = np.asarray(codes2[:L], np.int64)
    q1 = np.asarray(quals1, np.int64)
    q2 = np.asarray(quals2[:L], np.int64)
    same = b1 == b2
    if gate:
        same &= (q1 > 29) & (q2 > 29)
    return np.where(same, b1, N).astype(np.uint8), np.where(same, np.minimum(QUAL_CAP, q1 + q2), 0).astype(np.int64)


def most_common_first(values):
    """The most common value; among equally common ones the first seen (Counter.most_common with the
    reference's randint tie break fixed at 0)."""
    count, order = {}, []
    for v in values:
        if v not in count:
            count[v] = 0
            order.append(v)
        count[v] += 1
    top = max(count.values())
    for v in order:
        if count[v] == top:
            return v


def pick_flag(flags):
    """The most common flag; among tied ones 99 > 83 > 147 > 163, else the first seen."""
    count, order = {}, []
    for v in flags:
        if v not in count:
            count[v] = 0
            order.append(v)
        count[v] += 1
    top = max(count.values())
    tied = [v for v in order if count[v] == top]
    if len(tied) > 1:
        for f in FLAG_PRIORITY:
            if f in tied:
                return f
    return tied[0]


def family_rg(rgs):
    """The family's read group: None when any member has none (get_tag raises, no RG is set)."""
    if any(r is None for r in rgs):
        return None
    return most_common_first(rgs)
