"""tests/join_refs.py (cc_duplex_join's k_join_decide / k_join_serial restated) pinned to the Python oracle
(cc_oracle.dcs_join / sc_join) on every named case of tests/join_cases.py and on every partner assignment
of small graphs, the constants it mirrors checked against csrc/cc_engine.hip, and the census of which kernel
decides each named case: the GPU test (tests/test_gpu_join_edges.py) relies on it to know that a case
reaches k_join_serial.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

import cc_oracle
import join_cases as JC
import join_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return JC.join_cases()


def test_kernel_constants_are_mirrored():
    with open(os.path.join(ROOT, "consensuscruncher_amd", "csrc", "cc_engine.hip")) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, pattern
        return m[0]

    assert int(one(r"constexpr int DUPLEX_CHAIN = (\d+);")) == R.DUPLEX_CHAIN == JC.DUPLEX_CHAIN
    assert int(one(r"constexpr int KEY_MAX_WORDS = (\d+);")) == R.KEY_MAX_WORDS
    assert int(one(r"uint64_t size = (\d+);\n    while \(size < \(uint64_t\)\(2 \* n\)\) size <<= 1;")) == R.TABLE_FLOOR
    one(r"if \(key_bytes <= 0 \|\| \(key_bytes & 3\) \|\| key_bytes > 4 \* KEY_MAX_WORDS\) \{")
    # both chain walks of k_join_decide hand over at the same count (the product path's kernels hold the rest)
    assert len(re.findall(r"if \(nc == DUPLEX_CHAIN\) \{ atomicOr\(seq, 1u\); break; \}", src)) == 2
    one(r"if \(p\[i\] >= 0 && indeg\[p\[i\]\] > 1\) atomicOr\(seq, 1u\);")
    # the edges as the issue that asked for them lists them
    assert JC.HOPS == (1, 2, 31, 32, 33, 64) and JC.WIDTHS == (4, 8, 12, 252, 256) and JC.BAD_KEY_BYTES == (0, 6, 260)
    assert JC.JOIN_SIZES == (1, 255, 256, 257, 512, 513, 2048)
    assert JC.GROUP_SIZES == (255, 256, 257, 4095, 4096, 4097) and JC.GROUP_FAMILIES == (1, 2, 255, 256, 257, 1024, 1025)
    assert [R.table_size(n) for n in (1, 512, 513, 2048, 2049)] == [1024, 1024, 2048, 4096, 8192]
    assert [R.key_args_ok(b) for b in (0, 4, 6, 12, 252, 256, 260)] == [False, True, False, True, True, True, False]


def test_refs_by_hand():
    k = [b"a", b"b", b"c", b"d"]
    p, xs, xfirst, indeg, dup = R.resolve(k, [b"c", b"c", b"x", b"y"], [b"y", b"x"])
    assert (p, xs, xfirst, indeg, dup) == ([2, 2, -1, -1], [-1, -1, 1, 0], [3, 2], [0, 0, 2, 0], False)
    assert R.resolve([b"a", b"b", b"a"], [b"a", b"q", b"q"])[0] == [0, -1, -1] and R.resolve([b"a", b"a"], [b"b"] * 2)[4]
    assert R.resolve([b"a"], [b"b"], [b"c", b"c"])[4]
    # DCS: a pair, the later one skipped; SC: a mutual pair
    assert R.join(0, [b"a", b"b"], [b"b", b"a"]) == R.Result("parallel", False, [(0, 1), (2, -1)])
    assert R.join(1, [b"a", b"b"], [b"b", b"a"], [b"z"]) == R.Result("parallel", False, [(1, 1), (1, 0)])
    assert R.join(1, [b"a"], [b"a"]) == R.Result("serial", True, None)
    assert R.join(0, [b"a", b"b"], [b"z", b"a"]) == R.Result("parallel", True, None)
    assert R.join(0, [b"a", b"a"], [b"z", b"y"]).path == "invalid"


def oracle_rows(mode, keys, parts, x):
    try:
        return cc_oracle.dcs_join(keys, parts) if mode == 0 else cc_oracle.sc_join(keys, parts, x)
    except cc_oracle.OracleError as e:
        assert str(e).startswith("KeyError")
        return None


def test_named_cases_match_oracle_and_take_their_paths(cases):
    assert len({c.name for c in cases}) == len(cases)
    census = {}
    for c in cases:
        k, p, x = c.tags()
        assert len(set(k)) == len(k) and len(set(x)) == len(x), c.name     # the encodings are injective
        assert c.n <= 4096 and len(x) <= 4096, c.name
        want = oracle_rows(c.mode, k, p, x)
        res = R.join(c.mode, k, p, x)
        assert (want is None) == c.raises == res.error, c.name             # the oracle's verdict, as named
        assert res.rows == want, c.name
        assert res.path == c.path, (c.name, res.path)                      # the path, as named
        census.setdefault((c.mode, R.verdict(res), res.path), []).append(c.name)
        # each chain walk alone, too: the serial pass decides any case
        pp, xs, xfirst, indeg, dup = R.resolve(k, p, x if c.mode == 1 else ())
        rows, err = R.serial(c.mode, pp, xs, len(x))
        assert not dup and err == c.raises and (err or rows == want), c.name
    # both kernels decide clean cases in both modes; both raise the DCS KeyError; the SC KeyError is the serial one's
    assert set(census) == {(0, "parallel", "parallel"), (0, "serial", "serial"), (0, "error", "parallel"),
                           (0, "error", "serial"), (1, "parallel", "parallel"), (1, "serial", "serial"),
                           (1, "error", "serial")}, sorted(census)


def test_census_of_the_named_edges(cases):
    by = {c.name: c for c in cases}
    for base in ("", "-at250"):
        for h in JC.HOPS:
            path = "serial" if h > 32 else "parallel"
            for far in ("absent", "later", "cycle"):
                c = by["dcs-chain-%d-%s%s" % (h, far, base)]
                assert (c.path, c.raises) == (path, far == "absent"), c.name
            for far in ("sscs", "absent", "later"):
                c = by["sc-chain-%d-%s%s" % (h, far, base)]
                assert (c.path, c.raises) == (path, False), c.name
            if base:   # the chain crosses the block edge
                assert 250 + h >= 256 or h < 6
    # the chain's head, by the parity of its hops (DCS: the far end joined, so odd hops are skipped)
    for h in JC.HOPS:
        assert by["dcs-chain-%d-later" % h].expected()[h] == ((2, -1) if h % 2 else (0, h - 1))
        assert by["sc-chain-%d-sscs" % h].expected()[h] == (2, -1)
        assert by["sc-chain-%d-later" % h].expected()[h] == ((1, h - 1) if h <= 1 else (2, -1))
    serial = {c.name for c in cases if c.path == "serial"}
    assert {n for n in by if n.startswith("sc-shared-") and n != "sc-shared-sscs"} <= serial
    assert {"sc-self", "sc-self-late", "sc-self-300", "dcs-vote-serial", "sc-vote-serial", "dcs-size-2048-serial",
            "sc-size-2048-serial", "dcs-size-257-serial", "sc-size-257-serial"} <= serial
    assert not {"dcs-fanin", "dcs-fanin-300", "dcs-fanin-keyerror", "dcs-self", "sc-mutual", "sc-shared-sscs",
                "sc-sscs-equals-single", "sc-self-with-sscs", "sc-no-sscs", "sc-empty-sscs"} & serial
    assert {c.name for c in cases if c.raises and c.mode == 1} == {"sc-self", "sc-self-late", "sc-self-300"}
    assert by["dcs-fanin-keyerror"].raises and not by["dcs-fanin"].raises
    # fan-in counts and the shared-partner orders
    for name, deg in (("sc-shared-2-later", 2), ("sc-shared-3-later", 3), ("sc-shared-2-earlier", 2),
                      ("sc-shared-3-earlier", 3), ("sc-shared-3-later-after", 3)):
        k, p, x = by[name].tags()
        assert max(R.resolve(k, p, x)[3]) == deg, name
    assert by["sc-shared-3-later-after"].expected() == [(1, 2), (1, 2), (1, 0), (2, -1)]   # the late sharer: deleted
    assert by["sc-shared-2-earlier"].expected()[:3] == [(1, 4), (1, 0), (2, -1)]
    assert by["sc-shared-sscs"].expected() == [(0, 1), (2, -1), (2, -1), (0, 0)]
    assert by["sc-shared-sscs-single"].expected()[:3] == [(0, 0), (1, 5), (1, 5)]
    assert by["sc-mutual"].expected()[:4] == [(1, 3), (1, 2), (1, 1), (1, 0)]
    assert by["sc-sscs-equals-single"].expected()[0] == (0, 1) and by["sc-self-with-sscs"].expected()[1] == (0, 0)
    assert by["dcs-self"].expected() == [(1, -1), (0, 1), (2, -1), (1, -1), (0, 4), (2, -1)]
    assert by["sc-no-sscs"].x is None and len(by["sc-empty-sscs"].x) == 0
    # sizes and widths: every decision present in every mixed set that has room for them
    for c in cases:
        if "-size-" in c.name or "-width-" in c.name or c.votes:
            assert c.n in JC.JOIN_SIZES or c.n in (80, 120)
            if c.n >= 80:
                assert {d for d, _ in c.expected()} == {0, 1, 2}, c.name
    assert {(c.width, c.style, c.mode) for c in cases if "-width-" in c.name} == {
        (w, s, m) for w in JC.WIDTHS for s in JC.STYLES for m in (0, 1)}
    assert {(c.n, c.mode) for c in cases if "-size-" in c.name} == {(n, m) for n in JC.JOIN_SIZES for m in (0, 1)}
    # the key families differ where they say, and only there
    for width in JC.WIDTHS:
        a = JC.encode(np.arange(200), width, "last").view("<u4")
        assert (a[:, :-1] == a[0, :-1]).all() and len(set(a[:, -1].tolist())) == 200
        a = JC.encode(np.arange(200), width, "first").view("<u4")
        assert (a[:, 1:] == a[0, 1:]).all() and len(set(a[:, 0].tolist())) == 200
        a = JC.encode(np.arange(200), width, "byte")
        assert (a[:, :-1] == a[0, :-1]).all() and len(set(a[:, -1].tolist())) == 200
    # the refusals
    for name, mode, k, p, x in JC.duplicate_cases():
        res = R.join(mode, JC.rows_as_bytes(k), JC.rows_as_bytes(p), [] if x is None else JC.rows_as_bytes(x))
        assert res.path == "invalid", name
    far = JC.duplicate_cases()[3][2]
    assert far[0].tobytes() == far[599].tobytes() and len(far) == 600


@pytest.mark.parametrize("mode", [0, 1])
def test_every_small_graph_matches_oracle(mode):
    """Every partner assignment of n <= 5 entries (partner: any entry, itself included, or none), SC with every
    set of at most two SSCS keys among the entries' partner keys, an absent one and entry 0's own key; 6,000 seeded
    graphs of 6 .. 8 entries; chains of 31 .. 40 hops with a random tail.  With the chain limit at 2 the same
    graphs send their 3-hop chains through the serial pass."""
    paths = set()

    def check(n, pid, xid):
        keys = [b"k%d" % i for i in range(n)]
        parts = [b"k%d" % j for j in pid]
        x = [b"k%d" % j for j in xid]
        want = oracle_rows(mode, keys, parts, x)
        for limit in (R.DUPLEX_CHAIN, 2):
            res = R.join(mode, keys, parts, x, chain=limit)
            assert res.rows == want and res.error == (want is None), (n, pid, xid, limit)
            paths.add((R.verdict(res), res.path))

    for n in range(1, 6):
        xsets = [()]
        if mode == 1:
            ids = list(range(n + 1))
            xsets = [()] + [(a,) for a in ids] + list(itertools.permutations(ids, 2))
            if n >= 4:
                xsets = xsets[:1 + len(ids)] + xsets[1 + len(ids)::7]
        for pid in itertools.product(range(n + 1), repeat=n):     # n: no entry's key
            for xid in xsets:
                check(n, pid, xid)
    rng = np.random.default_rng(2024 + mode)
    for _ in range(6000):
        n = int(rng.integers(6, 9))
        pid = [int(v) for v in rng.integers(0, n + 2, n)]
        xid = [int(v) for v in rng.permutation(n + 3)[:int(rng.integers(0, 4))]] if mode == 1 else []
        check(n, pid, xid)
    for _ in range(300):
        h = int(rng.integers(31, 41))
        pid = [int(rng.integers(0, h + 4))] + list(range(h)) + [int(v) for v in rng.integers(0, h + 4, 2)]
        xid = [int(v) for v in rng.permutation(h + 5)[:int(rng.integers(0, 3))]] if mode == 1 else []
        check(len(pid), pid, xid)
    want = {("parallel", "parallel"), ("serial", "serial"), ("error", "serial")}
    assert paths == (want | {("error", "parallel")} if mode == 0 else want), paths


def test_group_cases_cover_their_edges():
    cases = JC.group_cases()
    assert len({c.name for c in cases}) == len(cases)
    seen = set()
    for c in cases:
        n = len(c.fam)
        assert n <= 4097 and c.keys.shape == (n, c.width)
        seen.add((n, c.families))
        want = c.expected()
        assert len(want) == c.families and sorted(i for f in want for i in f) == list(range(n))
        if "interleaved" in c.name and c.families > 1:
            assert all(b - a == c.families for f in want for a, b in zip(f, f[1:])), c.name     # members far apart
            first = [c.fam[f[0]] for f in want]
            assert first != sorted(first) or c.families < 3, c.name    # first-seen order is not key order
    assert {(n, F) for n in JC.GROUP_SIZES for F in JC.GROUP_FAMILIES if F <= n} <= seen
    assert {(n, n) for n in JC.GROUP_SIZES} | {(1, 1)} <= seen
    assert {c.width for c in cases} >= {4, 48, 256}
