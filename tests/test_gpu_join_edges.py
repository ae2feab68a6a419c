"""cc_duplex_join and cc_group (the function-level ABI on caller-given keys: k_key_insert, k_key_probe,
k_join_decide, k_join_serial, k_group_starts, k_group_fams) on the named cases of tests/join_cases.py through
Engine.duplex_join / Engine.group, against the Python oracle (cc_oracle.dcs_join / sc_join / group_keys /
pair_vote) on the byte keys themselves: chains of 1 .. 64 hops around DUPLEX_CHAIN, at entry 0 and across the
256-thread block edge, fan-in, self-partners, shared singleton and SSCS partners, the KeyErrors of both
decision kernels, key widths of 4 .. 256 bytes whose keys differ in one word or one byte, the key table's
size step, the refusals, and cc_group's family-count and scan-tile steps.  Everything compared is an integer,
for equality.

Which kernel decided: k_join_serial is launched under no profiling scope (cc_kernel_times cannot show it), so
the test reads cc_launch_count instead.  A call that goes to the serial pass enqueues exactly two device
operations more than one that does not (the error word's fill and k_join_serial); a call that raises skips
the two result copies.  Each case's count is compared with that of a call of the same mode and shapes
in which no entry has a partner (k_join_decide alone, whatever it holds), and the difference must be what
the case's path says.  The paths themselves are the census of tests/test_join_refs.py, which needs no GPU.

After a case that raises, a clean case runs on the same engine and is compared: an error leaves nothing
behind.  An engine error other than a refusal (CC_E_INVALID, CC_E_KEYERROR) ends the module."""
import numpy as np
import pytest

import cc_oracle
import join_cases as JC
from consensuscruncher_amd import native as N
from test_gpu_function_abi import random_bam, seq_str, upload

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in JC.join_cases()}
_broken = []     # an engine error that is no refusal ends the module: nothing more is started on a device that may have faulted
REFUSALS = (N.CC_E_INVALID, N.CC_E_KEYERROR)     # decided by the call's own checks, the device in order


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def call(engine, mode, keys, parts, x, vote=None):
    """(rows or the error, votes, device operations enqueued)."""
    before = engine.launch_count()
    try:
        out = engine.duplex_join(mode, keys, parts, x, vote=vote)
    except N.CCError as e:
        return e, None, engine.launch_count() - before
    rows = list(zip(out[0].tolist(), out[1].tolist()))
    return rows, (out[2] if vote is not None else None), engine.launch_count() - before


def run_case(engine, c, vote=None):
    """None, or what is wrong with the case's result."""
    try:
        want = c.expected()
    except cc_oracle.OracleError:
        want = None
    assert (want is None) == c.raises
    absent = JC.encode(np.arange(c.n) + 3 * JC.FAR if c.style != "byte" else np.full(c.n, 255), c.width, c.style)
    _, _, base_ops = call(engine, c.mode, c.keys, absent, c.x)
    got, votes, ops = call(engine, c.mode, c.keys, c.parts, c.x, vote)
    extra = ops + (2 if c.raises else 0) - base_ops
    print("JOINCASE %s n %d m %d path %s raises %s ops %d base %d" % (
        c.name, c.n, 0 if c.x is None else len(c.x), c.path, c.raises, ops, base_ops))
    if isinstance(got, N.CCError):
        if got.code not in REFUSALS:
            _broken.append("%s: %s" % (c.name, got))
        if not c.raises or got.code != N.CC_E_KEYERROR:
            return "raised %s" % got, None
    elif c.raises:
        return "did not raise", None
    elif got != want:
        bad = [i for i in range(c.n) if got[i] != want[i]]
        return "%d rows differ, first %d: %s, want %s" % (len(bad), bad[0], got[bad[0]], want[bad[0]]), None
    if vote is None and extra != (2 if c.path == "serial" else 0):
        return "%d device operations beyond k_join_decide's, path %s" % (extra, c.path), None
    return None, votes


def run_all(engine, names):
    assert not _broken, "an earlier case ended in an engine error: %s" % _broken[0]
    failed = []
    for name in names:
        c = CASES[name]
        why, _ = run_case(engine, c)
        if _broken:
            break
        if why:
            failed.append((name, why))
        if c.raises:      # the engine goes on after the error, its error word clean
            after = CASES["dcs-fanin" if c.mode == 0 else "sc-shared-3-later-after"]
            why, _ = run_case(engine, after)
            if _broken:
                break
            if why:
                failed.append((name + " then " + after.name, why))
    for name, why in failed:
        print("JOINFAIL %s: %s" % (name, why))
    assert not _broken, _broken[0]
    assert not failed, "%d of %d cases: %s" % (len(failed), len(names), failed[:12])


def names(pred):
    out = [n for n in CASES if pred(n)]
    assert out
    return out


@pytest.mark.parametrize("mode", ["dcs", "sc"])
@pytest.mark.parametrize("base", [0, 250])
def test_chains(engine, mode, base):
    """1, 2, 31, 32 hops in k_join_decide, 33 and 64 through k_join_serial; the DCS chains with an absent far
    end raise from whichever kernel decides."""
    run_all(engine, names(lambda n: n.startswith(mode + "-chain-") and n.endswith("-at250") == bool(base)))


def test_dcs_fan_in_and_self_partner(engine):
    run_all(engine, ["dcs-fanin", "dcs-fanin-300", "dcs-self", "dcs-fanin-keyerror"])


def test_sc_shared_partners_mutual_pairs_and_own_complement(engine):
    run_all(engine, names(lambda n: n.startswith(("sc-shared-", "sc-mutual", "sc-self", "sc-sscs-", "sc-no-", "sc-empty-"))))


@pytest.mark.parametrize("n", JC.JOIN_SIZES)
def test_sizes(engine, n):
    """The launch edge (255 / 256 / 257) and the table's size step (half load at 512 and 2048, the next size
    from 513), three seeds per mode; at 257 and 2048 also through k_join_serial."""
    run_all(engine, names(lambda k: ("-size-%d-" % n) in k))


@pytest.mark.parametrize("width", JC.WIDTHS)
def test_key_widths(engine, width):
    """1, 2, 3, 63 and 64 words (odd counts take key_hash's tail), keys that differ in every word, only in the
    first, only in the last, only in the final byte."""
    run_all(engine, names(lambda k: ("-width-%d-" % width) in k))


def test_empty_input(engine):
    for mode in (0, 1):
        for width in (4, 48):
            e = np.zeros((0, width), np.uint8)
            dec, part = engine.duplex_join(mode, e, e, JC.encode([5, 6], width) if mode else None)
            assert len(dec) == 0 and len(part) == 0
            dec, part = engine.duplex_join(mode, e, e, None)
            assert len(dec) == 0 and len(part) == 0
    perm, off = engine.group(np.zeros((0, 4), np.uint8))
    assert len(perm) == 0 and off.tolist() == [0]


def test_refusals_leave_the_engine_usable(engine):
    assert not _broken
    for kb in JC.BAD_KEY_BYTES:
        k = np.zeros((3, kb), np.uint8)
        for mode in (0, 1):
            with pytest.raises(N.CCError) as e:
                engine.duplex_join(mode, k, k, k if mode else None)
            assert e.value.code == N.CC_E_INVALID, (kb, str(e.value))
        with pytest.raises(N.CCError) as e:
            engine.group(k)
        assert e.value.code == N.CC_E_INVALID, (kb, str(e.value))
    for name, mode, k, p, x in JC.duplicate_cases():
        with pytest.raises(N.CCError) as e:
            engine.duplex_join(mode, k, p, x)
        assert e.value.code == N.CC_E_INVALID and "duplicate key" in str(e.value), (name, str(e.value))
        why, _ = run_case(engine, CASES["sc-mutual" if mode else "dcs-self"])
        assert not why, (name, why)
    assert not _broken, _broken[0]


@pytest.mark.parametrize("name", ["dcs-vote-serial", "sc-vote-serial"])
def test_vote_rows_after_the_serial_pass(engine, tmp_path, name):
    """The consensus rows of a case k_join_serial decides: table X's reads (151 bases, odd) longer than table
    A's (100), out_stride the engine's; a voted row is duplex_consensus of the two reads, every other row stays
    as the caller passed it (zero)."""
    assert not _broken
    c = CASES[name]
    LA, LX = 100, 151
    m = 0 if c.x is None else len(c.x)
    ra = random_bam(str(tmp_path / "a.bam"), c.n, LA, seed=81 + c.mode, n_frac=0.05)
    rx = random_bam(str(tmp_path / "x.bam"), max(m, 3), LX, seed=83, n_frac=0.05)
    ta, _ = upload(engine, str(tmp_path / "a.bam"))
    tx, _ = upload(engine, str(tmp_path / "x.bam"))
    try:
        why, votes = run_case(engine, c, vote=(ta, np.arange(c.n), tx, np.arange(m) if c.mode else None))
        assert not why and not _broken, (name, why)
        seq, qual, meta = votes
        assert qual.shape == (c.n, (LX + 15) & ~15) and seq.shape == qual.shape
        voted = 0
        kinds = set()
        for i, (d, j) in enumerate(c.expected()):
            if (c.mode == 0 and d != 0) or (c.mode == 1 and d == 2):
                assert not seq[i].any() and not qual[i].any() and not meta[i].any(), (name, i, d)
                continue
            other = rx[j] if (c.mode == 1 and d == 0) else ra[j]
            s, q = cc_oracle.pair_vote(ra[i], other, gate=bool(c.mode))
            assert seq_str(seq[i], LA) == s and list(qual[i][:LA]) == list(q), (name, i, d, j)
            assert meta[i][0] == LA, (name, i, meta[i].tolist())
            voted += 1
            kinds.add(d)
        assert voted > 20 and kinds == ({0} if c.mode == 0 else {0, 1}) and voted < c.n
    finally:
        if not _broken:
            engine.free_table(ta)
            engine.free_table(tx)


# ---- cc_group ------------------------------------------------------------------------------------------------
GROUPS = JC.group_cases()


def group_names(n):
    return [c for c in GROUPS if len(c.fam) == n]


@pytest.mark.parametrize("n", sorted({len(c.fam) for c in GROUPS}))
def test_group_matches_read_dict_at_its_edges(engine, n):
    """perm / fam_offsets rows against cc_oracle.group_keys: families in first-seen order, members in input order,
    at the launch edge, the 4,096-entry scan tile and the family counts at which the sort's bits change."""
    assert not _broken
    failed = []
    for c in group_names(n):
        try:
            perm, off = engine.group(c.keys)
        except N.CCError as e:
            if e.code not in REFUSALS:
                _broken.append("%s: %s" % (c.name, e))
                raise
            failed.append((c.name, "raised %s" % e))
            continue
        want = c.expected()
        print("GROUPCASE %s n %d families %d width %d" % (c.name, n, c.families, c.width))
        if off.tolist() != np.concatenate([[0], np.cumsum([len(f) for f in want])]).tolist():
            failed.append((c.name, "fam_offsets", len(off) - 1, len(want)))
        elif [perm[off[k]:off[k + 1]].tolist() for k in range(len(off) - 1)] != want:
            failed.append((c.name, "perm"))
    for f in failed:
        print("GROUPFAIL %s" % (f,))
    assert not failed, failed[:12]
