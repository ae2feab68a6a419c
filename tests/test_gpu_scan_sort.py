"""The engine's prefix scan (scan_launch: k_scan_reduce + k_scan_down, or the look-back k_scan_one) and
its stable LSD radix sort (sort_pairs: k_rs_hist, the scan, k_rs_scatter) against numpy, through the
test hooks cc_debug_scan / cc_debug_sort_pairs, at sizes chosen for the code's own switches: the tile
(4096), the 64-tile look-back window, the default engine's switch at 64 tiles, a last tile of one
element, a digit histogram of more than one scan tile.  Every comparison is exact integer equality.

The hook's four kinds reach every path of the store phase (the scan is an exclusive sum only, and an
emitter fed uint32 input does not compile), through one unstaged and one staged emitter: not every
instantiation the engine makes."""
import functools

import numpy as np
import pytest

from scan_sort_refs import CANARY, TILE, ref_compact, ref_scan, ref_sort, sort_window

pytestmark = pytest.mark.gpu

T = TILE
CANARY_I32 = CANARY - (1 << 32)
CANARY_U64 = (CANARY << 32) | CANARY

SCAN_SIZES = [0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T, 64 * T - 1, 64 * T, 64 * T + 1, 65 * T + 3,
              130 * T + 1,   # engine 1: the last tiles walk back over three look-back windows
              300 * T + 77]
# size-major, so that the cached inputs and references of a size serve all its cases in a row
SCAN_CASES = [(kind, engine, n) for n in SCAN_SIZES for kind in range(4)
              for engine in ((0, 1, -1) if n in (64 * T, 64 * T + 1) else (0, 1))]


@pytest.fixture(scope="module")
def eng():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def same(got, want, what):
    """Exact equality, naming the first difference and its tile."""
    got = np.asarray(got).astype(np.int64)
    want = np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if len(got) else []
    assert len(bad) == 0, "%s: %d of %d differ, first at %d (tile %d, offset %d): got %s, expected %s" % (
        what, len(bad), len(got), bad[0], bad[0] // T, bad[0] % T, got[bad[0]], want[bad[0]])


def untouched(tail, what):
    """The elements behind an output still hold the hook's fill."""
    want = {4: CANARY, 8: CANARY_U64}[tail.dtype.itemsize] if tail.dtype.kind == "u" else CANARY_I32
    bad = np.flatnonzero((tail != tail.dtype.type(want)).reshape(len(tail), -1).any(axis=1))
    assert len(bad) == 0, "%s: %d elements behind the output were written, first at +%d" % (what, len(bad), bad[0])


def flag_patterns(n, rng):
    """(name, flags) for a size: the issue's patterns, where n allows."""
    pats = [("zeros", np.zeros(n, np.uint8)), ("ones", np.ones(n, np.uint8)),
            ("p0.5", (rng.random(n) < 0.5).astype(np.uint8)), ("p0.01", (rng.random(n) < 0.01).astype(np.uint8))]
    if n >= 1:
        first = np.zeros(n, np.uint8)
        first[0] = 1
        last = np.zeros(n, np.uint8)
        last[n - 1] = 1
        pats += [("first", first), ("last", last)]
    if n > T:
        edge = np.zeros(n, np.uint8)
        edge[T - 1] = edge[T] = 1
        pats.append(("tile_edge", edge))
    return pats


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=2)
def flag_cases(n):
    """Per pattern: flags, their references and kind 3's columns, computed once per size and shared
    (read-only) by the kinds and engines."""
    rng = np.random.default_rng(7_000_003 + n)
    aux = rng.integers(-2**31, 2**31, size=(3, n), dtype=np.int64).astype(np.int32)
    out = []
    for name, flags in flag_patterns(n, rng):
        excl, total = ref_scan(flags)
        vslot, lst, vpair = ref_compact(flags, aux)
        assert total < 2**32 and total == len(lst)
        out.append((name,) + frozen(flags, excl, vslot, lst, vpair) + (total,))
    return frozen(aux)[0], out


@functools.lru_cache(maxsize=2)
def value_cases(n):
    """Kind 0: uint32 values below 2^12 under the same patterns (every total stays below 2^32)."""
    rng = np.random.default_rng(9_000_011 + n)
    out = []
    for name, flags in flag_patterns(n, rng):
        values = flags.astype(np.uint32) * rng.integers(0, 1 << 12, n, dtype=np.uint32)
        if name in ("first", "last", "tile_edge"):
            values[flags != 0] |= 1   # the single elements count
        excl, total = ref_scan(values)
        assert total < 2**32
        out.append((name,) + frozen(values, excl) + (total,))
    return out


def check_flags(eng, kind, engine, n, name, flags, excl, vslot, lst, vpair, total, aux):
    what = "kind %d engine %d n %d %s" % (kind, engine, n, name)
    a, b, tot = eng.debug_scan(kind, engine, flags, aux if kind == 3 else None)
    assert tot == total, "%s: total %d, expected %d" % (what, tot, total)
    untouched(a[n:], what + " out_a")
    if kind == 1:
        same(a[:n], excl, what + " prefix")
        return
    same(a[:n], vslot, what + " vslot")
    untouched(b[total:], what + " out_b")
    same(b[:total], lst if kind == 2 else vpair, what + (" list" if kind == 2 else " vpair"))


@pytest.mark.parametrize("kind,engine,n", SCAN_CASES, ids=["k%d-e%d-n%d" % c for c in SCAN_CASES])
def test_scan(eng, kind, engine, n):
    if kind == 0:
        for name, values, excl, total in value_cases(n):
            what = "kind 0 engine %d n %d %s" % (engine, n, name)
            a, b, tot = eng.debug_scan(0, engine, values)
            assert b is None
            assert tot == total, "%s: total %d, expected %d" % (what, tot, total)
            untouched(a[n:], what + " out_a")
            same(a[:n], excl, what + " prefix")
        return
    aux, cases = flag_cases(n)
    for name, flags, excl, vslot, lst, vpair, total in cases:
        check_flags(eng, kind, engine, n, name, flags, excl, vslot, lst, vpair, total, aux)


def test_look_back_state_reuse(eng):
    """Three look-back scans in a row on one engine: the third is longer than the second, so its tiles
    from 3 up find the per-tile states the first run left, which must read as "not published" (the
    epoch tag) and never as prefixes."""
    rng = np.random.default_rng(20_261_019)
    for n in (130 * T + 1, 3 * T, 131 * T):
        flags = (rng.random(n) < 0.5).astype(np.uint8)
        aux = rng.integers(-2**31, 2**31, size=(3, n), dtype=np.int64).astype(np.int32)
        excl, total = ref_scan(flags)
        vslot, lst, vpair = ref_compact(flags, aux)
        for kind in (1, 3):
            check_flags(eng, kind, 1, n, "reuse", flags, excl, vslot, lst, vpair, total, aux)


def test_hook_rejects_bad_arguments(eng):
    from consensuscruncher_amd import native as N
    flags = np.ones(8, np.uint8)
    for kind, engine in ((4, 0), (-1, 0), (1, 2), (1, -2)):
        with pytest.raises(N.CCError) as e:
            eng.debug_scan(kind, engine, flags, np.zeros(24, np.int32))
        assert e.value.code == -1
    with pytest.raises(N.CCError):
        eng.debug_sort_pairs(0, np.zeros(4, np.uint64), np.zeros(4, np.uint32), 9, 8)
    with pytest.raises(N.CCError):
        eng.debug_sort_pairs(0, np.zeros(4, np.uint64), np.zeros(4, np.uint32), 0, 65)
    # the engine is usable afterwards
    a, _, tot = eng.debug_scan(1, -1, flags)
    assert tot == 8 and a[:8].tolist() == list(range(8))


# ------------------------------------------------------------------ the sort
SORT_SIZES = [0, 1, 255, 256, T - 1, T, T + 1, 3 * T + 5,
              17 * T,   # 256 * 17 = 4352 digit counts: the histogram scan has two tiles
              70_000]
WINDOWS = [(0, 64), (0, 48), (0, 8), (0, 16), (0, 1), (16, 40), (56, 64), (0, 0)]
SORT_CASES = [(n, engine, w) for n in SORT_SIZES for engine in ((-1, 0, 1) if n == 17 * T else (-1,)) for w in WINDOWS]


def key_sets(n, begin_bit, end_bit, rng):
    """(name, keys, vals): the digits inside the sort's window by the set, random nonzero bits outside."""
    lo, hi = sort_window(begin_bit, end_bit)
    w = hi - lo
    wmask = ((1 << w) - 1) << lo
    outside = ~wmask & (2**64 - 1)
    i = np.arange(n, dtype=np.uint64)

    def rnd(bits):
        return rng.integers(0, 2**64, n, dtype=np.uint64) & np.uint64((1 << bits) - 1) if bits else np.zeros(n, np.uint64)

    def one():
        return int(rng.integers(0, 2**64, dtype=np.uint64)) & ((1 << w) - 1)

    def keys_of(digits):
        out = rng.integers(0, 2**64, n, dtype=np.uint64) & np.uint64(outside)
        if outside:
            out[out == 0] = np.uint64(outside & -outside)   # nonzero outside the window
        return out | (np.asarray(digits, np.uint64) << np.uint64(lo)) if w else out

    vals = rng.integers(0, 2**32, n, dtype=np.uint32)
    sets = [("uniform", keys_of(rnd(w)), vals),
            ("equal", keys_of(np.full(n, one(), np.uint64)), np.arange(n, dtype=np.uint32))]
    a, b = one(), one()
    sets.append(("two_digits", keys_of(np.where(rng.random(n) < 0.5, np.uint64(a), np.uint64(b))), vals))
    if w and (1 << w) >= max(n, 1):
        desc = (np.uint64(max(n - 1, 0)) - i) * np.uint64(((1 << w) - 1) // max(n - 1, 1))   # strictly descending
    else:
        desc = ((np.uint64(max(n - 1, 0)) - i) << np.uint64(w)) // np.uint64(max(n, 1))  # as steep as the window allows
    sets.append(("descending", keys_of(desc), vals))
    lone = np.full(n, one(), np.uint64)
    if n:
        lone[int(rng.integers(0, n))] ^= np.uint64(((1 << w) - 1) & 0x5555555555555555)
    sets.append(("one_bin_but_one", keys_of(lone), vals))
    return sets


def check_sort(eng, engine, n, window, name, keys, vals):
    what = "sort n %d window %s engine %d %s" % (n, window, engine, name)
    k, v = eng.debug_sort_pairs(engine, keys, vals, *window)
    rk, rv = ref_sort(keys, vals, *window)
    untouched(k[n:], what + " keys")
    untouched(v[n:], what + " values")
    assert np.array_equal(k[:n], rk), "%s: keys differ, first at %d" % (what, np.flatnonzero(k[:n] != rk)[0])
    assert np.array_equal(v[:n], rv), "%s: values differ, first at %d" % (what, np.flatnonzero(v[:n] != rv)[0])
    if name == "equal":
        assert np.array_equal(v[:n], np.arange(n, dtype=np.uint32)), what + ": equal digits left their input order"


@pytest.mark.parametrize("n,engine,window", SORT_CASES,
                         ids=["n%d-e%d-b%d_%d" % (n, e, w[0], w[1]) for n, e, w in SORT_CASES])
def test_sort(eng, n, engine, window):
    rng = np.random.default_rng(11_000_027 + 131 * n + 7 * window[0] + window[1])
    sets = key_sets(n, window[0], window[1], rng)
    assert [s[0] for s in sets] == ["uniform", "equal", "two_digits", "descending", "one_bin_but_one"]
    for name, keys, vals in sets:
        check_sort(eng, engine, n, window, name, keys, vals)


def test_sort_buffer_growth():
    """1000 pairs, then 17 tiles, then 1000 again on a fresh engine: the sort buffer is made, grown
    (freed and allocated anew) and reused at a smaller size."""
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    try:
        rng = np.random.default_rng(424_243)
        for n in (1000, 17 * T, 1000):
            keys = rng.integers(0, 2**64, n, dtype=np.uint64)
            vals = rng.integers(0, 2**32, n, dtype=np.uint32)
            for window in ((0, 64), (0, 16)):
                check_sort(e, -1, n, window, "growth", keys, vals)
    finally:
        e.close()
