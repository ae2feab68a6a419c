"""The device BGZF encoder's effort setting (cc_bgzf_set_effort; effort 2: bucketed candidates that
see their own tile, a one-step lazy parse).  The judge is Python's zlib, as in test_gpu_bgzf.py:
every member must be a well-formed BGZF member that inflates to exactly its piece."""
import json
import os
import shutil
import zlib

import numpy as np
import pytest

import pysam  # the oracle shim
from parity import GOLDEN
from test_gpu_bgzf import BUFFERS, EOF_MEMBER, INPUT, OUTPUTS, _check_members, _fetch

pytestmark = pytest.mark.gpu

PIECE = 0xff00
TILE = 512      # positions per tile of the match finder
SEGMENT = 64    # positions per wave: effort 2's blind range
WAYS = 4        # positions per bucket at effort 2


def _random(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def _filler(n, seed):
    """16 letters at random: 4 bits of entropy a byte, so a Huffman form beats the stored one and the
    tokens under test reach the member; the planted strings use other bytes."""
    return (np.random.RandomState(seed).randint(0, 16, n) + 0x40).astype(np.uint8).tobytes()


def _planted(n, seed):
    return (np.random.RandomState(seed).randint(0, 96, n) + 0xa0).astype(np.uint8).tobytes()


HUFFMAN = ("edge", "ways", "lazy_mid", "lazy_piece_end", "runs", "runs_end259", "runs_end517")


def _pairs():
    r = np.random.RandomState(29)
    out = bytearray()
    while len(out) < PIECE:
        s = r.randint(0, 256, 150).astype(np.uint8).tobytes()
        out += s + s
    return bytes(out[:PIECE])


def _edge():
    """A 40-byte string whose first copy ends at tile offset 511 and whose second begins at 512; a
    second string the same way across a 64-position segment edge inside a tile."""
    out = bytearray(_filler(4 * TILE, 31))
    s, t = _planted(40, 32), _planted(40, 33)
    out[2 * TILE - 40:2 * TILE] = s
    out[2 * TILE:2 * TILE + 40] = s
    at = 3 * TILE + 3 * SEGMENT
    out[at - 40:at] = t
    out[at:at + 40] = t
    return bytes(out)


def _ways():
    """One 4-byte prefix before 3 * WAYS + 1 differing tails, at spacings under and over a tile, so
    the buckets evict; the last occurrence repeats the oldest tail in full."""
    prefix = b"\x01\xfe\x02\xfd"
    tails = [_planted(24, 100 + k) for k in range(3 * WAYS)]
    out = bytearray(_filler(50, 38))
    for k, t in enumerate(tails):
        out += prefix + t
        out += _filler((90, 700, 30)[k % 3], 200 + k)
    out += prefix + tails[0] + _filler(10, 39)
    return bytes(out)


def _lazy(end):
    """x + A + T where "x + A" and, apart from it, "A + T" occurred before: the match at i + 1 is
    longer than the one at i.  end: the buffer's length; the construction's last byte is its last."""
    a, t = _planted(10, 41), _planted(20, 40)
    mid = b"x" + a + b"#" + _filler(700, 42) + b"y" + a + t + _filler(900, 43) + b"x" + a + t
    # at the end of a piece: "xab" + q and "yabcd" before, then "xabcd" as the last five bytes, so
    # position n - 5 has a 3-byte match and position n - 4 (the last one hashed) a 4-byte match
    tail = b"xabq" + _filler(200, 44) + b"yabcd" + _filler(300, 45) + b"xabcd"
    body = mid + _filler(100, 46)
    fill = end - len(body) - len(tail)
    assert fill >= 0
    return body + _filler(fill, 47) + tail


def _runs(at_end):
    head = _filler(100, 51) + b"a" * 259 + _filler(50, 52) + b"b" * 517 + _filler(30, 53)
    if not at_end:
        return head
    return head + (b"c" * 259 if at_end == 1 else b"d" * 517)


NEW_BUFFERS = {
    "pairs": _pairs(),
    "edge": _edge(),
    "ways": _ways(),
    "lazy_mid": _lazy(3000),
    "lazy_piece_end": _lazy(PIECE) + _filler(500, 48),
    "runs": _runs(0),
    "runs_end259": _runs(1),
    "runs_end517": _runs(2),
}


@pytest.fixture(scope="module")
def engine():
    from consensuscruncher_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def before(engine):
    """Effort-1 members from before any effort-2 call of this module's engine."""
    return {name: engine.bgzf_deflate(BUFFERS[name]) for name in ("bam", "three")}


@pytest.mark.parametrize("name", sorted(BUFFERS))
def test_effort2_members_inflate_to_their_pieces(engine, name):
    data = BUFFERS[name]
    members = engine.bgzf_deflate(data, effort=2)
    btypes = _check_members(members, data, name)
    assert engine.bgzf_deflate(data, effort=2) == members, "a second call must return the same bytes"
    assert sum(len(m) for m in members) <= len(data) + 31 * len(members), "never larger than stored"
    if name == "random":
        assert btypes == [0]
    if name == "zeros":
        assert len(members[0]) < 600


@pytest.mark.parametrize("name", sorted(NEW_BUFFERS))
def test_new_buffers_at_both_efforts(engine, name):
    data = NEW_BUFFERS[name]
    one = engine.bgzf_deflate(data, effort=1)
    two = engine.bgzf_deflate(data, effort=2)
    types = _check_members(one, data, name + "@1") + _check_members(two, data, name + "@2")
    if name in HUFFMAN:
        assert 0 not in types, "a stored member would hide the tokens under test"
    assert engine.bgzf_deflate(data, effort=2) == two
    print(name, "effort 1:", [len(m) for m in one], "effort 2:", [len(m) for m in two])
    if name == "pairs":
        # literals alone are 0.50 of the piece, zlib's levels 1 and 6 give 0.511; the margin is the
        # dynamic header and the copies a blind segment cuts
        assert len(two[0]) <= 0.60 * len(data)
        assert len(two[0]) < len(one[0])


def test_launch_independence(engine):
    """More than one 256-piece launch: a piece's member does not depend on its neighbours."""
    piece = NEW_BUFFERS["pairs"]
    alone = engine.bgzf_deflate(piece, effort=2)[0]
    data = piece * 300 + _random(77, 61)
    members = engine.bgzf_deflate(data, effort=2)
    assert len(members) == 301
    assert all(m == alone for m in members[:300])
    _check_members(members[300:], data[300 * PIECE:], "launch tail")


def test_effort_is_per_call_and_effort1_is_unchanged(engine, before):
    for name in ("bam", "three"):
        two = engine.bgzf_deflate(BUFFERS[name], effort=2)
        assert engine.bgzf_effort == 1
        assert engine.bgzf_deflate(BUFFERS[name]) == before[name], name
        if name == "bam":
            assert two != before[name]


def test_invalid_efforts_change_nothing(engine, before):
    from consensuscruncher_amd import native as N
    for bad in (0, 3):
        assert engine.lib.cc_bgzf_set_effort(engine.h, bad) == -1   # CC_E_INVALID
        assert N.CC_E[-1] == "CC_E_INVALID"
        assert engine.bgzf_deflate(BUFFERS["bam"]) == before["bam"]
    with pytest.raises(ValueError):
        engine.bgzf_deflate(b"abc", effort=3)
    with pytest.raises(ValueError):
        engine.device_bgzf(True, effort=0)
    assert not engine.bgzf_device and engine.bgzf_effort == 1
    assert engine.lib.cc_bgzf_set_effort(engine.h, 2) == 0
    try:
        assert engine.lib.cc_bgzf_set_effort(engine.h, 3) == -1
        assert engine.bgzf_deflate(BUFFERS["bam"]) != before["bam"], "still at effort 2"
    finally:
        assert engine.lib.cc_bgzf_set_effort(engine.h, 1) == 0
    assert engine.bgzf_deflate(BUFFERS["bam"]) == before["bam"]


def test_writers_follow_the_effort(engine, tmp_path):
    from consensuscruncher_amd.engine import Bam
    src = Bam(INPUT)
    one, two = str(tmp_path / "one.bam"), str(tmp_path / "two.bam")
    engine.device_bgzf(True)
    try:
        src.write(one, level=1)
        engine.device_bgzf(True, effort=2)
        assert engine.bgzf_effort == 2
        src.write(two, level=1)
    finally:
        engine.device_bgzf(False, effort=1)
    assert engine.bgzf_effort == 1 and not engine.bgzf_device
    assert open(one, "rb").read() != open(two, "rb").read()
    assert pysam.sam_lines(one) == pysam.sam_lines(two)


def test_environment_sets_the_effort(engine, monkeypatch):
    from consensuscruncher_amd.engine import Engine
    monkeypatch.setenv("CC_BGZF_DEVICE", "1")
    monkeypatch.setenv("CC_BGZF_EFFORT", "2")
    e = Engine(0)
    try:
        assert e.bgzf_device and e.bgzf_effort == 2
        assert e.bgzf_deflate(NEW_BUFFERS["pairs"]) == engine.bgzf_deflate(NEW_BUFFERS["pairs"], effort=2)
    finally:
        e.close()
    assert engine.bgzf_effort == 1


def _pipeline(engine, tmp, **options):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    d = os.path.join(GOLDEN, "basic")
    kw = dict(json.load(open(os.path.join(d, "params.json")))["run"])
    os.makedirs(tmp)
    shutil.copy(INPUT, os.path.join(tmp, "sample.bam"))
    kw["level"] = 1
    kw.update(options)
    return consensus_pipeline(os.path.join(tmp, "sample.bam"), tmp, engine=engine, **kw)


def test_pipeline_at_effort2_writes_the_same_records(engine, tmp_path):
    dev = _pipeline(engine, str(tmp_path / "device"), bgzf="device", bgzf_effort=2)
    assert engine.bgzf_effort == 1 and not engine.bgzf_device, "the options are wired for the call only"
    host = _pipeline(engine, str(tmp_path / "host"))
    exp = os.path.join(GOLDEN, "basic", "expected")
    differ = 0
    for k in OUTPUTS:
        a, b = pysam.sam_lines(dev[k]), pysam.sam_lines(host[k])
        assert a == b, k
        assert a == pysam.sam_lines(os.path.join(exp, k + ".bam")), k
        raw = open(dev[k], "rb").read()
        assert raw[-28:] == EOF_MEMBER, k
        differ += raw != open(host[k], "rb").read()
        if a:
            for regions in ([(0, 0, 40000)], [(0, 50000, 90000), (0, 120000, 10 ** 8)]):
                assert _fetch(dev[k], regions) == _fetch(host[k], regions), (k, regions)
    assert differ, "the device encoder wrote none of the files"


def test_effort2_is_no_larger_on_bam_bytes(engine, before):
    data = BUFFERS["bam"]
    one = sum(len(m) for m in before["bam"])
    two = sum(len(m) for m in engine.bgzf_deflate(data, effort=2))
    pieces = [data[o:o + PIECE] for o in range(0, len(data), PIECE)]

    def z(level):
        total = 0
        for p in pieces:
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            total += len(c.compress(p) + c.flush()) + 26
        return total
    print("bam bytes %d: effort 1 %d, effort 2 %d, zlib level 1 %d, zlib level 6 %d" % (len(data), one, two, z(1), z(6)))
    assert two <= one
