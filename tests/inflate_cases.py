"""Raw DEFLATE streams for the inflater's tests (tests/test_inflate_core_host.py on the host,
tests/test_gpu_inflate.py on the device): buffers, zlib's compression variants, and hand-made
corrupt streams.  Python's zlib is the judge of every one."""
import os
import struct
import zlib

import numpy as np

from parity import GOLDEN

PIECE = 0xff00
INPUT = os.path.join(GOLDEN, "basic", "input.bam")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _rng(seed):
    return np.random.RandomState(seed)


def random_bytes(n, seed):
    return _rng(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def text(n, seed):
    words = [b"ACGT", b"chr1", b"\t", b"NNNN", b"IIIIHHGG", b"read", b":", b"0", b"147", b"\n", b"GATTACA", b"="]
    r = _rng(seed)
    out = bytearray()
    while len(out) < n:
        out += words[r.randint(len(words))]
        if r.randint(5) == 0:
            out.append(33 + r.randint(60))
    return bytes(out[:n])


def members_of(raw):
    """(payload, crc, isize) of every BGZF member of raw."""
    off, out = 0, []
    while off < len(raw):
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, off + bsize - 8)
        out.append((raw[off + 12 + xlen:off + bsize - 8], crc, isize))
        off += bsize
    assert off == len(raw)
    return out


def bam_stream():
    return b"".join(zlib.decompress(p, -15) for p, _, _ in members_of(open(INPUT, "rb").read()))


def ladder():
    """Every match length 3..258 once."""
    seed = random_bytes(300, 11)
    out = bytearray(seed)
    for ln in range(3, 259):
        out += seed[:ln] + bytes([seed[ln] ^ 0x55])
    return bytes(out)


def window_repeat():
    """A repeat at distance 32768 exactly in the data (zlib's deflate cannot reach that far: the matches at
    that distance are far_match_streams')."""
    r = random_bytes(32768, 13)
    return r + r[:20000]


def buffers():
    return {
        "text": text(50000, 3),
        "text257": text(257, 5),
        "zeros": bytes(PIECE),
        "random": random_bytes(PIECE, 7),
        "ladder": ladder(),
        "window": window_repeat(),
        "bam": bam_stream(),
    }


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return z.compress(data) + z.flush()
    return z.compress(data[:flush_at]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(data[flush_at:]) + z.flush()


VARIANTS = {
    "level0": dict(level=0),
    "level1": dict(level=1),
    "level6": dict(level=6),
    "level9": dict(level=9),
    "fixed": dict(strategy=zlib.Z_FIXED),
    "huffman": dict(strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(strategy=zlib.Z_RLE),
    "flush": dict(flush_at=-1),   # Z_FULL_FLUSH in the middle: several blocks and an empty stored one
}


def pieces(data):
    return [data[o:o + PIECE] for o in range(0, len(data), PIECE)] or [b""]


def valid_streams():
    """(name, raw deflate stream, its bytes): every buffer cut into pieces of at most 0xff00 bytes,
    every piece under every variant, and the empty final block of the BGZF EOF member."""
    out = []
    for bname, data in sorted(buffers().items()):
        for vname, kw in sorted(VARIANTS.items()):
            for j, p in enumerate(pieces(data)):
                kw2 = dict(kw)
                if "flush_at" in kw2:
                    kw2["flush_at"] = len(p) // 2
                out.append(("%s/%s/%d" % (bname, vname, j), raw_deflate(p, **kw2), p))
    out.append(("eof", EOF_MEMBER[18:-8], b""))
    out += far_match_streams()
    return out


def judge(stream, ulen):
    """What zlib makes of stream: the bytes when it is a complete stream of exactly ulen bytes, else None."""
    z = zlib.decompressobj(-15)
    try:
        got = z.decompress(stream, ulen + 1)
    except zlib.error:
        return None
    if not z.eof or len(got) != ulen or z.unconsumed_tail:
        return None
    return got


class BitWriter(object):
    """LSB-first bit packing; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.acc = 0
        self.n = 0

    def put(self, v, nb):
        self.acc |= (v & ((1 << nb) - 1)) << self.n
        self.n += nb
        return self

    def code(self, c, nb):
        for k in range(nb - 1, -1, -1):
            self.put((c >> k) & 1, 1)
        return self

    def fixed(self, sym):
        if sym < 144:
            return self.code(0x30 + sym, 8)
        if sym < 256:
            return self.code(0x190 + sym - 144, 9)
        if sym < 280:
            return self.code(sym - 256, 7)
        return self.code(0xc0 + sym - 280, 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _stored(data, final=False):
    assert len(data) <= 0xffff
    return bytes([1 if final else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data


def _fixed_match(w, length, dist):
    """One length/distance pair in fixed-Huffman coding."""
    if length == 258:
        w.fixed(285)
    elif length < 11:
        w.fixed(254 + length)
    else:
        e = (length - 3).bit_length() - 3
        w.fixed(261 + 4 * e + (((length - 3) >> e) & 3)).put((length - 3) & ((1 << e) - 1), e)
    d = dist - 1
    if d < 4:
        return w.code(d, 5)
    e = d.bit_length() - 2
    return w.code(2 * (e + 1) + ((d >> e) & 1), 5).put(d & ((1 << e) - 1), e)


def _apply(out, length, dist):
    for _ in range(length):
        out.append(out[-dist])


def far_match_streams():
    """Hand-made valid streams with matches zlib's deflate never emits (it stops 262 short of the
    window): a stored block, then a fixed block of matches at distance 32768 exactly and just under
    it, lengths 3 to 258.  The second ends at 0xff00 bytes, so a 32768-byte window wraps under them.
    zlib's inflate is the judge of both."""
    res = []
    for name, first, plan, fill in (
            ("near_start", 32768, [(258, 32768), (3, 32768), (258, 32767), (100, 32600), (64, 32768), (65, 32768),
                                   (258, 32768), (11, 32511)], 0),
            ("near_end", 65000, [(258, 32768), (3, 32768), (7, 32768), (2, 0)], None)):
        data = bytearray(random_bytes(first, 71))
        w = BitWriter().put(1, 1).put(1, 2)
        for length, dist in plan:
            if dist == 0:   # literals
                for k in range(length):
                    w.fixed(0x41 + k)
                    data.append(0x41 + k)
            else:
                _fixed_match(w, length, dist)
                _apply(data, length, dist)
        while fill is None and len(data) < PIECE:   # matches at distance 32768 up to the member's last byte
            n = min(258, PIECE - len(data))
            if n < 3:
                w.fixed(0x5a)
                data.append(0x5a)
            else:
                _fixed_match(w, n, 32768)
                _apply(data, n, 32768)
        w.fixed(256)
        stream = _stored(bytes(data[:first])) + w.bytes()
        assert len(stream) <= 65510
        assert judge(stream, len(data)) == bytes(data), name
        res.append(("dist32768/%s/0" % name, stream, bytes(data)))
    assert len(res[1][2]) == PIECE
    return res


def handmade_corrupt():
    """(name, stream, ulen): streams that must be refused whatever else happens."""
    out = []
    # a match whose distance reaches before the first byte: 'a', then length 3 at distance 2
    w = BitWriter().put(1, 1).put(1, 2).fixed(ord("a")).fixed(257).code(1, 5).fixed(256)
    out.append(("distance_beyond_output", w.bytes(), 4))
    # a dynamic header whose code-length code gives four symbols a one-bit code
    w = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)
    for _ in range(4):
        w.put(1, 3)
    w.put(0, 32)
    out.append(("oversubscribed_lengths", w.bytes(), 4))
    # literal/length symbol 286
    w = BitWriter().put(1, 1).put(1, 2).fixed(ord("a")).fixed(286).code(0, 5).fixed(256)
    out.append(("symbol_286", w.bytes(), 4))
    # distance symbol 30
    w = BitWriter().put(1, 1).put(1, 2).fixed(ord("a")).fixed(257).code(30, 5).fixed(256)
    out.append(("distance_symbol_30", w.bytes(), 4))
    # a stored block whose NLEN is not ~LEN
    out.append(("bad_nlen", bytes([1]) + struct.pack("<HH", 4, 0xfffa) + b"abcd", 4))
    # well-formed streams against the wrong ISIZE
    good = raw_deflate(text(700, 9), 6)
    out.append(("output_longer_than_ulen", good, 699))
    out.append(("output_shorter_than_ulen", good, 701))
    stored = raw_deflate(text(700, 9), 0)
    out.append(("stored_longer_than_ulen", stored, 699))
    # a member cut short: no final block ever ends
    out.append(("no_final_block", good[:len(good) // 2], 700))
    for name, s, ulen in out:
        assert judge(s, ulen) is None, name
    return out
