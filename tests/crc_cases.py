"""Shared by the CRC32 tests: the segment lengths and start alignments at which k_crc32's per-lane
rule changes path (an empty segment, within one 16-byte word, around one word, around one lane
stride of 4,080 + 16 bytes, around two, and the ends of a BGZF piece and member), and the contents."""
import numpy as np

LENGTHS = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 4079, 4080, 4081, 4095, 4096, 4097, 4112, 8191, 8192, 8193, 65279,
           65280, 65535, 65536)
ALIGNS = (0, 1, 7, 8, 15)
LONG = (65537, 200000, (1 << 20) + 3)   # ranges the host side cuts into segments


def contents(n, seed=7):
    """name -> n bytes: zeros, 0xff, seeded random, a single set bit in the first byte and in the last."""
    first = bytearray(n)
    last = bytearray(n)
    if n:
        first[0] = 0x01
        last[n - 1] = 0x80
    return {"zeros": bytes(n), "ff": b"\xff" * n,
            "random": np.random.RandomState(seed).randint(0, 256, n, dtype=np.uint8).tobytes(),
            "first_bit": bytes(first), "last_bit": bytes(last)}
