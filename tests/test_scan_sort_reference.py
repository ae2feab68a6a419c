"""The numpy references of tests/test_gpu_scan_sort.py on hand-written cases (no GPU): a wrong
reference must not be able to agree with a wrong kernel by construction."""
import numpy as np

from scan_sort_refs import ref_compact, ref_scan, ref_sort, sort_window, window_digits


def test_scan_six_elements():
    excl, total = ref_scan(np.array([3, 0, 5, 1, 0, 2], np.uint32))
    assert excl.tolist() == [0, 3, 3, 8, 9, 9]
    assert total == 11
    excl, total = ref_scan(np.zeros(0, np.uint8))
    assert excl.tolist() == [] and total == 0
    # byte flags do not wrap at 256, u32 values not at 2^32
    excl, total = ref_scan(np.ones(300, np.uint8))
    assert excl[-1] == 299 and total == 300
    excl, total = ref_scan(np.full(3, 0xC0000000, np.uint32))
    assert excl.tolist() == [0, 0xC0000000, 0x180000000] and total == 0x240000000


def test_compaction_five_flags():
    flags = np.array([0, 1, 1, 0, 1], np.uint8)
    t_rec = np.array([10, 11, 12, 13, 14], np.int32)
    p_rec = np.array([20, 21, 22, 23, 24], np.int32)
    dec = np.array([0, 1, 2, 3, 0], np.int32)
    vslot, lst, vpair = ref_compact(flags, (t_rec, p_rec, dec))
    assert vslot.tolist() == [-1, 0, 1, -1, 2]
    assert lst.tolist() == [1, 2, 4]
    assert vpair.tolist() == [[11, 21, 1, 1], [12, 22, 2, 2], [14, 24, 0, 4]]
    vslot, lst, vpair = ref_compact(np.zeros(3, np.uint8), (t_rec[:3], p_rec[:3], dec[:3]))
    assert vslot.tolist() == [-1, -1, -1] and lst.tolist() == [] and vpair.shape == (0, 4)
    assert ref_compact(flags)[2] is None


def test_sort_window():
    assert sort_window(0, 64) == (0, 64)
    assert sort_window(0, 48) == (0, 48)
    assert sort_window(0, 1) == (0, 8)          # whole digits: wider than [0, 1)
    assert sort_window(4, 12) == (4, 12)
    assert sort_window(3, 12) == (3, 19)
    assert sort_window(16, 40) == (16, 40)
    assert sort_window(56, 64) == (56, 64)
    assert sort_window(60, 63) == (60, 64)      # clipped at 64
    assert sort_window(0, 0) == (0, 0)


def test_sort_six_pairs_window_4_12():
    # digit = bits [4, 12); the low nibble and the bits from 12 up must not matter
    keys = np.array([0x5023,               # digit 0x02
                     0x101F,               # digit 0x01
                     0x0020,               # digit 0x02 (ties with pair 0, stays behind it)
                     0xF007,               # digit 0x00
                     0x2011,               # digit 0x01 (ties with pair 1; its low nibble is smaller)
                     0x8000000000000FFE],  # digit 0xff
                    np.uint64)
    vals = np.array([100, 101, 102, 103, 104, 105], np.uint32)
    assert window_digits(keys, 4, 12).tolist() == [0x02, 0x01, 0x02, 0x00, 0x01, 0xFF]
    k, v = ref_sort(keys, vals, 4, 12)
    assert v.tolist() == [103, 101, 104, 100, 102, 105]
    assert k.tolist() == [0xF007, 0x101F, 0x2011, 0x5023, 0x0020, 0x8000000000000FFE]
    # no pass: a plain copy
    k, v = ref_sort(keys, vals, 0, 0)
    assert k.tolist() == keys.tolist() and v.tolist() == vals.tolist()
    # the full key
    k, v = ref_sort(keys, vals, 0, 64)
    assert v.tolist() == [102, 101, 104, 100, 103, 105]
