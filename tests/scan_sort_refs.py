"""numpy references for the engine's prefix scan and radix sort (tests/test_gpu_scan_sort.py compares the
kernels with them; tests/test_scan_sort_reference.py checks them on hand-written cases without a GPU)."""
import numpy as np

TILE = 4096                 # the scan's tile (SCAN_TILE) and the sort's (RS_TILE)
TAIL = 64                   # canary elements behind every output array of the debug hooks
CANARY = 0xA5A5A5A5         # their 32-bit fill


def ref_scan(values):
    """Exclusive prefix sum and total, in int64."""
    v = np.asarray(values).astype(np.int64)
    inc = np.cumsum(v, dtype=np.int64)
    excl = inc - v
    return excl, (int(inc[-1]) if len(v) else 0)


def ref_compact(flags, aux=None):
    """The flagged indices compacted: vslot[i] = rank of i among the flagged (-1 when not flagged),
    list[k] = the k-th flagged index, and with aux = (t_rec, p_rec, dec) also
    vpair[k] = (t_rec[i], p_rec[i], dec[i], i) for i = list[k]."""
    flags = np.asarray(flags)
    idx = np.flatnonzero(flags).astype(np.int64)
    vslot = np.full(len(flags), -1, np.int64)
    vslot[idx] = np.arange(len(idx), dtype=np.int64)
    vpair = None
    if aux is not None:
        t_rec, p_rec, dec = (np.asarray(a).astype(np.int64) for a in aux)
        vpair = np.stack([t_rec[idx], p_rec[idx], dec[idx], idx], axis=1).reshape(len(idx), 4)
    return vslot, idx, vpair


def sort_window(begin_bit, end_bit):
    """The key bits the sort orders by: whole 8-bit digits from begin_bit, clipped at 64."""
    passes = (end_bit - begin_bit + 7) // 8 if end_bit > begin_bit else 0
    return begin_bit, min(64, begin_bit + 8 * passes)


def window_digits(keys, begin_bit, end_bit):
    """The keys restricted to the sort's window (uint64)."""
    keys = np.asarray(keys, np.uint64)
    lo, hi = sort_window(begin_bit, end_bit)
    if hi == lo:
        return np.zeros(len(keys), np.uint64)
    return (keys >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)


def ref_sort(keys, vals, begin_bit, end_bit):
    """Stable sort by the window: the whole keys in that order, the values with them."""
    keys = np.asarray(keys, np.uint64)
    vals = np.asarray(vals, np.uint32)
    order = np.argsort(window_digits(keys, begin_bit, end_bit), kind="stable")
    return keys[order], vals[order]
