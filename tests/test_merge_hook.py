"""libccio's merge hooks (ccio_set_merge_hooks), without a GPU: Python callbacks stand in for the
device merge on three sorted, overlapping slices of the golden basic input (the overlap gives ties
across the inputs).  A truthful hook gives the no-hook file and .bai byte for byte, through the plain
hook and through the keep hook with the resident output set (whose encoder refuses here, so the host
codec compresses the fetched rounds), with and without a kept handle, CCIO_W_ASYNC and CCIO_W_MEMORY.
Every lie is caught by libccio's checks and the host merges; with keep, each token is released
exactly once.  An unsorted input, a combined view and nine inputs never reach a hook."""
import ctypes as C
import os

import numpy as np
import pytest

from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam, Interner, Sink, flush_writes, make_specs, merge_kept, write_bam
from parity import GOLDEN
from test_out_resident_hook import _fields

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
SLICES = [(0, 120), (100, 220), (50, 90)]
LIES = ["nonzero", "tie_swap", "dup_org", "size_off", "total_off", "header"]


def _keys(stream, offs):
    k = np.zeros(len(offs), np.uint64)
    for i, a in enumerate(offs):
        tid = int.from_bytes(stream[a + 4:a + 8], "little")
        pos = (int.from_bytes(stream[a + 8:a + 12], "little") + 1) & 0xffffffff
        flag = int.from_bytes(stream[a + 18:a + 20], "little")
        k[i] = (tid << 32) | (pos << 1) | ((flag >> 4) & 1)
    return k


class Dev(object):
    """The merge hooks, the resident set they keep into, and their log."""

    def __init__(self, mode="good"):
        self.mode, self.calls, self.keep_calls, self.need_host = mode, 0, 0, []
        self.tokens, self.released, self.next, self.index_calls = {}, [], 71, 0
        self.fn = N.MERGE_FN(self._merge)
        self.kfn = N.MERGE_KEEP_FN(self._keep)
        self.set = (N.ASSEMBLE_KEEP_FN(lambda *a: 1), N.DEFLATE_RESIDENT_FN(lambda *a: 1), N.INDEX_FIELDS_FN(self._index),
                    N.RESIDENT_FETCH_FN(self._fetch), N.RESIDENT_RELEASE_FN(self._release))
        self.cb = N.ccio_out_resident(*[C.cast(f, N.P) for f in self.set])

    def _build(self, header, header_bytes, srcs, nsrc):
        hdr = C.string_at(header, header_bytes)
        recs, keys = [], []
        for f in range(nsrc):
            s = srcs[f]
            st = C.string_at(s.stream, s.bytes) if s.bytes else b""
            off = [C.cast(s.rec_off, C.POINTER(C.c_uint64))[i] for i in range(s.nrec)]
            keys.append(_keys(st, off))
            recs += [st[a:a + 4 + int.from_bytes(st[a:a + 4], "little")] for a in off]
        keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
        org = [int(v) for v in np.argsort(keys, kind="stable")]
        m = self.mode
        if m == "tie_swap":   # two tied records of different sources, the later source first
            i = next(i for i in range(len(org) - 1) if keys[org[i]] == keys[org[i + 1]] and
                     len(recs[org[i]]) == len(recs[org[i + 1]]))
            org[i], org[i + 1] = org[i + 1], org[i]
        stream = bytearray(hdr + b"".join(recs[g] for g in org))
        at = list(np.cumsum([len(hdr)] + [len(recs[g]) for g in org]))
        total = len(stream)
        if m == "dup_org":
            org[4] = org[3]
        if m == "size_off":
            at[6] += 1
        if m == "total_off":
            total += 1
        if m == "header":
            stream[len(hdr) - 1] ^= 1
        return bytes(stream), at, org, total

    def _fill(self, stream, at_v, org_v, total_v, alloc, actx, at, org, total, host):
        if host:
            buf = alloc(actx, len(stream))
            if not buf:
                return 1
            C.memmove(buf, stream, len(stream))
        for i, v in enumerate(at_v):
            at[i] = int(v)
        for i, v in enumerate(org_v):
            org[i] = v
        total[0] = total_v
        return 0

    def _merge(self, user, header, header_bytes, srcs, nsrc, alloc, actx, at, org, total):
        self.calls += 1
        if self.mode == "nonzero":
            return 1
        stream, at_v, org_v, total_v = self._build(header, header_bytes, srcs, nsrc)
        return self._fill(stream, at_v, org_v, total_v, alloc, actx, at, org, total, True)

    def _keep(self, user, header, header_bytes, srcs, nsrc, alloc, actx, need_host, at, org, total, token):
        self.keep_calls += 1
        self.need_host.append(need_host)
        if self.mode == "nonzero":
            return 1
        stream, at_v, org_v, total_v = self._build(header, header_bytes, srcs, nsrc)
        token[0] = self.next
        self.tokens[self.next] = stream
        self.next += 1
        return self._fill(stream, at_v, org_v, total_v, alloc, actx, at, org, total, need_host)

    def _index(self, user, token, at, n, fields):
        self.index_calls += 1
        f = _fields(self.tokens[token], [at[i] for i in range(n + 1)])
        C.memmove(fields, f.ctypes.data, f.nbytes)
        return 0

    def _fetch(self, user, token, off, n, dst):
        C.memmove(dst, self.tokens[token][off:off + n], n)
        return 0

    def _release(self, user, token):
        self.released.append(token)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Three sorted kept handles over slices of the input (records in place in their own streams)."""
    src = Bam(INPUT)
    hs = []
    for k, (a, b) in enumerate(SLICES):
        sp = make_specs(b - a)
        sp["kind"] = N.OUT_RAW
        sp["src_rec"] = np.arange(a, b)
        p = str(tmp_path_factory.mktemp("in%d" % k) / "in.bam")
        sink = Sink(fused=[p], keep=[p])
        out = write_bam(p, src, Interner(), sp, [src], level=1, sink=sink)
        hs.append(sink.take(out))
    yield hs
    for h in hs:
        h.close()


def _merge(inputs, d, name, **kw):
    p = str(d / name)
    h = merge_kept(p, inputs, level=1, **kw)
    if kw.get("async_writes"):
        flush_writes()
    return p, h


def _all(h):
    return h.pack(np.arange(h.n, dtype=np.int64)).tobytes()


@pytest.fixture(scope="module")
def host(inputs, tmp_path_factory):
    p, h = _merge(inputs, tmp_path_factory.mktemp("host"), "host.bam")
    ref = dict(bam=open(p, "rb").read(), bai=open(p + ".bai", "rb").read(), recs=_all(h))
    h.close()
    return ref


@pytest.fixture
def wired():
    io = N.io()

    def use(kind, mode="good"):
        d = Dev(mode)
        if kind == "keep":
            io.ccio_set_out_resident(C.byref(d.cb), None)
            io.ccio_set_merge_hooks(None, C.cast(d.kfn, N.P), None)
        else:
            io.ccio_set_merge_hooks(C.cast(d.fn, N.P), None, None)
        return d
    yield use
    io.ccio_flush()
    io.ccio_set_merge_hooks(None, None, None)
    io.ccio_set_out_resident(None, None)


def _once(d):
    assert sorted(d.released) == sorted(d.tokens) and len(set(d.released)) == len(d.released)


@pytest.mark.parametrize("kind", ["plain", "keep"])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("async_writes", [False, True])
def test_truthful_hook_gives_the_host_files(wired, inputs, host, tmp_path, kind, keep, async_writes):
    d = wired(kind)
    p, h = _merge(inputs, tmp_path, "out.bam", keep=keep, async_writes=async_writes)
    assert (d.keep_calls if kind == "keep" else d.calls) == 1
    assert open(p, "rb").read() == host["bam"]
    assert open(p + ".bai", "rb").read() == host["bai"]
    if keep:
        assert _all(h) == host["recs"]
        h.close()
    if kind == "keep":
        assert d.need_host == [1 if keep else 0] and d.index_calls == 1
        _once(d)
        assert len(d.tokens) == 1


@pytest.mark.parametrize("kind", ["plain", "keep"])
def test_truthful_hook_in_memory(wired, inputs, host, tmp_path, kind):
    d = wired(kind)
    h = merge_kept(None, inputs, memory=True)
    assert (d.keep_calls if kind == "keep" else d.calls) == 1
    assert _all(h) == host["recs"]
    h.close()
    _once(d)


@pytest.mark.parametrize("kind", ["plain", "keep"])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("mode", LIES)
def test_every_lie_leaves_the_host_files(wired, inputs, host, tmp_path, kind, keep, mode):
    d = wired(kind, mode)
    p, h = _merge(inputs, tmp_path, "out.bam", keep=keep)
    assert (d.keep_calls if kind == "keep" else d.calls) == 1
    assert open(p, "rb").read() == host["bam"]
    assert open(p + ".bai", "rb").read() == host["bai"]
    if keep:
        assert _all(h) == host["recs"]
        h.close()
    _once(d)
    assert len(d.tokens) == (1 if kind == "keep" and mode != "nonzero" else 0)
    assert d.index_calls == 0   # refused by the checks (the same pass serves both hooks), not merely equal bytes


def test_unsorted_view_and_nine_inputs_never_reach_a_hook(wired, inputs, tmp_path):
    io = N.io()
    d = Dev()
    io.ccio_set_out_resident(C.byref(d.cb), None)
    io.ccio_set_merge_hooks(C.cast(d.fn, N.P), C.cast(d.kfn, N.P), None)   # (the fixture unsets them)
    wired  # noqa: B018
    src = Bam(INPUT)
    sp = make_specs(40)
    sp["kind"] = N.OUT_RAW
    sp["src_rec"] = np.arange(40)[::-1]
    un = Bam(write_bam(str(tmp_path / "unsorted.bam"), src, Interner(), sp, [src], level=1))
    assert not un.is_sorted(1)
    view = Bam.combine([inputs[2]], key=1)
    cases = dict(unsorted=[inputs[0], un], view=[inputs[0], view], nine=[inputs[k % 3] for k in range(9)])
    for name, ins in cases.items():
        on = merge_kept(str(tmp_path / (name + ".on.bam")), ins, level=1, keep=False)
        assert on is None and d.calls == 0 and d.keep_calls == 0, name
        io.ccio_set_merge_hooks(None, None, None)
        merge_kept(str(tmp_path / (name + ".off.bam")), ins, level=1, keep=False)
        io.ccio_set_merge_hooks(C.cast(d.fn, N.P), C.cast(d.kfn, N.P), None)
        for ext in ("", ".bai"):
            assert open(str(tmp_path / (name + ".on.bam")) + ext, "rb").read() == \
                open(str(tmp_path / (name + ".off.bam")) + ext, "rb").read(), name
    eight = merge_kept(str(tmp_path / "eight.bam"), [inputs[k % 3] for k in range(8)], level=1, keep=False)
    assert eight is None and d.keep_calls == 1   # eight inputs do
    _once(d)
    view.close()
    un.close()


def test_unset_is_the_host_merge_again(wired, inputs, host, tmp_path):
    d = wired("plain")
    N.io().ccio_set_merge_hooks(None, None, None)
    p, h = _merge(inputs, tmp_path, "out.bam", keep=False)
    assert d.calls == 0 and open(p, "rb").read() == host["bam"]
