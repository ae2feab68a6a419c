"""ccio_write_bam_ex with names == NULL ("the names are with the hook": cc_bam_assemble_names), without a
GPU: a Python callback stands in for the device assembler and brings its own copy of the names.  When
no hook takes such a write and a RENAME or NEW spec needs a name the result is -3, "write_bam: names
not in host memory", and nothing is written; specs that need no name are written by the host as
always; a hook that assembles from its own names writes what the host writes with the names."""
import ctypes as C
import os

import numpy as np
import pytest

import pysam  # the oracle shim
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam, Interner, make_specs
from parity import GOLDEN

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
NREC = 60
TEXT = "write_bam: names not in host memory"


def _write(path, tmpl, specs, srcs, names, name_off, cons=None):
    """ccio_write_bam_ex itself: its result.  names None goes as NULL."""
    arr = (N.P * len(srcs))(*[s.h for s in srcs])
    cs, cq = cons if cons is not None else (np.zeros(1, np.uint8), np.zeros(1, np.uint8))
    return N.io().ccio_write_bam_ex(path.encode(), tmpl.h, Interner().h, len(specs), N.ptr(specs), arr, len(srcs),
                                    None if names is None else N.ptr(names), N.ptr(name_off), N.ptr(cs), N.ptr(cq), 1, 0,
                                    0, None)


@pytest.fixture(scope="module")
def source():
    return Bam(INPUT)


@pytest.fixture(scope="module")
def named():
    """A name per record, of lengths 1..40, and their offsets."""
    names = [("n%d_" % i).encode() + b"x" * (i % 37) for i in range(NREC)]
    off = np.zeros(NREC + 1, np.int64)
    off[1:] = np.cumsum([len(n) for n in names])
    return names, np.frombuffer(b"".join(names), np.uint8).copy(), off


def _specs(kinds):
    sp = make_specs(NREC)
    sp["src_rec"] = np.arange(NREC)
    for i in range(NREC):
        k = kinds[i % len(kinds)]
        sp["kind"][i] = k
        if k != N.OUT_RAW:
            sp["name_id"][i] = i
        if k == N.OUT_NEW:
            sp["cons_off"][i], sp["cons_len"][i], sp["flag"][i], sp["mapq"][i] = 8 * i, 6, 99, 60
    return sp


CONS = (np.full(4 * NREC + 8, 0x12, np.uint8), np.full(8 * NREC + 8, 30, np.uint8))


class Hook(object):
    """A ccio_assemble_fn that renames from its own copy of the names (RAW and RENAME specs), or refuses."""

    def __init__(self, names, refuse=False):
        self.names, self.refuse = names, refuse
        self.calls, self.seen = 0, None
        self.fn = N.ASSEMBLE_FN(self._call)   # held as long as the hook may be called

    def _call(self, user, header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
              cons_seq_bytes, cons_qual, cons_qual_bytes, rg_blob, rg_off, n_rg, flags, alloc, actx, at, total):
        self.calls += 1
        off = np.ctypeslib.as_array(C.cast(name_off, C.POINTER(C.c_int64)), (n_names + 1,)).copy()
        self.seen = dict(names=names, n_names=n_names, names_bytes=names_bytes, off=off)
        if self.refuse:
            return 1
        sp = np.ctypeslib.as_array(C.cast(spec, C.POINTER(C.c_uint8)), (n * N.OUT_SPEC_DTYPE.itemsize,)).view(N.OUT_SPEC_DTYPE)
        src = C.string_at(srcs[0].stream, srcs[0].bytes)
        ro = np.ctypeslib.as_array(C.cast(srcs[0].rec_off, C.POINTER(C.c_uint64)), (srcs[0].nrec,))
        out = [C.string_at(header, header_bytes)]
        for s in sp:
            a = int(ro[s["src_rec"]])
            bs = int.from_bytes(src[a:a + 4], "little")
            rec = src[a + 4:a + 4 + bs]
            if s["kind"] == N.OUT_RAW:
                out.append(src[a:a + 4 + bs])
                continue
            nm = self.names[s["name_id"]]
            lqn = rec[8]
            body = rec[:8] + bytes([len(nm) + 1]) + rec[9:32] + nm + b"\0" + rec[32 + lqn:]
            out.append(len(body).to_bytes(4, "little") + body)
        stream = b"".join(out)
        buf = alloc(actx, len(stream))
        if not buf:
            return 1
        C.memmove(buf, stream, len(stream))
        for i, v in enumerate(np.cumsum([len(o) for o in out])):
            at[i] = int(v)
        total[0] = len(stream)
        return 0


@pytest.fixture
def hooked():
    io = N.io()
    live = []

    def use(h):
        live.append(h)
        io.ccio_set_assemble_hook(C.cast(h.fn, N.P), None)
        return h
    yield use
    io.ccio_set_assemble_hook(None, None)


@pytest.mark.parametrize("kind", [N.OUT_RENAME, N.OUT_NEW], ids=["rename", "new"])
def test_null_names_without_a_hook_is_minus_3(source, named, tmp_path, kind):
    p = str(tmp_path / "none.bam")
    sp = _specs([N.OUT_RAW, kind])
    assert _write(p, source, sp, [source], None, named[2], CONS) == -3
    assert N.io_error() == TEXT
    assert not os.path.exists(p), "nothing is written"
    # the same specs with the names are written
    assert _write(p, source, sp, [source], named[1], named[2], CONS) == 0 and os.path.getsize(p) > 0


def test_null_names_with_raw_specs_is_the_host_file(source, named, tmp_path):
    sp = _specs([N.OUT_RAW])
    a, b = str(tmp_path / "with.bam"), str(tmp_path / "without.bam")
    assert _write(a, source, sp, [source], named[1], named[2]) == 0
    assert _write(b, source, sp, [source], None, named[2]) == 0
    assert open(a, "rb").read() == open(b, "rb").read()
    # a named spec's name_id on a RAW record is not a name anybody needs
    sp["name_id"] = np.arange(NREC)
    assert _write(b, source, sp, [source], None, named[2]) == 0
    assert open(a, "rb").read() == open(b, "rb").read()


def test_hook_with_its_own_names_writes_the_host_file(hooked, source, named, tmp_path):
    sp = _specs([N.OUT_RENAME, N.OUT_RAW, N.OUT_RENAME])
    a, b = str(tmp_path / "host.bam"), str(tmp_path / "hook.bam")
    assert _write(a, source, sp, [source], named[1], named[2]) == 0   # (no hook yet: the host writer)
    h = hooked(Hook(named[0]))
    assert _write(b, source, sp, [source], None, named[2]) == 0
    assert h.calls == 1
    assert h.seen["names"] is None, "the hook receives names as NULL"
    # n_names and names_bytes still come from the host's name_off: the last named spec is NREC - 1
    last = int(sp["name_id"].max())
    assert h.seen["n_names"] == last + 1 and h.seen["names_bytes"] == named[2][last + 1]
    assert (h.seen["off"] == named[2][:last + 2]).all()
    assert open(a, "rb").read() == open(b, "rb").read()
    assert pysam.bgzf_decompress(open(b, "rb").read()).count(b"n6_xxxxxx\0") == 1


def test_refusing_hook_is_minus_3(hooked, source, named, tmp_path):
    sp = _specs([N.OUT_RENAME, N.OUT_RAW])
    p = str(tmp_path / "refused.bam")
    h = hooked(Hook(named[0], refuse=True))
    assert _write(p, source, sp, [source], None, named[2]) == -3
    assert h.calls == 1 and N.io_error() == TEXT and not os.path.exists(p)
    # a view source never reaches the hook: the same -3
    view = Bam.combine([source], key=2)
    assert _write(p, source, sp, [view], None, named[2]) == -3
    assert h.calls == 1 and N.io_error() == TEXT and not os.path.exists(p)
