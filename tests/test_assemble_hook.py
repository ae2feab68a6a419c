"""libccio's assemble hook (ccio_set_assemble_hook), without a GPU: a Python callback stands in for
the device assembler.  A hook that refuses, or whose stream fails one of libccio's checks (a wrong
block_size, offsets that do not increase, a short total), leaves the bytes the host assembles; a
correct hook's own bytes are written (here: the records in reverse, which only the hook produces);
a view source never reaches the hook; with the hook unset the writer is the host's again."""
import ctypes as C
import os

import numpy as np
import pytest

import pysam  # the oracle shim
from consensuscruncher_amd import native as N
from consensuscruncher_amd.engine import Bam, Interner, make_specs, write_bam
from parity import GOLDEN

INPUT = os.path.join(GOLDEN, "basic", "input.bam")
NREC = 300


class Hook(object):
    """A ccio_assemble_fn and its call log.  mode: "refuse", "good" (the records in reverse order),
    "block_size", "non_monotone" or "short"."""

    def __init__(self, mode, records, header):
        self.mode, self.records, self.header = mode, records, header
        self.calls = 0
        self.seen = None
        self.fn = N.ASSEMBLE_FN(self._call)   # held as long as the hook may be called

    def _call(self, user, header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
              cons_seq_bytes, cons_qual, cons_qual_bytes, rg_blob, rg_off, n_rg, flags, alloc, actx, at, total):
        self.calls += 1
        self.seen = dict(nsrc=nsrc, n=n, header=C.string_at(header, header_bytes), nrec=srcs[0].nrec, bytes=srcs[0].bytes,
                         first=C.string_at(srcs[0].stream, 4), resident=srcs[0].resident_id)
        if self.mode == "refuse":
            return 1
        recs = list(reversed(self.records))
        if self.mode == "block_size":
            recs[5] = (len(recs[5]) - 3).to_bytes(4, "little") + recs[5][4:]
        stream = self.header + b"".join(recs)
        offs = np.cumsum([len(self.header)] + [len(r) for r in recs]).astype(np.uint64)
        if self.mode == "non_monotone":
            offs[7], offs[8] = offs[8], offs[7]
        if self.mode == "short":
            stream = stream[:-1]
            offs[-1] -= 1
        buf = alloc(actx, len(stream))
        if not buf:
            return 1
        C.memmove(buf, stream, len(stream))
        for i, v in enumerate(offs):
            at[i] = int(v)
        total[0] = len(stream)
        return 0


@pytest.fixture(scope="module")
def source():
    return Bam(INPUT)


@pytest.fixture(scope="module")
def job(source, tmp_path_factory):
    """NREC raw copies of the input's first records, what the host writes for them, and its records."""
    sp = make_specs(NREC)
    sp["kind"] = N.OUT_RAW
    sp["src_rec"] = np.arange(NREC)
    p = str(tmp_path_factory.mktemp("host") / "host.bam")
    write_bam(p, source, Interner(), sp, [source], level=1)
    stream = pysam.bgzf_decompress(open(p, "rb").read())
    packed = source.pack(np.arange(NREC, dtype=np.int64)).tobytes()
    header = stream[:len(stream) - len(packed)]
    assert stream == header + packed
    recs, a = [], 0
    while a < len(packed):
        b = a + 4 + int.from_bytes(packed[a:a + 4], "little")
        recs.append(packed[a:b])
        a = b
    assert len(recs) == NREC
    return sp, open(p, "rb").read(), recs, header


@pytest.fixture
def hooked(job):
    io = N.io()
    live = []

    def use(mode):
        h = Hook(mode, job[2], job[3])
        live.append(h)
        io.ccio_set_assemble_hook(C.cast(h.fn, N.P), None)
        return h
    yield use
    io.ccio_set_assemble_hook(None, None)


@pytest.mark.parametrize("mode", ["refuse", "block_size", "non_monotone", "short"])
def test_rejected_hook_leaves_the_host_bytes(hooked, source, job, tmp_path, mode):
    h = hooked(mode)
    p = str(tmp_path / "fallback.bam")
    write_bam(p, source, Interner(), job[0], [source], level=1)
    assert h.calls == 1
    assert open(p, "rb").read() == job[1]


def test_correct_hook_gives_its_bytes(hooked, source, job, tmp_path):
    h = hooked("good")
    p = str(tmp_path / "hooked.bam")
    write_bam(p, source, Interner(), job[0], [source], level=1)
    assert h.calls == 1
    assert pysam.bgzf_decompress(open(p, "rb").read()) == job[3] + b"".join(reversed(job[2]))
    # what the hook was handed: the header, the source's own stream and its records
    assert h.seen["header"] == job[3] and h.seen["nsrc"] == 1 and h.seen["n"] == NREC and h.seen["resident"] == 0
    assert h.seen["nrec"] == source.n and h.seen["first"] == job[2][0][:4]


def test_view_source_never_reaches_the_hook(hooked, source, job, tmp_path):
    h = hooked("good")
    view = Bam.combine([source], key=2)
    p = str(tmp_path / "view.bam")
    write_bam(p, source, Interner(), job[0], [view], level=1)
    assert h.calls == 0
    assert open(p, "rb").read() == job[1]


def test_unset_hook_is_the_host_writer_again(hooked, source, job, tmp_path):
    h = hooked("good")
    N.io().ccio_set_assemble_hook(None, None)
    p = str(tmp_path / "unset.bam")
    write_bam(p, source, Interner(), job[0], [source], level=1)
    assert h.calls == 0
    assert open(p, "rb").read() == job[1]
