"""Host orchestration around the C ABI: BAM decode -> SoA -> HBM -> GPU stages -> BAM.

Result arrays fetched from a read_bam group (cc_fetch names):
  read_bam            fam_sizes_by_creation[F] (after cc_consensus_maker), bad_rec[NB]
  cc_consensus_maker  emit_fam/emit_n/emit_rec/emit_vslot[NE], emit_ckey[9*NE/2] (per entry),
                      vote_meta[5*NV] (L, mapq, tlen, flag, rg), cons_seq, cons_qual
  cc_duplex_consensus dec/t_rec/p_rec/vslot[Q], vote_meta, cons_seq, cons_qual
  cc_singleton_corr.  dec/t_rec/p_rec/vslot[Q], q_ckey[9*Q], vote_meta, cons_seq, cons_qual
dec codes: DCS 0 = duplex made, 1 = SSCS singleton, 2 = partner already used, 3 = empty slot;
           SC  0 = corrected by SSCS, 1 = by singleton, 2 = uncorrected, 3 = empty slot.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import native as N
from .consensus_helper import region_list, region_runs

MODE_SSCS, MODE_DUPLEX = 0, 1


class Interner(object):
    def __init__(self):
        self.h = N.io().ccio_interner_new()

    def __del__(self):
        try:
            if self.h:
                N.io().ccio_interner_free(self.h)
        except Exception:
            pass

    def size(self, kind):
        return int(N.io().ccio_interner_size(self.h, kind))

    def get(self, kind, i):
        buf = C.create_string_buffer(4096)
        n = N.io().ccio_interner_get(self.h, kind, int(i), buf, 4096)
        if n < 0:
            raise KeyError(i)
        return buf.value.decode()

    def intern(self, kind, s):
        return int(N.io().ccio_interner_intern(self.h, kind, s.encode()))

    def blob(self, kind):
        """A table's strings side by side (ccio_interner_blob): (uint8 blob, int64 offsets, size + 1 of them)."""
        off = np.zeros(self.size(kind) + 1, np.int64)
        need = int(N.io().ccio_interner_blob(self.h, kind, None, 0, N.ptr(off)))
        if need < 0:
            raise RuntimeError(N.io_error())
        blob = np.zeros(max(need, 1), np.uint8)
        if int(N.io().ccio_interner_blob(self.h, kind, N.ptr(blob), need, N.ptr(off))) != need:
            raise RuntimeError(N.io_error())
        return blob, off

    def swap_table(self):
        n = int(N.io().ccio_interner_swap_table(self.h, None, 0))
        out = np.zeros(max(n, 1), np.int32)
        N.io().ccio_interner_swap_table(self.h, N.ptr(out), n)
        return out[:n]


class Records(object):
    """cc_records SoA as numpy arrays (owned here, pointed to by .struct)."""

    FIELDS = [("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("tlen", np.int32),
              ("flag", np.uint16), ("mapq", np.uint8), ("cigar_id", np.int32), ("qlen", np.int32),
              ("lseq", np.int32), ("bc_id", np.int32), ("rg_id", np.int32), ("rflags", np.uint8),
              ("qn_off", np.uint64), ("qn_len", np.uint16), ("pay_off", np.uint64), ("rdig", np.uint64)]

    # the kernels' per-record layout, built by the decoder (cc_records' derived columns): per record
    # (dtype, values per record)
    DERIVED = [("rkey", np.uint64, 1), ("meta", np.uint32, 4), ("core", np.int32, 8), ("qn_ol", np.uint64, 1),
               ("qdig", np.uint64, 1), ("rdeep", np.uint8, 1)]

    def __init__(self, n, qn_bytes, pay_bytes, max_len, nref=0, derived=True):
        self.n = int(n)
        self.max_len = int(max_len)
        for name, dt in self.FIELDS:
            setattr(self, name, np.zeros(max(self.n, 1), dt))
        self.qn_blob = np.zeros(int(qn_bytes) + 16, np.uint8)
        self.payload = np.zeros(int(pay_bytes) + 64, np.uint8)
        s = N.cc_records()
        s.n = self.n
        for name, _ in self.FIELDS:
            setattr(s, name, getattr(self, name).ctypes.data)
        s.qn_blob = self.qn_blob.ctypes.data
        s.qn_blob_bytes = int(qn_bytes)
        s.payload = self.payload.ctypes.data
        s.payload_bytes = int(pay_bytes)
        s.rdig = self.rdig.ctypes.data
        self.derived = bool(derived) and not os.environ.get("CC_DEVICE_DERIVE")
        if self.derived:
            for name, dt, k in self.DERIVED:
                setattr(self, name, np.empty(max(self.n, 1) * k, dt))
                setattr(s, name, getattr(self, name).ctypes.data)
            self.dlist = np.empty(self.n // 65 + 2, np.int32)
            self.ext = np.zeros(max(int(nref), 1), np.int32)
            s.dlist = self.dlist.ctypes.data
            s.ext = self.ext.ctypes.data
            s.n_ext = int(nref)
        self.struct = s


class Bam(object):
    """A BAM file decoded into memory by libccio (pysam.AlignmentFile stand-in)."""

    def __init__(self, path, nthreads=0):
        self.path = path
        self._attach(N.io().ccio_bam_open(path.encode(), nthreads))

    def _attach(self, h):
        if not h:
            raise IOError(N.io_error())
        self.h = h
        self._res_owner = None   # the engine that holds this handle's resident stream (resident)
        if _KEEP_OWNER is not None:
            tok = C.c_int64()
            if N.io().ccio_bam_resident(self.h, C.byref(tok), C.byref(C.c_uint64())):
                self._res_owner = weakref.ref(_KEEP_OWNER)
        self.n = int(N.io().ccio_bam_nrec(self.h))
        self.refs = []
        buf = C.create_string_buffer(4096)
        ln = C.c_int32()
        for i in range(int(N.io().ccio_bam_nref(self.h))):
            N.io().ccio_bam_ref(self.h, i, buf, 4096, C.byref(ln))
            self.refs.append((buf.value.decode(), ln.value))

    @classmethod
    def _handle(cls, h, path=None):
        b = cls.__new__(cls)
        b.path = path
        b.h = None
        b._attach(h)
        return b

    # ---- rank-local record sets (the multi-GPU driver, sharded.py)
    @classmethod
    def open_regions(cls, path, tids, begs, ends, nthreads=0):
        """The records with beg <= pos < end on tid of one of the regions, in file order, read through
        path's BAI (only the regions' BGZF blocks are read)."""
        t = np.ascontiguousarray(tids, np.int32)
        b = np.ascontiguousarray(begs, np.int64)
        e = np.ascontiguousarray(ends, np.int64)
        return cls._handle(N.io().ccio_bam_open_regions(path.encode(), len(t), N.ptr(t), N.ptr(b), N.ptr(e),
                                                        nthreads), path)

    @classmethod
    def combine(cls, parts, blobs=(), key=1, tmpl=None):
        """parts' records then the raw record blobs', in that order, stably sorted by key (0: tid, pos;
        1: the samtools-sort stand-in key tid, pos, is_reverse; 2: unsorted)."""
        hs = (N.P * max(len(parts), 1))(*[p.h for p in parts])
        blobs = [np.ascontiguousarray(x, np.uint8) for x in blobs]
        bp = (N.P * max(len(blobs), 1))(*[x.ctypes.data for x in blobs])
        bn = np.array([len(x) for x in blobs] or [0], np.int64)
        h = N.io().ccio_bam_combine(tmpl.h if tmpl is not None else None, hs, len(parts), bp, N.ptr(bn), len(blobs),
                                    int(key), 0)
        return cls._handle(h)

    def origin(self):
        out = np.zeros(max(self.n, 1), np.int64)
        if N.io().ccio_bam_origin(self.h, N.ptr(out)) != 0:
            raise IOError(N.io_error())
        return out[:self.n]

    def cores(self):
        """(tid, pos, mtid, mpos, flag) of every record."""
        n = max(self.n, 1)
        t, p, mt, mp = (np.zeros(n, np.int32) for _ in range(4))
        f = np.zeros(n, np.uint16)
        N.io().ccio_bam_cores(self.h, N.ptr(t), N.ptr(p), N.ptr(mt), N.ptr(mp), N.ptr(f))
        return t[:self.n], p[:self.n], mt[:self.n], mp[:self.n], f[:self.n]

    def pack(self, idx):
        """The raw records idx (block_size first), concatenated."""
        i = np.ascontiguousarray(idx, np.int64)
        need = N.io().ccio_bam_pack(self.h, len(i), N.ptr(i), None, 0)
        if need < 0:
            raise IOError(N.io_error())
        out = np.zeros(max(int(need), 1), np.uint8)
        N.io().ccio_bam_pack(self.h, len(i), N.ptr(i), N.ptr(out), int(need))
        return out[:int(need)]

    def write_all(self, path, level=6, nthreads=0):
        if N.io().ccio_bam_write_all(path.encode(), self.h, level, nthreads) != 0:
            raise IOError(N.io_error())

    def write(self, path, level=6, index=False, async_write=False, nthreads=0):
        """The records as they stand written to path (+ path.bai with index: in samtools-sort order);
        async_write: compressed in the background (flush_writes)."""
        fl = (N.W_INDEX if index else 0) | (N.W_ASYNC if async_write else 0)
        if N.io().ccio_bam_write_ex(path.encode(), self.h, level, nthreads, fl) != 0:
            raise IOError(N.io_error())

    def is_sorted(self, key=1):
        """True when the records are in key order (0: tid, pos; 1: the samtools-sort stand-in's)."""
        return bool(N.io().ccio_bam_is_sorted(self.h, int(key)))

    def route(self, keep, blobs=(), own_at=0, key=1):
        """A rank's part of a routed record set: the raw record blobs' records (sender order) with this
        handle's records that have keep[i] (all when keep is None) placed before blob own_at, stably
        sorted by key (as combine)."""
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        blobs = [np.ascontiguousarray(x, np.uint8) for x in blobs]
        bp = (N.P * max(len(blobs), 1))(*[x.ctypes.data for x in blobs])
        bn = np.array([len(x) for x in blobs] or [0], np.int64)
        h = N.io().ccio_bam_route(self.h, N.ptr(k) if k is not None else None, int(own_at), bp, N.ptr(bn), len(blobs),
                                  int(key), 0)
        return Bam._handle(h)

    def resident(self):
        """(engine, id, base) when the engine's inflater kept this file's inflated bytes on the device
        (Engine.device_resident) and the handle's records are still that stream's own, from byte base
        on (ccio_bam_resident); None otherwise: views, combined handles, region opens, a handle whose
        stream was consumed (resident_done) or whose engine is closed."""
        eng = self._res_owner() if self._res_owner is not None else None
        if eng is None or not eng.h or not self.h:
            return None
        tok, base = C.c_int64(), C.c_uint64()
        if not N.io().ccio_bam_resident(self.h, C.byref(tok), C.byref(base)):
            return None
        return eng, int(tok.value), int(base.value)

    def resident_done(self):
        """The resident stream is freed (Engine.unpack): close has nothing left to free."""
        self._res_owner = None

    def close(self):
        if self.h:
            # a resident stream nobody unpacked (a stats-only open) goes with the handle while its engine
            # lives; cc_destroy frees it otherwise
            eng = self._res_owner() if getattr(self, "_res_owner", None) is not None else None
            if eng is not None and eng.h:
                tok = C.c_int64()
                if N.io().ccio_bam_resident(self.h, C.byref(tok), C.byref(C.c_uint64())):
                    eng.lib.cc_resident_free(eng.h, tok.value)
            self._res_owner = None
            N.io().ccio_bam_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def qname(self, i):
        buf = C.create_string_buffer(1024)
        N.io().ccio_bam_qname(self.h, int(i), buf, 1024)
        return buf.value.decode()

    def decode(self, interner, mode, delim="|", nthreads=0):
        qn = C.c_uint64()
        pay = C.c_uint64()
        ml = C.c_int32()
        N.io().ccio_bam_layout(self.h, C.byref(qn), C.byref(pay), C.byref(ml), nthreads)
        rec = Records(self.n, qn.value, pay.value, ml.value, nref=len(self.refs))
        rc = N.io().ccio_bam_decode(self.h, interner.h, mode, (delim or "|").encode(), C.byref(rec.struct), nthreads)
        if rc != 0:
            raise IOError(N.io_error())
        return rec

    def decode_ids(self, interner, mode, delim="|", nthreads=0):
        """The slim decode in front of the device unpacker (ccio_bam_decode_ids): (records, stream,
        rec_off).  records is a Records with its host integer columns, ids and rflags filled and no
        blobs (qn_off, pay_off, rdig and the derived columns stay unset); stream is a uint8 view of
        the handle's records as one contiguous stream (valid while this handle is open and not
        decoded again), rec_off each record's offset in it."""
        rec = Records(self.n, 0, 0, 0, nref=len(self.refs), derived=False)
        off = np.zeros(max(self.n, 1), np.uint64)
        sp, sb, ml = N.P(), C.c_uint64(), C.c_int32()
        rc = N.io().ccio_bam_decode_ids(self.h, interner.h, mode, (delim or "|").encode(), C.byref(rec.struct), nthreads,
                                        C.byref(sp), C.byref(sb), N.ptr(off), C.byref(ml))
        if rc != 0:
            raise IOError(N.io_error())
        rec.max_len = int(ml.value)
        if sb.value:
            stream = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint8)), shape=(int(sb.value),))
        else:
            stream = np.zeros(0, np.uint8)
        return rec, stream, off[:self.n]

    def decode_cols(self, nthreads=0):
        """decode_ids without the string pass (ccio_bam_decode_cols), in front of the device interner:
        (records, stream, rec_off) as decode_ids gives them, but the records' cigar_id, bc_id and rg_id
        are unset and rflags holds the parser's bit (CC_RF_QUAL_MISSING) only."""
        rec = Records(self.n, 0, 0, 0, nref=len(self.refs), derived=False)
        off = np.zeros(max(self.n, 1), np.uint64)
        sp, sb, ml = N.P(), C.c_uint64(), C.c_int32()
        rc = N.io().ccio_bam_decode_cols(self.h, C.byref(rec.struct), nthreads, C.byref(sp), C.byref(sb), N.ptr(off),
                                         C.byref(ml))
        if rc != 0:
            raise IOError(N.io_error())
        rec.max_len = int(ml.value)
        if sb.value:
            stream = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint8)), shape=(int(sb.value),))
        else:
            stream = np.zeros(0, np.uint8)
        return rec, stream, off[:self.n]

    def intern_first(self, interner, mode, delim, local, first, nthreads=0, out=None):
        """The device interner's local ids turned into the interner's (ccio_intern_first).  local: the
        three int32[n] local-id columns (barcode, cigar, RG; -1: none), first: per table the record of
        each local id's first occurrence.  Returns (bc_id, cigar_id, rg_id) as decode_ids gives them
        (written into out's three int32 arrays when given)."""
        n = self.n
        local = [np.ascontiguousarray(a, np.int32) for a in local]
        first = [np.ascontiguousarray(a, np.int32) for a in first]
        assert all(len(a) == n for a in local)
        out = out or [np.zeros(max(n, 1), np.int32) for _ in range(3)]
        assert all(a.dtype == np.int32 and a.flags.c_contiguous and len(a) >= n for a in out)
        nd = np.array([len(a) for a in first], np.int32)
        lp = (N.P * 3)(*[N.ptr(a) for a in local])
        fp = (N.P * 3)(*[N.ptr(a) if len(a) else None for a in first])
        rc = N.io().ccio_intern_first(self.h, interner.h, mode, (delim or "|").encode(), fp, N.ptr(nd), lp, n,
                                      N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), nthreads)
        if rc != 0:
            raise IOError(N.io_error())
        return out[0][:n], out[1][:n], out[2][:n]

    def intern_keys(self, mode, delim="|"):
        """Test entry (ccio_intern_keys): the device interner's key finders run on the host.  Returns
        (off[3, n], len[3, n], none[3, n], flags[n], refuse[n]); rows: barcode, cigar, RG."""
        n = self.n
        off, ln = np.zeros((3, max(n, 1)), np.uint32), np.zeros((3, max(n, 1)), np.uint32)
        none, flags, refuse = np.zeros((3, max(n, 1)), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        if n:
            if N.io().ccio_intern_keys(self.h, mode, (delim or "|").encode(), N.ptr(off), N.ptr(ln), N.ptr(none),
                                       N.ptr(flags), N.ptr(refuse)) != 0:
                raise IOError(N.io_error())
        return off[:, :n], ln[:, :n], none[:, :n], flags[:n], refuse[:n]


class Stream(object):
    """The order in which read_bam sees records: whole file (until_eof) or the bed
    regions in file order, each region = records with start <= pos < end on its
    contig (pysam overlap fetch + the pos filter of consensus_helper.py:391-396)."""

    def __init__(self, rec_idx, region, region_run, region_keys):
        self.rec = np.ascontiguousarray(rec_idx, np.int32)
        self.region = np.ascontiguousarray(region, np.int32)
        self.region_run = np.ascontiguousarray(region_run, np.int32)
        self.region_keys = region_keys

    @property
    def n(self):
        return len(self.rec)


def whole_file_stream(records):
    n = records.n
    return Stream(np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.zeros(1, np.int32), None)


def bed_stream(records, refs, bedfile, block=None):
    """The stream over the bed regions in file order (block = (lo, hi): only regions lo <= r < hi, a
    rank's block), built natively (ccio_region_stream)."""
    regions = region_list(bedfile)
    names = {name: i for i, (name, _) in enumerate(refs)}
    for _, chrom, _, _ in regions:
        if chrom not in names:
            raise ValueError("invalid contig `%s`" % chrom)   # pysam fetch on an unknown contig
    n = records.n
    tid = np.ascontiguousarray(records.tid[:n], np.int32)
    pos = np.ascontiguousarray(records.pos[:n], np.int32)
    rt = np.array([names[c] for _, c, _, _ in regions] or [0], np.int32)
    rb = np.array([s for _, _, s, _ in regions] or [0], np.int64)
    re_ = np.array([e for _, _, _, e in regions] or [0], np.int64)
    lo, hi = (0, len(regions)) if block is None else (int(block[0]), int(block[1]))
    io = N.io()
    k = io.ccio_region_stream(n, N.ptr(tid), N.ptr(pos), lo, hi, N.ptr(rt), N.ptr(rb), N.ptr(re_), None, None)
    if k < 0:
        raise ValueError(N.io_error())
    rec = np.zeros(max(int(k), 1), np.int32)
    reg = np.zeros(max(int(k), 1), np.int32)
    io.ccio_region_stream(n, N.ptr(tid), N.ptr(pos), lo, hi, N.ptr(rt), N.ptr(rb), N.ptr(re_), N.ptr(rec), N.ptr(reg))
    return Stream(rec[:k], reg[:k], np.array(region_runs(regions), np.int32), [x[0] for x in regions])


def coord_sorted(records):
    """True when records are in (tid, pos) order with unmapped (tid -1) last: position groups are
    then contiguous and the engine groups tags per position group instead of a global sort."""
    if not hasattr(records, "_coord_sorted"):
        n = records.n
        tid = records.tid[:n].astype(np.int64)
        key = np.where(tid < 0, np.int64(1) << 62, (tid << 32) + records.pos[:n].astype(np.int64))
        records._coord_sorted = bool(n < 2 or np.all(key[1:] >= key[:-1]))
    return records._coord_sorted


_BGZF_OWNER = None   # the engine whose encoder libccio's (process-wide) deflate hook points at
_INFLATE_OWNER = None   # likewise for the inflate hook
_KEEP_OWNER = None   # and for the inflate hook that keeps resident streams
_ASSEMBLE_OWNER = None   # and for the assemble hook
_OUT_RESIDENT_OWNER = None   # and for the resident output set
_MERGE_OWNER = None   # and for the merge hooks


class Engine(object):
    """One HIP context on one GPU (cc_ctx)."""

    def __init__(self, device=0):
        self.lib = N.amd()
        h = N.P()
        rc = self.lib.cc_create(int(device), C.byref(h))
        if rc != 0:
            raise N.CCError(rc, "cc_create failed (no usable GPU?)")
        self.h = h
        self.tables = {}
        self.bgzf_device = False
        self._bgzf_effort = 1
        self.inflate_device = False
        self.decode_device = False
        self.resident_device = False
        self.ids_device = False
        self._keep_wired = False
        self.crc_device = False
        self.assemble_device = False
        self.merge_device = False
        self.out_resident_device = False   # the resident output set is wired (device_out_resident)
        self._out_resident_want = os.environ.get("CC_OUT_RESIDENT_DEVICE") == "1"
        self.names_device = os.environ.get("CC_NAMES_DEVICE") == "1"
        self._names_resident_want = os.environ.get("CC_NAMES_RESIDENT_DEVICE") == "1"
        if os.environ.get("CC_CRC_DEVICE") == "1":   # before the hooks below are wired: they take the crc variants
            self.device_crc(True)
        if os.environ.get("CC_RESIDENT_DEVICE") == "1":
            self.device_resident(True)
        if os.environ.get("CC_BGZF_EFFORT"):   # the encoder's effort, for CC_BGZF_DEVICE and bgzf_deflate alike
            self._set_bgzf_effort(os.environ["CC_BGZF_EFFORT"])
        if os.environ.get("CC_BGZF_DEVICE") == "1":   # opt-in, in the style of CC_EXTRACT_GPU
            self.device_bgzf(True)
        if os.environ.get("CC_INFLATE_DEVICE") == "1":
            self.device_inflate(True)
        if os.environ.get("CC_DECODE_DEVICE") == "1":
            self.device_decode(True)
        if os.environ.get("CC_IDS_DEVICE") == "1":
            self.device_ids(True)
        if os.environ.get("CC_ASSEMBLE_DEVICE") == "1":
            self.device_assemble(True)
        if os.environ.get("CC_MERGE_DEVICE") == "1":
            self.device_merge(True)
        self._sync_out_resident()

    def device_decode(self, on):
        """Switches table() between the host decoder (Bam.decode + upload, the default) and the device
        record unpacker (unpack: Bam.decode_ids + cc_table_unpack).  The tables, and every file
        written from them, are the same either way.  A per-engine switch (no process-wide hook).
        Returns the previous state."""
        was = self.decode_device
        self.decode_device = bool(on)
        self._sync_keep()
        return was

    def device_ids(self, on):
        """Switches unpack between libccio's string pass (Bam.decode_ids, the default) and the device
        interner: Bam.decode_cols, cc_table_ids over the raw records (the resident stream when there is
        one) and Bam.intern_first for the distinct strings only.  It has effect only while
        device_decode is on.  A file the device interner refuses (CC_E_INVALID, CC_E_COLLISION,
        CC_E_UNSUPPORTED) goes through the host pass.  The ids, the tables and every file written from
        them are the same either way.  Returns the previous state."""
        was = self.ids_device
        self.ids_device = bool(on)
        return was

    def device_resident(self, on):
        """Switches the resident path on or off (off is the default): a whole-file open leaves the
        bytes the device inflater produced in a device buffer (cc_bgzf_inflate_keep), and unpack has
        cc_table_unpack_resident read the records there instead of uploading them again.  It has
        effect only together with device_inflate and device_decode: while either is off nothing is
        wired, no resident stream is made and every path is as without the switch (no error is
        raised).  The tables, and every file written from them, are the same either way.  Returns
        the previous state."""
        was = self.resident_device
        self.resident_device = bool(on)
        self._sync_keep()
        return was

    def _sync_keep(self, rewire=False):
        """libccio's keep hook (cc_bgzf_inflate_keep_hook -> ccio_set_inflate_keep_hook) wired exactly
        while this engine has device_inflate, device_decode and device_resident on, with the inflate
        hook's one-owner rules.  While device_crc is on the hook wired is its crc variant
        (cc_bgzf_inflate_keep_crc_hook -> ccio_set_inflate_keep_crc_hook); rewire: the variant changed."""
        global _KEEP_OWNER
        want = bool(self.h) and self.inflate_device and self.decode_device and self.resident_device
        if want == self._keep_wired and not (rewire and want):
            return
        io = N.io()
        if want:
            keep, patch, user = N.P(), N.P(), N.P()
            get = self.lib.cc_bgzf_inflate_keep_crc_hook if self.crc_device else self.lib.cc_bgzf_inflate_keep_hook
            self._check(get(self.h, C.byref(keep), C.byref(patch), C.byref(user)))
            prev = _KEEP_OWNER
            if prev is not None and prev is not self:
                prev._keep_wired = False
            if self.crc_device:   # one variant at a time: the other is the previous owner's, or this engine's old one
                io.ccio_set_inflate_keep_crc_hook(keep, patch, user)
                io.ccio_set_inflate_keep_hook(None, None, None)
            else:
                io.ccio_set_inflate_keep_hook(keep, patch, user)
                io.ccio_set_inflate_keep_crc_hook(None, None, None)
            _KEEP_OWNER = self
            self._keep_wired = True
            return
        io.ccio_set_inflate_keep_hook(None, None, None)
        io.ccio_set_inflate_keep_crc_hook(None, None, None)
        _KEEP_OWNER = None
        self._keep_wired = False

    def _wire_inflate(self):
        """This engine's inflate hook handed to libccio: the plain one, or with device_crc on its crc
        variant (cc_bgzf_inflate_crc_hook -> ccio_set_inflate_crc_hook); the other variant is unset."""
        io = N.io()
        fn, user = N.P(), N.P()
        get = self.lib.cc_bgzf_inflate_crc_hook if self.crc_device else self.lib.cc_bgzf_inflate_hook
        self._check(get(self.h, C.byref(fn), C.byref(user)))
        if self.crc_device:
            io.ccio_set_inflate_crc_hook(fn, user)
            io.ccio_set_inflate_hook(None, None)
        else:
            io.ccio_set_inflate_hook(fn, user)
            io.ccio_set_inflate_crc_hook(None, None)

    def device_crc(self, on):
        """Switches the device CRC32 (k_crc32) on or off (off is the default) for both BGZF directions.
        While it is on, device_inflate and the resident path wire the crc variants of their hooks:
        the device reports each member's CRC32 over the bytes it wrote (with a resident stream, the
        bytes the unpacker reads) and libccio compares that with the member's field instead of
        computing a CRC over the downloaded copy; and the device encoder (device_bgzf, bgzf_deflate)
        takes its members' CRC32 fields from the device input buffer (cc_bgzf_set_crc) instead of
        the calling thread.  The bytes read and the members written are the same either way.
        Toggling while hooks are wired re-wires them; with device_bgzf on it first waits for the
        background writes.  Without device_inflate or device_bgzf it has no effect and raises nothing.
        A per-engine switch.  Returns the previous state."""
        was = self.crc_device
        on = bool(on)
        if on == was:
            return was
        if self.bgzf_device and N.io().ccio_flush() != 0:   # a file's CRC fields come from one place throughout
            raise IOError(N.io_error())
        self._check(self.lib.cc_bgzf_set_crc(self.h, int(on)))
        self.crc_device = on
        if self.inflate_device:
            self._wire_inflate()
        self._sync_keep(rewire=True)
        return was

    @property
    def bgzf_effort(self):
        """The device BGZF encoder's effort (cc_bgzf_set_effort): 1 or 2."""
        return self._bgzf_effort

    def _set_bgzf_effort(self, effort):
        """cc_bgzf_set_effort; returns the previous effort.  ValueError for anything but 1 or 2."""
        was = self._bgzf_effort
        try:
            effort = int(effort)
        except (TypeError, ValueError):
            raise ValueError("bgzf effort must be 1 or 2")
        if effort not in (1, 2):
            raise ValueError("bgzf effort must be 1 or 2")
        self._check(self.lib.cc_bgzf_set_effort(self.h, effort))
        self._bgzf_effort = effort
        return was

    def device_bgzf(self, on, effort=None):
        """Wires (or unwires) this context's device BGZF encoder into libccio's writers
        (cc_bgzf_hook -> ccio_set_deflate_hook): every BAM written at level >= 1 from now on is
        deflated by k_bgzf_deflate instead of the host codec.  The records are the same either way;
        the compressed bytes and the .bai virtual offsets differ.  The hook is one per process: the
        last engine to wire it serves the writers, and the engine it took the hook from reads
        bgzf_device False from then on (its close or unwiring leaves the new owner's hook alone).
        Wiring and unwiring wait for the background writes first, so a file is encoded by one
        encoder throughout.  effort (1 or 2; None leaves it as it is) is the encoder's effort from
        now on, for the writers and for bgzf_deflate; a change while the hook is wired waits for the
        background writes first.  Returns the previous state."""
        global _BGZF_OWNER
        was = self.bgzf_device
        on = bool(on)
        if effort is not None:
            if int(effort) not in (1, 2):
                raise ValueError("bgzf effort must be 1 or 2")
            if was and int(effort) != self._bgzf_effort:
                if N.io().ccio_flush() != 0:   # a file is encoded at one effort throughout
                    raise IOError(N.io_error())
            self._set_bgzf_effort(effort)
        if on == was:
            return was
        io = N.io()
        if on:
            fn, user = N.P(), N.P()
            self._check(self.lib.cc_bgzf_hook(self.h, C.byref(fn), C.byref(user)))
            prev = _BGZF_OWNER
            if prev is not None and prev is not self:
                rc = io.ccio_flush()   # no writer thread is inside the previous owner's encoder
                prev.bgzf_device = False
                prev._sync_out_resident()
                if rc != 0:
                    raise IOError(N.io_error())
            io.ccio_set_deflate_hook(fn, user)
            _BGZF_OWNER = self
            self.bgzf_device = True
            self._sync_out_resident()
            return was
        rc = io.ccio_flush()   # no writer thread is inside the hook after this
        io.ccio_set_deflate_hook(None, None)
        _BGZF_OWNER = None
        self.bgzf_device = False
        self._sync_out_resident()
        if rc != 0:
            raise IOError(N.io_error())
        return was

    def device_assemble(self, on):
        """Wires (or unwires) this context's device record assembler into libccio's stage writer
        (cc_bam_assemble_hook -> ccio_set_assemble_hook): every write_bam from now on whose sources
        hold their records in place has its stream assembled by k_asm_sizes / k_asm_copy; libccio
        checks the result and assembles whatever the device refused on the host, so the files are the
        same either way.  The hook is one per process, with device_bgzf's ownership rules: the last
        engine to wire it serves the writer, and the engine it took the hook from reads
        assemble_device False from then on.  Assembly is synchronous, so there is nothing to wait
        for.  Returns the previous state."""
        global _ASSEMBLE_OWNER
        was = self.assemble_device
        on = bool(on)
        if on == was:
            return was
        io = N.io()
        if on:
            fn, user = N.P(), N.P()
            self._check(self.lib.cc_bam_assemble_hook(self.h, C.byref(fn), C.byref(user)))
            prev = _ASSEMBLE_OWNER
            if prev is not None and prev is not self:
                prev.assemble_device = False
                prev._sync_out_resident()
            io.ccio_set_assemble_hook(fn, user)
            _ASSEMBLE_OWNER = self
            self.assemble_device = True
            self._sync_out_resident()
            return was
        io.ccio_set_assemble_hook(None, None)
        _ASSEMBLE_OWNER = None
        self.assemble_device = False
        self._sync_out_resident()
        return was

    def device_merge(self, on):
        """Wires (or unwires) this context's device merge into libccio's merges (cc_bam_merge_hooks ->
        ccio_set_merge_hooks): every merge_kept from now on whose inputs hold their records in place,
        are at most 8 and are each in key order is built by k_merge_keys / k_merge_rank / k_merge_copy
        (with the resident output path on, the stream stays on the device for the encoder and the
        index); libccio checks the result and merges whatever the device refused on the host, so the
        files are the same either way.  The hooks are one pair per process, with device_assemble's
        ownership rules: the last engine to wire them serves the merges, and the engine it took them
        from reads merge_device False from then on.  The merge is synchronous, so there is nothing to
        wait for.  Returns the previous state."""
        global _MERGE_OWNER
        was = self.merge_device
        on = bool(on)
        if on == was:
            return was
        io = N.io()
        if on:
            fn, keep, user = N.P(), N.P(), N.P()
            self._check(self.lib.cc_bam_merge_hooks(self.h, C.byref(fn), C.byref(keep), C.byref(user)))
            prev = _MERGE_OWNER
            if prev is not None and prev is not self:
                prev.merge_device = False
            io.ccio_set_merge_hooks(fn, keep, user)
            _MERGE_OWNER = self
            self.merge_device = True
            return was
        io.ccio_set_merge_hooks(None, None, None)
        _MERGE_OWNER = None
        self.merge_device = False
        return was

    def device_out_resident(self, on):
        """Asks for (or gives up) the resident output path (cc_out_resident_hooks -> ccio_set_out_resident):
        write_bam's assembled stream stays on the device, the encoder reads its pieces there
        (cc_bgzf_deflate_resident) and the .bai comes from k_index_fields, so a file nobody keeps in
        memory never crosses PCIe uncompressed.  The files are byte for byte those of assemble_device
        with bgzf_device.  Effective only while assemble_device and bgzf_device are both on: otherwise
        nothing is wired and nothing raises, and the set is wired once both are (out_resident_device
        says whether it is).  One set per process, with device_bgzf's ownership rules.  Wiring and
        unwiring wait for the background writes first.  Returns the previous request."""
        was = self._out_resident_want
        self._out_resident_want = bool(on)
        self._sync_out_resident()
        return was

    def _sync_out_resident(self):
        global _OUT_RESIDENT_OWNER
        want = bool(self._out_resident_want and self.assemble_device and self.bgzf_device and self.h)
        if want == self.out_resident_device:
            return
        io = N.io()
        rc = io.ccio_flush()   # no writer thread is inside the set (or the previous owner's) after this
        if want:
            cb, user = N.ccio_out_resident(), N.P()
            self._check(self.lib.cc_out_resident_hooks(self.h, C.byref(cb), C.byref(user)))
            prev = _OUT_RESIDENT_OWNER
            if prev is not None and prev is not self:
                prev.out_resident_device = False
            io.ccio_set_out_resident(C.byref(cb), user)
            _OUT_RESIDENT_OWNER = self
            self.out_resident_device = True
        else:
            if _OUT_RESIDENT_OWNER is self:
                io.ccio_set_out_resident(None, None)
                _OUT_RESIDENT_OWNER = None
            self.out_resident_device = False
        if rc != 0:
            raise IOError(N.io_error())

    def resident_put(self, data):
        """cc_resident_put: data (bytes-like or a uint8 array) uploaded as a resident stream; its id."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        buf = np.ascontiguousarray(buf, np.uint8)
        rid = C.c_int64(0)
        self._check(self.lib.cc_resident_put(self.h, N.ptr(buf) if buf.size else None, buf.size, C.byref(rid)))
        return int(rid.value)

    def resident_free(self, rid):
        self._check(self.lib.cc_resident_free(self.h, int(rid)))

    def resident_count(self):
        return int(self.lib.cc_resident_count(self.h))

    def resident_fetch(self, rid):
        """A resident stream's bytes (cc_resident_fetch)."""
        total = int(self.lib.cc_resident_fetch(self.h, int(rid), None, 0))
        if total < 0:
            self._check(total)
        out = np.zeros(max(total, 1), np.uint8)
        got = int(self.lib.cc_resident_fetch(self.h, int(rid), N.ptr(out), total))
        if got < 0:
            self._check(got)
        return out[:total].tobytes()

    def bgzf_deflate_resident(self, token, off, n, effort=None):
        """cc_bgzf_deflate_resident: the framed BGZF members of bytes [off, off + n) of resident stream
        `token`, as bgzf_deflate returns them."""
        if effort is not None:
            was = self._set_bgzf_effort(effort)
            try:
                return self.bgzf_deflate_resident(token, off, n)
            finally:
                self._set_bgzf_effort(was)
        pieces = (int(n) + 0xff00 - 1) // 0xff00
        slot = 0x10000
        stage = np.zeros(max(pieces, 1) * slot, np.uint8)
        lens = np.zeros(max(pieces, 1), np.uint32)
        got = int(self.lib.cc_bgzf_deflate_resident(self.h, int(token), int(off), int(n), N.ptr(stage), slot,
                                                    N.ptr(lens), pieces))
        if got < 0:
            raise N.CCError(got, self.lib.cc_last_error(self.h).decode(errors="replace"))
        return [stage[j * slot:j * slot + int(lens[j])].tobytes() for j in range(got)]

    def index_fields(self, token, at):
        """cc_index_fields: one N.INDEX_FIELD_DTYPE row per record of resident stream `token`, record i
        at byte at[i] (len(at) - 1 records)."""
        at = np.ascontiguousarray(at, np.uint64)
        n = len(at) - 1
        out = np.zeros(max(n, 1), N.INDEX_FIELD_DTYPE)
        self._check(self.lib.cc_index_fields(self.h, int(token), N.ptr(at), n, N.ptr(out)))
        return out[:n]

    def pin_source(self, bam):
        """A context manager: bam's stream (a handle whose records lie in place) uploaded once as a
        resident stream and named to the assemble hooks (ccio_bam_set_resident), so that every write
        from it inside the block reads that copy instead of uploading the stream again.  On exit the
        background writes are waited for, the name is cleared and the stream freed.  A handle that
        already names a resident copy, or whose records do not lie in place, is left as it is."""
        return _PinnedSource(self, bam)

    def device_names(self, on):
        """Switches the stages' consensus read names between libccio's formatters (csn_names / dcs_names,
        the default) and the device formatter (Engine.csn_names / Engine.dcs_names: k_name_sizes_* and
        k_name_write_*).  The names, and every file written with them, are the same either way.  A
        per-engine switch (no process-wide hook).  Returns the previous state."""
        was = self.names_device
        self.names_device = bool(on)
        return was

    def device_names_resident(self, on):
        """Asks for (or gives up) resident names (off is the default): the stages keep the blob the device
        formatter wrote on the device as a name set (cc_names_keep) that the device assembler reads in
        place (write_bam: names_dev), and the SSCS stage formats its names from the group's own
        emit_ckey / emit_n (csn_names_group), so neither the blob nor those fields cross the bus.  The
        files are the same either way.  Effective only while names_device and assemble_device are both
        on (names_resident_device says whether it is); otherwise it has no effect and raises nothing.
        A per-engine switch.  Returns the previous request."""
        was = self._names_resident_want
        self._names_resident_want = bool(on)
        return was

    @property
    def names_resident_device(self):
        return bool(self._names_resident_want and self.names_device and self.assemble_device and self.h)

    def _names_blob(self, n, off, total, keep=False):
        if keep:
            nid = C.c_int64(0)
            self._check(self.lib.cc_names_keep(self.h, C.byref(nid)))
            return KeptNames(nid.value), off
        blob = np.zeros(max(int(total), 1), np.uint8)
        self._check(self.lib.cc_names_read(self.h, N.ptr(blob), int(total)))
        return blob, off

    def names_fetch(self, names_id):
        """A name set's blob (cc_names_fetch) as a uint8 array; the set stays as it is."""
        total = int(self.lib.cc_names_fetch(self.h, int(names_id), None, 0))
        if total < 0:
            self._check(total)
        blob = np.zeros(max(total, 1), np.uint8)
        got = int(self.lib.cc_names_fetch(self.h, int(names_id), N.ptr(blob), total))
        if got < 0:
            self._check(got)
        return blob

    def names_free(self, names_id):
        self._check(self.lib.cc_names_free(self.h, int(names_id)))

    def names_count(self):
        return int(self.lib.cc_names_count(self.h))

    def csn_names_group(self, group, interner, keep=False):
        """The SSCS stage's names from the group's own buffers (cc_format_csn_names_group): what
        csn_names(interner, repeat(fetch(emit_ckey), 2), fetch(emit_n)) gives, without fetching or
        uploading either array.  The result is csn_names': (blob, off), or with keep=True
        (KeptNames, off); what the device refuses or does not support goes to the host function over
        the fetched arrays and comes back as (blob, off)."""
        bc, bc_off = interner.blob(0)
        cg, cg_off = interner.blob(1)
        n = self._used(group, "emit_n") // 4
        off = np.zeros(n + 1, np.int64)
        total = C.c_int64(0)
        rc = self.lib.cc_format_csn_names_group(self.h, int(group), N.ptr(bc), N.ptr(bc_off), len(bc_off) - 1, N.ptr(cg),
                                                N.ptr(cg_off), len(cg_off) - 1, N.ptr(off), C.byref(total))
        if rc in (N.CC_E_INVALID, N.CC_E_UNSUPPORTED):
            ckey = np.repeat(self.fetch(group, "emit_ckey", np.int32).reshape(-1, 9), 2, axis=0).reshape(-1)
            return csn_names(interner, ckey, self.fetch(group, "emit_n", np.int32))
        self._check(rc)
        return self._names_blob(n, off, total.value, keep)

    def _used(self, group, name):
        """A group buffer's bytes in use (cc_fetch's size query)."""
        nb = int(self.lib.cc_fetch(self.h, group, name.encode(), None, 0))
        if nb < 0:
            raise N.CCError(nb, self.lib.cc_last_error(self.h).decode())
        return nb

    def csn_names(self, interner, ckey9, suffix, keep=False):
        """csn_names on the device (cc_format_csn_names): the same (blob, off).  What the device refuses
        (an id outside its table) or does not support goes to the host function, which raises what
        it always raised.  keep=True leaves the blob on the device as a name set (cc_names_keep) and
        returns (KeptNames, off): KeptNames is the set's id (an int subclass) for names_fetch,
        names_free, assemble(names_id=) and write_bam(names_dev=).  When the host function ran instead
        the result is the ordinary (blob, off) whatever keep says, so a caller that keeps tells the
        two by isinstance(result[0], KeptNames)."""
        n = len(suffix)
        ck = np.ascontiguousarray(ckey9, np.int32).reshape(-1)
        sf = np.ascontiguousarray(suffix, np.int64)
        if len(ck) != 9 * n:
            raise ValueError("csn_names: nine fields per name")
        bc, bc_off = interner.blob(0)
        cg, cg_off = interner.blob(1)
        off = np.zeros(n + 1, np.int64)
        total = C.c_int64(0)
        rc = self.lib.cc_format_csn_names(self.h, n, N.ptr(ck), N.ptr(sf), N.ptr(bc), N.ptr(bc_off), len(bc_off) - 1,
                                          N.ptr(cg), N.ptr(cg_off), len(cg_off) - 1, N.ptr(off), C.byref(total))
        if rc in (N.CC_E_INVALID, N.CC_E_UNSUPPORTED):
            return csn_names(interner, ckey9, suffix)
        self._check(rc)
        return self._names_blob(n, off, total.value, keep)

    def dcs_names(self, bam, table, rec_tag, rec_ds, keep=False):
        """dcs_names on the device (cc_format_dcs_names) from `table`, the record table built from bam:
        the same (blob, off).  Names with a NUL inside (ccio_dcs_names_plain: the table keeps them up to
        it), whatever the device refuses (the reference's IndexError) and what it does not support go
        to the host function, which raises what it always raised.  keep: as for csn_names."""
        n = len(rec_tag)
        a = np.ascontiguousarray(rec_tag, np.int64)
        b = np.ascontiguousarray(rec_ds, np.int64)
        if N.io().ccio_dcs_names_plain(bam.h, n, N.ptr(a), N.ptr(b)) != 1:
            return dcs_names(bam, rec_tag, rec_ds)
        off = np.zeros(n + 1, np.int64)
        total = C.c_int64(0)
        rc = self.lib.cc_format_dcs_names(self.h, int(table), n, N.ptr(a), N.ptr(b), N.ptr(off), C.byref(total))
        if rc in (N.CC_E_INVALID, N.CC_E_UNSUPPORTED):
            return dcs_names(bam, rec_tag, rec_ds)
        self._check(rc)
        return self._names_blob(n, off, total.value, keep)

    def assemble(self, header, sources, specs, names=None, name_off=None, cons_seq=None, cons_qual=None, group=None,
                 rg_values=(), sort=False, keep=False, names_id=None):
        """cc_bam_assemble: the output stream (header bytes, then the records of `specs`) and its
        n + 1 record offsets, as (bytes, uint64 array).  sources: per source (stream, rec_off) with the
        records' bytes and offsets in host memory, or (None, rec_off, resident id, base, nbytes) for a
        resident stream.  The consensus arrays are cons_seq / cons_qual, or group's device buffers.
        rg_values: the RG table's values (bytes), by rg_id.  sort: samtools-sort order.  keep=True is
        cc_bam_assemble_keep without a download: (at, token), the stream left on the device as resident
        stream `token` (resident_fetch, bgzf_deflate_resident, index_fields; resident_free when done).
        names_id, in place of names: a name set (csn_names / dcs_names with keep=True) read where it
        lies (cc_bam_assemble_names, selected for this call only); name_off (the set's off, or a prefix
        of it) then says how many names and bytes of the set the specs may use."""
        if names_id is not None:
            if names is not None:
                raise ValueError("assemble: names or names_id, not both")
            self._check(self.lib.cc_bam_assemble_names(self.h, int(names_id)))
            try:
                return self._assemble(header, sources, specs, None, name_off, cons_seq, cons_qual, group, rg_values, sort,
                                      keep, True)
            finally:
                self.lib.cc_bam_assemble_names(self.h, 0)
        return self._assemble(header, sources, specs, names, name_off, cons_seq, cons_qual, group, rg_values, sort, keep,
                              False)

    @staticmethod
    def _asm_sources(sources):
        """assemble's / merge's sources as a cc_asm_src array, and the arrays it points into."""
        arr = (N.cc_asm_src * max(len(sources), 1))()
        hold = []
        for f, src in enumerate(sources):
            off = np.ascontiguousarray(src[1], np.uint64)
            hold.append(off)
            if src[0] is None:
                arr[f] = N.cc_asm_src(None, int(src[4]), int(src[2]), int(src[3]), off.ctypes.data, len(off))
            else:
                st = np.frombuffer(bytes(src[0]), np.uint8) if not isinstance(src[0], np.ndarray) else \
                    np.ascontiguousarray(src[0], np.uint8)
                hold.append(st)
                arr[f] = N.cc_asm_src(st.ctypes.data if len(st) else None, len(st), 0, 0, off.ctypes.data, len(off))
        return arr, hold

    def merge(self, header, sources, keep=False):
        """cc_bam_merge: the merge of `sources` (assemble's sources, at most 8, each in key order) as
        (stream bytes, at, org): the header's bytes then every record in key order, ties to the earlier
        source then the earlier record; at the n + 1 record offsets (uint64), org each output record's
        index in the concatenation of the sources (uint32).  keep=True is cc_bam_merge_keep without a
        download: (at, org, token), the stream left on the device as resident stream `token`
        (resident_fetch, bgzf_deflate_resident, index_fields; resident_free when done)."""
        header = np.frombuffer(bytes(header), np.uint8)
        arr, hold = self._asm_sources(sources)
        n = sum(len(src[1]) for src in sources)
        at = np.zeros(n + 1, np.uint64)
        org = np.zeros(max(n, 1), np.uint32)
        total = C.c_uint64()
        hp = N.ptr(header) if len(header) else None
        if keep:
            rid = C.c_int64(0)
            self._check(self.lib.cc_bam_merge_keep(self.h, hp, len(header), arr, len(sources), None, 0, N.ptr(at),
                                                   N.ptr(org), C.byref(total), C.byref(rid)))
            return at, org[:n], int(rid.value)
        self._check(self.lib.cc_bam_merge(self.h, hp, len(header), arr, len(sources), None, 0, None, None,
                                          C.byref(total)))
        out = np.zeros(max(int(total.value), 1), np.uint8)
        self._check(self.lib.cc_bam_merge(self.h, hp, len(header), arr, len(sources), N.ptr(out), int(total.value),
                                          N.ptr(at), N.ptr(org), C.byref(total)))
        return out[:int(total.value)].tobytes(), at, org[:n]

    def _assemble(self, header, sources, specs, names, name_off, cons_seq, cons_qual, group, rg_values, sort, keep,
                  in_set):
        header = np.frombuffer(bytes(header), np.uint8)
        specs = np.ascontiguousarray(specs, N.OUT_SPEC_DTYPE)
        n = len(specs)
        arr, hold = self._asm_sources(sources)
        names = np.zeros(0, np.uint8) if names is None else np.ascontiguousarray(names).view(np.uint8)
        name_off = np.zeros(1, np.int64) if name_off is None else np.ascontiguousarray(name_off, np.int64)
        names_bytes = int(name_off[-1]) if in_set else len(names)   # (a set: the bytes its first n_names names take)
        cs = np.zeros(0, np.uint8) if cons_seq is None else np.ascontiguousarray(cons_seq, np.uint8)
        cq = np.zeros(0, np.uint8) if cons_qual is None else np.ascontiguousarray(cons_qual, np.uint8)
        rg = [bytes(v) for v in rg_values]
        rg_off = np.zeros(len(rg) + 1, np.int64)
        rg_off[1:] = np.cumsum([len(v) for v in rg]) if rg else []
        rg_blob = np.frombuffer(b"".join(rg) + b"\0", np.uint8)

        def call(out, cap, at, total):
            return self.lib.cc_bam_assemble(
                self.h, N.ptr(header) if len(header) else None, len(header), arr, len(sources), N.ptr(specs), n,
                N.ptr(names) if len(names) else None, N.ptr(name_off), len(name_off) - 1, names_bytes,
                N.ptr(cs) if len(cs) else None, len(cs), N.ptr(cq) if len(cq) else None, len(cq),
                -1 if group is None else int(group), N.ptr(rg_blob), N.ptr(rg_off), len(rg), N.W_SORT if sort else 0,
                out, cap, at, total)
        total = C.c_uint64()
        if keep:
            at = np.zeros(n + 1, np.uint64)
            rid = C.c_int64(0)
            self._check(self.lib.cc_bam_assemble_keep(
                self.h, N.ptr(header) if len(header) else None, len(header), arr, len(sources), N.ptr(specs), n,
                N.ptr(names) if len(names) else None, N.ptr(name_off), len(name_off) - 1, names_bytes,
                N.ptr(cs) if len(cs) else None, len(cs), N.ptr(cq) if len(cq) else None, len(cq),
                -1 if group is None else int(group), N.ptr(rg_blob), N.ptr(rg_off), len(rg), N.W_SORT if sort else 0,
                None, 0, N.ptr(at), C.byref(total), C.byref(rid)))
            return at, int(rid.value)
        self._check(call(None, 0, None, C.byref(total)))
        out = np.zeros(max(int(total.value), 1), np.uint8)
        at = np.zeros(n + 1, np.uint64)
        self._check(call(N.ptr(out), int(total.value), N.ptr(at), C.byref(total)))
        return out[:int(total.value)].tobytes(), at

    def device_inflate(self, on):
        """Wires (or unwires) this context's device BGZF inflater into libccio's readers
        (cc_bgzf_inflate_hook -> ccio_set_inflate_hook): every BAM opened from now on (whole file,
        regions, header) has its members inflated by k_bgzf_inflate first; libccio checks each
        member's CRC32 and inflates whatever the device refused, or got wrong, with the host codec,
        so the bytes read are the same either way.  The hook is one per process, with device_bgzf's
        ownership rules: the last engine to wire it serves the readers, the engine it took the hook
        from reads inflate_device False from then on, and that engine's close or unwiring leaves the
        new owner's hook alone.  Reads are synchronous, so there is nothing to wait for.  With
        device_decode and device_resident on as well, the hook that keeps resident streams is wired
        with it (and unwired with it).  With device_crc on, the hooks wired are their crc variants:
        the device reports each member's CRC32 and libccio compares it with the member's field.
        Returns the previous state."""
        global _INFLATE_OWNER
        was = self.inflate_device
        on = bool(on)
        if on == was:
            return was
        io = N.io()
        if on:
            prev = _INFLATE_OWNER
            if prev is not None and prev is not self:
                prev.inflate_device = False
                prev._sync_keep()
            self._wire_inflate()
            _INFLATE_OWNER = self
            self.inflate_device = True
            self._sync_keep()
            return was
        io.ccio_set_inflate_hook(None, None)
        io.ccio_set_inflate_crc_hook(None, None)
        _INFLATE_OWNER = None
        self.inflate_device = False
        self._sync_keep()
        return was

    def bgzf_inflate(self, raw, crc=False):
        """cc_bgzf_inflate over the bytes of a BGZF file or run of members: (data, ok_list), data the
        members' inflated bytes side by side (ISIZE bytes each; a refused member's are unspecified),
        ok_list one bool per member.  crc=True: cc_bgzf_inflate_crc, and (data, ok_list, crcs) with the
        device's CRC32 of every member's bytes (meaningful where ok)."""
        raw = bytes(raw)
        coff, clen, uoff, ulen = [], [], [], []
        off = total = 0
        while off < len(raw):
            if off + 18 > len(raw) or raw[off:off + 4] != b"\x1f\x8b\x08\x04":
                raise ValueError("not a BGZF member at byte %d" % off)
            xlen = int.from_bytes(raw[off + 10:off + 12], "little")
            x, bsize = off + 12, 0
            while x + 4 <= off + 12 + xlen and x + 4 <= len(raw):
                slen = int.from_bytes(raw[x + 2:x + 4], "little")
                if raw[x:x + 2] == b"BC" and slen == 2 and x + 6 <= len(raw):
                    bsize = int.from_bytes(raw[x + 4:x + 6], "little") + 1
                x += 4 + slen
            if bsize < 12 + xlen + 8 or off + bsize > len(raw):
                raise ValueError("BGZF member without BC field or truncated at byte %d" % off)
            isize = int.from_bytes(raw[off + bsize - 4:off + bsize], "little")
            coff.append(off + 12 + xlen)
            clen.append(bsize - 12 - xlen - 8)
            uoff.append(total)
            ulen.append(isize)
            total += isize
            off += bsize
        n = len(coff)
        comp = np.frombuffer(raw, np.uint8)
        out = np.zeros(max(total, 1), np.uint8)
        ok = np.zeros(max(n, 1), np.uint8)
        a = [np.asarray(v if n else [0], t) for v, t in ((coff, np.uint64), (clen, np.uint32), (uoff, np.uint64),
                                                         (ulen, np.uint32))]
        args = (self.h, N.ptr(comp) if comp.size else None, N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), N.ptr(a[3]), n,
                N.ptr(out), N.ptr(ok))
        crcs = np.zeros(max(n, 1), np.uint32)
        got = int(self.lib.cc_bgzf_inflate_crc(*(args + (N.ptr(crcs),))) if crc else self.lib.cc_bgzf_inflate(*args))
        if got < 0:
            raise N.CCError(got, self.lib.cc_last_error(self.h).decode(errors="replace"))
        if crc:
            return out[:total].tobytes(), [bool(v) for v in ok[:n]], [int(v) for v in crcs[:n]]
        return out[:total].tobytes(), [bool(v) for v in ok[:n]]

    @staticmethod
    def _ranges(ranges):
        if any(int(r[0]) < 0 or int(r[1]) < 0 for r in ranges):
            raise ValueError("a range is (offset, length), both >= 0")
        off = np.asarray([int(r[0]) for r in ranges] or [0], np.uint64)
        ln = np.asarray([int(r[1]) for r in ranges] or [0], np.uint64)
        return off, ln

    def crc32(self, data, ranges=None):
        """cc_crc32: the CRC32 (zlib's) of every (offset, length) range of data (bytes-like), computed by
        k_crc32, as a list of ints; ranges may overlap and be of any length.  ranges=None: the CRC of
        the whole buffer, a list of one."""
        buf = np.frombuffer(bytes(data), np.uint8)
        ranges = [(0, buf.size)] if ranges is None else list(ranges)
        off, ln = self._ranges(ranges)
        out = np.zeros(max(len(ranges), 1), np.uint32)
        self._check(self.lib.cc_crc32(self.h, N.ptr(buf) if buf.size else None, buf.size, N.ptr(off), N.ptr(ln),
                                      len(ranges), N.ptr(out)))
        return [int(v) for v in out[:len(ranges)]]

    def resident_crc32(self, rid, ranges):
        """cc_resident_crc32: the same over the bytes of resident stream rid, in place."""
        ranges = list(ranges)
        off, ln = self._ranges(ranges)
        out = np.zeros(max(len(ranges), 1), np.uint32)
        self._check(self.lib.cc_resident_crc32(self.h, int(rid), N.ptr(off), N.ptr(ln), len(ranges), N.ptr(out)))
        return [int(v) for v in out[:len(ranges)]]

    def bgzf_deflate(self, data, effort=None):
        """cc_bgzf_deflate: the framed BGZF members of data (bytes-like), one per 0xff00-byte piece,
        as a list of bytes objects.  effort (1 or 2) holds for this call only; None encodes at the
        engine's effort."""
        if effort is not None:
            was = self._set_bgzf_effort(effort)
            try:
                return self.bgzf_deflate(data)
            finally:
                self._set_bgzf_effort(was)
        buf = np.frombuffer(bytes(data), np.uint8)
        pieces = (buf.size + 0xff00 - 1) // 0xff00
        slot = 0x10000
        stage = np.zeros(max(pieces, 1) * slot, np.uint8)
        lens = np.zeros(max(pieces, 1), np.uint32)
        got = int(self.lib.cc_bgzf_deflate(self.h, N.ptr(buf) if buf.size else None, buf.size, N.ptr(stage), slot,
                                           N.ptr(lens), pieces))
        if got < 0:
            raise N.CCError(got, self.lib.cc_last_error(self.h).decode(errors="replace"))
        return [stage[j * slot:j * slot + int(lens[j])].tobytes() for j in range(got)]

    def close(self):
        if self.h:
            try:
                self.device_resident(False)   # the hooks must not outlive the context; the resident streams
                self.device_inflate(False)    # that are left go with it (cc_destroy)
                self.device_bgzf(False)
                self.device_assemble(False)   # (the resident output set goes with either of the two)
                self.device_merge(False)
            finally:
                self.lib.cc_destroy(self.h)
                self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise N.CCError(rc, self.lib.cc_last_error(self.h).decode(errors="replace"))

    def table_column(self, table, name, dtype):
        """A table's derived column (cc_table_fetch: rkey, meta, core, qn_ol, qdig, rdeep, dlist, ext)."""
        nb = int(self.lib.cc_table_fetch(self.h, table, name.encode(), None, 0))
        if nb < 0:
            raise N.CCError(nb, self.lib.cc_last_error(self.h).decode(errors="replace"))
        out = np.zeros(max(nb, 1), np.uint8)
        nb = int(self.lib.cc_table_fetch(self.h, table, name.encode(), N.ptr(out), out.nbytes))
        if nb < 0:
            raise N.CCError(nb, self.lib.cc_last_error(self.h).decode(errors="replace"))
        return out[:nb].view(dtype)

    def debug_scan(self, kind, engine, values, aux=None):
        """The engine's scan on `values` (cc_debug_scan; kind 0: uint32 values, kinds 1-3: uint8 0/1 flags;
        engine 0 reduce-then-scan, 1 look-back, -1 the default; aux: kind 3's t_rec, p_rec, dec as 3 * n
        int32).  Returns (out_a, out_b, total) WITH the 64 canary elements behind each array: out_a is
        uint32 prefix[n + 64] (kinds 0, 1) or int32 vslot[n + 64]; out_b is None, int32 list[n + 64]
        (kind 2) or int32 vpair[n + 64, 4] (kind 3), written up to `total`."""
        values = np.ascontiguousarray(values, np.uint32 if kind == 0 else np.uint8)
        n = len(values)
        out_a = np.zeros(n + 64, np.uint32 if kind < 2 else np.int32)
        out_b = None if kind < 2 else np.zeros(n + 64 if kind == 2 else (n + 64, 4), np.int32)
        if aux is not None:
            aux = np.ascontiguousarray(aux, np.int32)
            assert aux.size == 3 * n
        total = C.c_int64(-1)
        self._check(self.lib.cc_debug_scan(self.h, int(kind), int(engine), N.ptr(values), n, N.ptr(aux), N.ptr(out_a),
                                           N.ptr(out_b), C.byref(total)))
        return out_a, out_b, total.value

    def debug_sort_pairs(self, engine, keys, vals, begin_bit=0, end_bit=64):
        """The engine's radix sort on (uint64 key, uint32 value) pairs (cc_debug_sort_pairs; engine: the
        digit scans' engine, as for debug_scan).  Returns (keys, vals) WITH 64 canary elements behind."""
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.uint32)
        n = len(keys)
        assert len(vals) == n
        out_k = np.zeros(n + 64, np.uint64)
        out_v = np.zeros(n + 64, np.uint32)
        self._check(self.lib.cc_debug_sort_pairs(self.h, int(engine), N.ptr(keys), N.ptr(vals), n, int(begin_bit),
                                                 int(end_bit), N.ptr(out_k), N.ptr(out_v)))
        return out_k, out_v

    def upload(self, records):
        tid = C.c_int32()
        self._check(self.lib.cc_table_upload(self.h, C.byref(records.struct), records.max_len, C.byref(tid)))
        self.tables[tid.value] = records
        return tid.value

    def unpack_raw(self, stream, rec_off, cigar_id, bc_id, rg_id, rflags):
        """cc_table_unpack on caller-given arrays: (table id, max_len).  The table is not registered
        with a Records (free it with free_table)."""
        stream = np.ascontiguousarray(stream, np.uint8)
        off = np.ascontiguousarray(rec_off, np.uint64)
        n = len(off)
        cols = [np.ascontiguousarray(a, t) for a, t in ((cigar_id, np.int32), (bc_id, np.int32), (rg_id, np.int32),
                                                        (rflags, np.uint8))]
        assert all(len(c) >= n for c in cols)
        ml, tid = C.c_int32(), C.c_int32()
        self._check(self.lib.cc_table_unpack(self.h, N.ptr(stream) if stream.size else None, stream.size,
                                             N.ptr(off) if n else None, n, N.ptr(cols[0]), N.ptr(cols[1]), N.ptr(cols[2]),
                                             N.ptr(cols[3]), C.byref(ml), C.byref(tid)))
        return tid.value, ml.value

    def unpack_resident(self, rid, base, nbytes, rec_off, cigar_id, bc_id, rg_id, rflags):
        """cc_table_unpack_resident on caller-given arrays: unpack_raw with the records read from bytes
        [base, base + nbytes) of resident stream rid.  The stream is not freed."""
        off = np.ascontiguousarray(rec_off, np.uint64)
        n = len(off)
        cols = [np.ascontiguousarray(a, t) for a, t in ((cigar_id, np.int32), (bc_id, np.int32), (rg_id, np.int32),
                                                        (rflags, np.uint8))]
        assert all(len(c) >= n for c in cols)
        ml, tid = C.c_int32(), C.c_int32()
        self._check(self.lib.cc_table_unpack_resident(self.h, int(rid), int(base), int(nbytes),
                                                      N.ptr(off) if n else None, n, N.ptr(cols[0]), N.ptr(cols[1]),
                                                      N.ptr(cols[2]), N.ptr(cols[3]), C.byref(ml), C.byref(tid)))
        return tid.value, ml.value

    def _table_ids(self, call, n, mode, delim):
        local = [np.zeros(max(n, 1), np.int32) for _ in range(3)]
        first = [np.zeros(max(n, 1), np.int32) for _ in range(3)]
        rflags, nd = np.zeros(max(n, 1), np.uint8), np.zeros(3, np.int32)
        self._check(call(mode, (delim or "|").encode(), N.ptr(local[0]), N.ptr(local[1]), N.ptr(local[2]), N.ptr(rflags),
                         N.ptr(first[0]), N.ptr(first[1]), N.ptr(first[2]), N.ptr(nd)))
        return [a[:n] for a in local], rflags[:n], [a[:int(k)] for a, k in zip(first, nd)]

    def table_ids(self, stream, rec_off, mode, delim="|"):
        """cc_table_ids on a host stream: (local, rflags, first).  local: the three int32[n] columns
        (barcode, cigar, RG) of local ids in order of first occurrence, -1 for none; rflags: all three
        bits; first: per table the record of each local id's first occurrence."""
        stream = np.ascontiguousarray(stream, np.uint8)
        off = np.ascontiguousarray(rec_off, np.uint64)
        n = len(off)
        return self._table_ids(lambda *a: self.lib.cc_table_ids(self.h, N.ptr(stream) if stream.size else None, stream.size,
                                                                N.ptr(off) if n else None, n, *a), n, mode, delim)

    def table_ids_resident(self, rid, base, nbytes, rec_off, mode, delim="|"):
        """cc_table_ids_resident: table_ids with the records read from bytes [base, base + nbytes) of
        resident stream rid.  The stream is not freed."""
        off = np.ascontiguousarray(rec_off, np.uint64)
        n = len(off)
        return self._table_ids(lambda *a: self.lib.cc_table_ids_resident(self.h, int(rid), int(base), int(nbytes),
                                                                         N.ptr(off) if n else None, n, *a), n, mode, delim)

    def debug_ids_hash_bits(self, bits):
        """Test hook (cc_debug_ids_hash_bits): table_ids keeps the low `bits` bits of a key's hash."""
        self._check(self.lib.cc_debug_ids_hash_bits(self.h, int(bits)))

    def _decode_ids_device(self, bam, interner, mode, delim):
        """Bam.decode_ids' result by the device interner, or None where it refuses the file (the host
        pass decides it then)."""
        rec, stream, off = bam.decode_cols()
        res = bam.resident()
        try:
            if res is not None and res[0] is self:
                local, rflags, first = self.table_ids_resident(res[1], res[2], stream.size, off, mode, delim)
            else:
                local, rflags, first = self.table_ids(stream, off, mode, delim)
        except N.CCError as e:
            if e.code not in (N.CC_E_INVALID, N.CC_E_COLLISION, N.CC_E_UNSUPPORTED):
                raise
            return None
        n = rec.n
        if n and ((rflags ^ rec.rflags[:n]) & 2).any():
            raise N.CCError(-1, "device and host disagree on CC_RF_QUAL_MISSING")
        bam.intern_first(interner, mode, delim, local, first, out=(rec.bc_id, rec.cigar_id, rec.rg_id))
        rec.rflags[:n] = rflags
        return rec, stream, off

    def unpack(self, bam, interner, mode, delim="|"):
        """The device decode of bam: (records, table).  libccio's slim pass (Bam.decode_ids) keeps the
        string work (interned cigar, barcode and RG ids, the string-derived record flags); the raw
        records go to the device, where cc_table_unpack builds every other column and both blobs of
        the table that bam.decode + upload would have given.  records holds the host integer columns
        only.  When this engine's inflater kept bam's bytes on the device (device_resident,
        bam.resident) the records are read there (cc_table_unpack_resident) and the resident stream
        is freed, whether the unpack succeeds or not; an id the engine does not know falls back to the
        upload."""
        got_ids = self._decode_ids_device(bam, interner, mode, delim) if self.ids_device else None
        rec, stream, off = got_ids or bam.decode_ids(interner, mode, delim)
        res = bam.resident()
        got = None
        if res is not None and res[0] is self:
            try:
                got = self.unpack_resident(res[1], res[2], stream.size, off, rec.cigar_id, rec.bc_id, rec.rg_id,
                                           rec.rflags)
            except N.CCError as e:
                if e.code != N.CC_E_INVALID:   # (records the device refuses are refused again below)
                    raise
            finally:
                self.lib.cc_resident_free(self.h, res[1])
                bam.resident_done()
        table, ml = got or self.unpack_raw(stream, off, rec.cigar_id, rec.bc_id, rec.rg_id, rec.rflags)
        if rec.n and ml != rec.max_len:
            self.lib.cc_table_free(self.h, table)
            raise N.CCError(-1, "device and host disagree on the longest read")
        self.tables[table] = rec
        rec.table = table   # (stages._upload takes it instead of uploading)
        return rec, table

    def table(self, bam, interner, mode, delim="|"):
        """(records, table) of bam by the decoder this engine is switched to (device_decode)."""
        if self.decode_device:
            return self.unpack(bam, interner, mode, delim)
        rec = bam.decode(interner, mode, delim)
        return rec, self.upload(rec)

    def derive(self, t):
        """The table's derived columns built again (cc_table_derive; asynchronous)."""
        self._check(self.lib.cc_table_derive(self.h, t))

    def free_table(self, t):
        self.lib.cc_table_free(self.h, t)
        self.tables.pop(t, None)

    def read_bam(self, table, stream, delim_filter, badread_file, scope_by_run, seed=0x5eed):
        sorted_ok = coord_sorted(self.tables[table])
        for attempt in range(6):
            prm = N.cc_read_bam_params(int(delim_filter), int(badread_file), int(scope_by_run), int(sorted_ok),
                                       (seed + 0x9E3779B97F4A7C15 * attempt) & 0xFFFFFFFFFFFFFFFF)
            gid = C.c_int32(0)
            rc = self.lib.cc_read_bam(self.h, table, stream.n, N.ptr(stream.rec), N.ptr(stream.region),
                                      len(stream.region_run), N.ptr(stream.region_run), C.byref(prm), C.byref(gid))
            if rc == N.CC_E_COLLISION:
                self.lib.cc_group_free(self.h, gid.value)
                continue
            if rc != 0:
                msg = self.lib.cc_last_error(self.h).decode(errors="replace")
                self.lib.cc_group_free(self.h, gid.value)
                raise N.CCError(rc, msg)
            return gid.value
        raise N.CCError(N.CC_E_COLLISION, "repeated hash collisions")

    def rerun(self, group, seed):
        self._check(self.lib.cc_read_bam_rerun(self.h, group, seed))

    def counters(self, group):
        a = np.zeros(N.NUM_COUNTERS, np.int64)
        self._check(self.lib.cc_group_counters(self.h, group, N.ptr(a)))
        return {k: int(a[v]) for k, v in N.CNT.items()}

    def fetch(self, group, name, dtype):
        nb = self.lib.cc_fetch(self.h, group, name.encode(), None, 0)
        if nb < 0:
            raise N.CCError(int(nb), self.lib.cc_last_error(self.h).decode())
        out = np.zeros(nb // np.dtype(dtype).itemsize, dtype)
        if nb:
            self.lib.cc_fetch(self.h, group, name.encode(), N.ptr(out), nb)
        return out

    def free_group(self, g):
        self.lib.cc_group_free(self.h, g)

    def consensus_maker(self, group, cutoff):
        n = C.c_int64()
        self._check(self.lib.cc_consensus_maker(self.h, group, float(cutoff), C.byref(n)))
        return n.value

    def duplex_consensus(self, group, swap):
        n = C.c_int64()
        self._check(self.lib.cc_duplex_consensus(self.h, group, N.ptr(swap), len(swap), C.byref(n)))
        return n.value

    def singleton_correction(self, sgroup, ssgroup, swap):
        n = C.c_int64()
        self._check(self.lib.cc_singleton_correction(self.h, sgroup, ssgroup, N.ptr(swap), len(swap), C.byref(n)))
        return n.value

    # ---- function-level boundary
    def sscs_vote(self, table, member_index, fam_offsets, cutoff, stride=None):
        """consensus_maker(readList, cutoff) (SSCS_maker.py:81-168) over caller-given families of a
        table's records: family k = records member_index[fam_offsets[k]:fam_offsets[k+1]], its first
        member the template.  Returns (seq codes (nfam, stride) as BAM nibble codes one per base,
        quals (nfam, stride), meta (nfam, 5) = L, mapq, tlen, flag, rg id)."""
        rec = self.tables[table]
        stride = stride or ((rec.max_len + 15) & ~15)
        mi = np.ascontiguousarray(member_index, np.int32)
        fo = np.ascontiguousarray(fam_offsets, np.int64)
        nf = len(fo) - 1
        seq = np.zeros((max(nf, 1), stride // 2), np.uint8)
        qual = np.zeros((max(nf, 1), stride), np.uint8)
        meta = np.zeros((max(nf, 1), 5), np.int32)
        self._check(self.lib.cc_sscs_vote(self.h, table, N.ptr(mi), N.ptr(fo), nf, float(cutoff), N.ptr(seq),
                                          N.ptr(qual), N.ptr(meta), stride))
        return unpack_nibbles(seq[:nf], stride), qual[:nf], meta[:nf]

    def pair_vote(self, mode, table_a, table_b, rec_a, rec_b, stride=None):
        """duplex_consensus(read1, read2) over caller-given pairs: mode 0 DCS (DCS_maker.py:99-123),
        mode 1 singleton correction's Q>29 variant (singleton_correction.py:61-86)."""
        ml = max(self.tables[table_a].max_len, self.tables[table_b].max_len)
        stride = stride or ((ml + 15) & ~15)
        a = np.ascontiguousarray(rec_a, np.int32)
        b = np.ascontiguousarray(rec_b, np.int32)
        n = len(a)
        seq = np.zeros((max(n, 1), stride // 2), np.uint8)
        qual = np.zeros((max(n, 1), stride), np.uint8)
        meta = np.zeros((max(n, 1), 5), np.int32)
        self._check(self.lib.cc_pair_vote(self.h, int(mode), table_a, table_b, N.ptr(a), N.ptr(b), n, N.ptr(seq),
                                          N.ptr(qual), N.ptr(meta), stride))
        return unpack_nibbles(seq[:n], stride), qual[:n], meta[:n]

    def group(self, keys):
        """cc_group: read_dict's grouping of caller-given keys ((n, key_bytes) uint8, key_bytes a
        multiple of 4): (perm int32, fam_offsets int64), families in first-seen order."""
        k = np.ascontiguousarray(keys, np.uint8)
        n = k.shape[0]
        perm = np.zeros(max(n, 1), np.int32)
        off = np.zeros(n + 1, np.int64)
        nf = C.c_int64()
        self._check(self.lib.cc_group(self.h, n, N.ptr(k), k.shape[1], N.ptr(perm), N.ptr(off), C.byref(nf)))
        return perm[:n], off[:nf.value + 1]

    def duplex_join(self, mode, keys, partner_keys, x_keys=None, vote=None):
        """cc_duplex_join: (decision int32, partner int64) per entry; vote = (table_a, rec_a, table_x,
        rec_x) also returns (seq codes, quals, meta) rows per entry."""
        k = np.ascontiguousarray(keys, np.uint8)
        p = np.ascontiguousarray(partner_keys, np.uint8)
        x = np.ascontiguousarray(x_keys if x_keys is not None else np.zeros((0, k.shape[1]), np.uint8), np.uint8)
        n, m = k.shape[0], x.shape[0]
        dec = np.zeros(max(n, 1), np.int32)
        part = np.zeros(max(n, 1), np.int64)
        seq = qual = meta = None
        ta, ra, tx, rx, stride = -1, None, -1, None, 0
        if vote is not None:
            ta, ra, tx, rx = vote
            ra = np.ascontiguousarray(ra, np.int32)
            rx = np.ascontiguousarray(rx if rx is not None else np.zeros(0, np.int32), np.int32)
            ml = max(self.tables[ta].max_len, self.tables[tx].max_len if tx >= 0 else 0)
            stride = (ml + 15) & ~15
            seq = np.zeros((max(n, 1), stride // 2), np.uint8)
            qual = np.zeros((max(n, 1), stride), np.uint8)
            meta = np.zeros((max(n, 1), 5), np.int32)
        self._check(self.lib.cc_duplex_join(self.h, int(mode), n, N.ptr(k), N.ptr(p), m, N.ptr(x), k.shape[1],
                                            N.ptr(dec), N.ptr(part), ta, N.ptr(ra), tx, N.ptr(rx), N.ptr(seq),
                                            N.ptr(qual), N.ptr(meta), stride))
        if vote is None:
            return dec[:n], part[:n]
        return dec[:n], part[:n], (unpack_nibbles(seq[:n], stride), qual[:n], meta[:n])

    def comm_init(self, world, rank, uid):
        c = N.P()
        self._check(self.lib.cc_comm_init(self.h, int(world), int(rank), uid, C.byref(c)))
        return c

    def reduce_stats(self, comm, counters, fam_count=None, fam_first=None):
        """The sharded pipeline's one collective (RCCL): counters and fam_count summed, fam_first
        min-reduced over the ranks, in place (int64 arrays)."""
        fl = 0 if fam_count is None else len(fam_count)
        self._check(self.lib.cc_reduce_stats(self.h, comm, N.ptr(counters), len(counters),
                                             N.ptr(fam_count) if fl else None, N.ptr(fam_first) if fl else None, fl))

    def allreduce_max(self, comm, v):
        self._check(self.lib.cc_allreduce_max(self.h, comm, N.ptr(v), len(v)))

    def set_profiling(self, on):
        self._check(self.lib.cc_set_profiling(self.h, int(on)))

    def profile_only(self, names=()):
        """Time only these kernel scopes (all when empty)."""
        self._check(self.lib.cc_profile_only(self.h, "\n".join(names).encode()))

    def launch_count(self):
        """Device operations enqueued so far by this process (cc_launch_count)."""
        return int(self.lib.cc_launch_count())

    def kernel_times(self):
        names = C.create_string_buffer(1 << 16)
        ms = np.zeros(256, np.float64)
        cnt = np.zeros(256, np.int64)
        k = self.lib.cc_kernel_times(self.h, names, 1 << 16, N.ptr(ms), N.ptr(cnt), 256)
        nm = names.value.decode().split("\n")[:k]
        return {nm[i]: (float(ms[i]), int(cnt[i])) for i in range(k)}

    def synchronize(self):
        self._check(self.lib.cc_synchronize(self.h))

    def deferred(self, calls):
        """Runs calls() (stage calls on resident groups, e.g. one bench step) with the planned passes'
        end-of-pass checks deferred to one wait at the end (cc_defer / cc_commit).  When a deferred
        pass did not hold its plan, calls() runs again with deferral off: every pass then checks
        itself and re-runs exactly where needed, as without deferral."""
        self._check(self.lib.cc_defer(self.h, 1))
        try:
            calls()
        finally:
            self.lib.cc_defer(self.h, 0)
            rc = self.lib.cc_commit(self.h)
        if rc == N.CC_E_REPLAY:
            calls()
        else:
            self._check(rc)


def comm_unique_id():
    """A fresh RCCL unique id (128 bytes) for cc_comm_init; rank 0 makes it, the others receive it."""
    buf = C.create_string_buffer(128)
    rc = N.amd().cc_comm_unique_id(buf, 128)
    if rc != 0:
        raise N.CCError(rc, "RCCL unique id")
    return buf.raw


def duplex_tag(tag):
    """duplex_tag(tag) (consensus_helper.py:639-683) through libccio (ccio_duplex_tag); IndexError for
    fewer than nine '_' fields, as the reference."""
    t = tag.encode()
    buf = C.create_string_buffer(2 * len(t) + 16)
    k = N.io().ccio_duplex_tag(t, buf, len(buf))
    if k < 0:
        raise IndexError(N.io_error())
    return buf.value.decode()


def pack_keys(tags, width=None):
    """Tag strings as fixed-width byte keys (zero padded to a multiple of 4) for cc_group /
    cc_duplex_join: (n, width) uint8."""
    raw = [t.encode() for t in tags]
    w = width or max([len(r) for r in raw] + [1])
    w = (w + 3) & ~3
    out = np.zeros((len(raw), w), np.uint8)
    for i, r in enumerate(raw):
        if len(r) > w:
            raise ValueError("tag longer than the key width")
        out[i, :len(r)] = np.frombuffer(r, np.uint8)
    return out


def unpack_nibbles(packed, stride):
    """(n, stride/2) BAM nibble bytes -> (n, stride) base codes (first base in the high nibble)."""
    out = np.zeros((packed.shape[0], stride), np.uint8)
    out[:, 0::2] = packed >> 4
    out[:, 1::2] = packed & 15
    return out


# ---------------------------------------------------------------- output helpers
def csn_names(interner, ckey9, suffix):
    n = len(suffix)
    off = np.zeros(n + 1, np.int64)
    ck = np.ascontiguousarray(ckey9, np.int32)
    sf = np.ascontiguousarray(suffix, np.int64)
    need = N.io().ccio_format_csn_names(interner.h, n, N.ptr(ck), N.ptr(sf), None, 0, N.ptr(off))
    if need < 0:
        raise RuntimeError(N.io_error())
    blob = np.zeros(max(int(need), 1), np.uint8)
    N.io().ccio_format_csn_names(interner.h, n, N.ptr(ck), N.ptr(sf), N.ptr(blob), int(need), N.ptr(off))
    return blob, off


def dcs_names(bam, rec_tag, rec_ds):
    n = len(rec_tag)
    off = np.zeros(n + 1, np.int64)
    a = np.ascontiguousarray(rec_tag, np.int64)
    b = np.ascontiguousarray(rec_ds, np.int64)
    need = N.io().ccio_format_dcs_names(bam.h, n, N.ptr(a), N.ptr(b), None, 0, N.ptr(off))
    if need < 0:
        raise RuntimeError(N.io_error())
    blob = np.zeros(max(int(need), 1), np.uint8)
    N.io().ccio_format_dcs_names(bam.h, n, N.ptr(a), N.ptr(b), N.ptr(blob), int(need), N.ptr(off))
    return blob, off


class KeptNames(int):
    """A name set's id (Engine.csn_names / dcs_names / csn_names_group with keep=True): the first item
    of their result in place of the blob.  An int, so it goes wherever a names_id goes."""


def write_bam(path, template, interner, specs, srcs, names=None, name_off=None, cons_seq=None, cons_qual=None,
              level=6, nthreads=0, sink=None, cons_group=None, names_dev=None):
    """Assembles and writes one output BAM (ccio_write_bam).  sink (the orchestrator's fused
    sort_index, Sink) may redirect it: written sorted and indexed under its sorted name, and kept in
    memory for the next stage.  cons_group, in place of cons_seq / cons_qual: (engine, group) whose
    device consensus buffers the engine's assembler reads (Engine.device_assemble); when the
    assembler does not take the write, the arrays are fetched and the host assembles as always.
    names_dev, in place of names: (engine, names_id), a name set the engine's assembler reads where it
    lies (cc_bam_assemble_names; name_off is still the host's); when no hook takes the write
    (ccio_write_bam_ex's -3) the blob is fetched once and the write goes the ordinary way.
    Returns the path written."""
    if names_dev is not None and names is None:
        eng, nid = names_dev
        if eng.assemble_device:
            eng._check(eng.lib.cc_bam_assemble_names(eng.h, int(nid)))
            try:
                return write_bam(path, template, interner, specs, srcs, _NAMES_WITH_HOOK, name_off, cons_seq, cons_qual,
                                 level, nthreads, sink, cons_group)
            except _NeedNames:
                pass
            finally:
                eng.lib.cc_bam_assemble_names(eng.h, 0)
        names = eng.names_fetch(nid)
    if cons_group is not None and cons_seq is None:
        eng, g = cons_group
        if eng.assemble_device:
            eng._check(eng.lib.cc_bam_assemble_group(eng.h, int(g)))
            try:
                return _write_bam(path, template, interner, specs, srcs, names, name_off, None, None, level, nthreads,
                                  sink, own_cons=True)
            except _NeedCons:
                pass
            finally:
                eng.lib.cc_bam_assemble_group(eng.h, -1)
        cons_seq = eng.fetch(g, "cons_seq", np.uint8)
        cons_qual = eng.fetch(g, "cons_qual", np.uint8)
    return _write_bam(path, template, interner, specs, srcs, names, name_off, cons_seq, cons_qual, level, nthreads, sink)


class _PinnedSource(object):
    """Engine.pin_source's context manager."""

    def __init__(self, eng, bam):
        self.eng, self.bam, self.rid = eng, bam, 0

    def __enter__(self):
        io = N.io()
        tok, base = C.c_int64(0), C.c_uint64(0)
        if io.ccio_bam_resident(self.bam.h, C.byref(tok), C.byref(base)):
            return self   # it names a copy already (the inflater's)
        data, nbytes, rec0 = N.P(), C.c_uint64(0), C.c_uint64(0)
        if io.ccio_bam_stream(self.bam.h, C.byref(data), C.byref(nbytes), C.byref(rec0)) != 0:
            return self   # a view: its writes never reach the hooks
        rid = C.c_int64(0)
        self.eng._check(self.eng.lib.cc_resident_put(self.eng.h, data, nbytes.value, C.byref(rid)))
        if io.ccio_bam_set_resident(self.bam.h, rid.value, rec0.value) != 0:
            self.eng.resident_free(rid.value)
            return self
        self.rid = int(rid.value)
        return self

    def __exit__(self, *exc):
        if self.rid:
            rc = N.io().ccio_flush()   # no background write still reads the copy
            N.io().ccio_bam_set_resident(self.bam.h, 0, 0)
            self.eng.resident_free(self.rid)
            self.rid = 0
            if rc != 0 and exc[0] is None:
                raise IOError(N.io_error())
        return False


class _NeedCons(Exception):
    """ccio_write_bam_ex's -2: consensus records, no host arrays, and no hook took the write."""


class _NeedNames(Exception):
    """ccio_write_bam_ex's -3: specs with names, no host names, and no hook took the write."""


_NAMES_WITH_HOOK = object()   # _write_bam's names: ccio_write_bam_ex gets NULL (the names are with the hook)


def _write_bam(path, template, interner, specs, srcs, names, name_off, cons_seq, cons_qual, level, nthreads, sink,
               own_cons=False):
    specs = np.ascontiguousarray(specs, N.OUT_SPEC_DTYPE)
    arr = (N.P * len(srcs))(*[s.h for s in srcs])
    dummy = np.zeros(1, np.uint8)
    dummy_off = np.zeros(2, np.int64)
    out, flags, keep = path, 0, None
    if sink is not None:
        out, flags, k = sink.route(path)
        keep = N.P() if k else None
    with_hook = names is _NAMES_WITH_HOOK
    rc = N.io().ccio_write_bam_ex(out.encode(), template.h, interner.h, len(specs), N.ptr(specs), arr, len(srcs),
                                  None if with_hook else N.ptr(names if names is not None else dummy),
                                  N.ptr(name_off if name_off is not None else dummy_off),
                                  None if own_cons else N.ptr(cons_seq if cons_seq is not None and len(cons_seq) else dummy),
                                  None if own_cons else N.ptr(cons_qual if cons_qual is not None and len(cons_qual) else dummy),
                                  level, nthreads, flags, C.byref(keep) if keep is not None else None)
    if rc == -2 and own_cons:
        raise _NeedCons()
    if rc == -3 and with_hook:
        raise _NeedNames()
    if rc != 0:
        raise IOError(N.io_error())
    if keep is not None:
        sink.kept[out] = Bam._handle(keep.value, out)
    return out


class Sink(object):
    """The orchestrator's fused sort_index (ConsensusCruncher.py:10-34): a stage output X.bam that the
    pipeline would write, then sort to X.sorted.bam (removing X.bam) and index, is written sorted and
    indexed under X.sorted.bam at once; the records of the outputs named in `keep` stay in memory
    (kept) for the stage that reads that file next.  Outputs not named in `fused` are written as the
    stage names them."""

    def __init__(self, fused=(), keep=(), async_writes=False):
        self.fused = set(os.path.abspath(p) for p in fused)
        self.keep = set(os.path.abspath(p) for p in keep)
        self.kept = {}
        # fused outputs compressed and written in the background (CCIO_W_ASYNC): the caller runs
        # flush_writes() before it moves or hands over those files
        self.async_flag = N.W_ASYNC if async_writes else 0

    def route(self, path):
        """(path to write, writer flags, keep the records)"""
        ap = os.path.abspath(path)
        if ap in self.fused:
            return ('{}.sorted.bam'.format(path.split('.bam', 1)[0]), N.W_SORT | N.W_INDEX | self.async_flag,
                    ap in self.keep)
        return path, 0, False

    def take(self, path):
        """The kept records of a written file (Bam, by the path it was written to), or None."""
        return self.kept.pop(path, None)


class MemorySink(Sink):
    """Every stage output kept in memory, no file (the multi-GPU driver, sharded.py): the outputs named
    in `fused` in samtools-sort order under their sorted names (X.bam -> X.sorted.bam), the others in
    written order under their own names; take() hands them over."""

    def __init__(self, fused=()):
        Sink.__init__(self, fused=fused)

    def route(self, path):
        ap = os.path.abspath(path)
        if ap in self.fused:
            return '{}.sorted.bam'.format(path.split('.bam', 1)[0]), N.W_SORT | N.W_MEMORY, True
        return path, N.W_MEMORY, True


def flush_writes():
    """Waits for every background (CCIO_W_ASYNC) write; raises the first failure."""
    if N.io().ccio_flush() != 0:
        raise IOError(N.io_error())


def merge_kept(out, bams, level=6, nthreads=0, index=True, keep=True, async_writes=False, memory=False):
    """samtools merge of sorted record sets in memory (ties keep input order) written to out (+ .bai);
    returns the merged records (Bam) when keep.  async_writes: compressed and written in the
    background (flush_writes); memory: no file, the merged records only."""
    arr = (N.P * len(bams))(*[b.h for b in bams])
    keep = keep or memory
    k = N.P() if keep else None
    fl = (N.W_MEMORY if memory else (N.W_INDEX if index else 0) | (N.W_ASYNC if async_writes else 0))
    rc = N.io().ccio_merge_handles((out or "").encode(), C.cast(arr, N.P), len(bams), level, nthreads, fl,
                                   C.byref(k) if keep else None)
    if rc != 0:
        raise IOError(N.io_error())
    return Bam._handle(k.value, out) if keep else None


def make_specs(n):
    s = np.zeros(n, N.OUT_SPEC_DTYPE)
    s["name_id"] = -1
    s["rg_id"] = -1
    return s


def sort_bam(inp, out, level=6, nthreads=0):
    if N.io().ccio_sort_bam(inp.encode(), out.encode(), level, nthreads) != 0:
        raise IOError(N.io_error())


def merge_bams(out, inputs, level=6, nthreads=0):
    arr = (C.c_char_p * len(inputs))(*[p.encode() for p in inputs])
    if N.io().ccio_merge_bams(out.encode(), C.cast(arr, N.P), len(inputs), level, nthreads) != 0:
        raise IOError(N.io_error())


def concat_bams(out, inputs, level=6, nthreads=0):
    arr = (C.c_char_p * len(inputs))(*[p.encode() for p in inputs])
    if N.io().ccio_concat_bams(out.encode(), C.cast(arr, N.P), len(inputs), level, nthreads) != 0:
        raise IOError(N.io_error())


def index_bam(path):
    """samtools index: writes path + '.bai'."""
    if N.io().ccio_index_bam(path.encode()) != 0:
        raise IOError(N.io_error())


class BarcodeAssertion(AssertionError):
    """extract_barcodes.py:291 `assert r1.id == r2.id`."""


EB_WIDTH, EB_BC = 32, 72   # cc_extract_barcodes: bases per read it reads, barcode bytes per pair


def extract_barcodes_gpu(engine, read1, read2, out_prefix, pattern=None, blist=None, nthreads=0):
    """The UMI extraction with the per-pair decision on the GPU (cc_extract_barcodes): libccio reads the
    FASTQs (ccio_fq_open / ccio_fq_heads) and writes the outputs from the decisions (ccio_fq_write).
    Same results as extract_barcodes; None when the barcodes exceed the kernel's sizes (32 bases,
    1024 listed barcodes, 31 lengths)."""
    io = N.io()
    if pattern is not None:
        if len(pattern) > EB_WIDTH:
            return None
        min_len, lens = len(pattern), None
    else:
        lens = sorted({len(b) for b in blist}, reverse=True)
        if len(blist) > 1024 or max(lens) > EB_WIDTH or len(lens) > 31:
            return None
        min_len = 0
    f = io.ccio_fq_open(read1.encode(), read2.encode(), min_len, nthreads)
    if not f:
        raise IOError(N.io_error())
    try:
        n = C.c_int64()
        stop = C.c_int32()
        io.ccio_fq_info(f, C.byref(n), C.byref(stop))
        stop_msg = N.io_error() if stop.value else None
        n = n.value
        h1 = np.zeros((max(n, 1), EB_WIDTH), np.uint8)
        h2 = np.zeros((max(n, 1), EB_WIDTH), np.uint8)
        l1 = np.zeros(max(n, 1), np.int32)
        l2 = np.zeros(max(n, 1), np.int32)
        if io.ccio_fq_heads(f, EB_WIDTH, N.ptr(h1), N.ptr(h2), N.ptr(l1), N.ptr(l2)) != 0:
            raise IOError(N.io_error())
        nh = 5 * len(pattern) if pattern is not None else len(blist)
        st = np.zeros(max(n, 1), np.uint8)
        bc = np.zeros((max(n, 1), EB_BC), np.uint8)
        c1 = np.zeros(max(n, 1), np.int32)
        c2 = np.zeros(max(n, 1), np.int32)
        b1 = np.zeros(max(n, 1), np.uint32)
        b2 = np.zeros(max(n, 1), np.uint32)
        cnt = np.zeros(3, np.int64)
        r1 = np.zeros(max(nh, 1), np.int64)
        r2 = np.zeros(max(nh, 1), np.int64)
        arr = (C.c_char_p * len(blist))(*[b.encode() for b in blist]) if pattern is None else None
        engine._check(engine.lib.cc_extract_barcodes(
            engine.h, n, N.ptr(h1), N.ptr(h2), N.ptr(l1), N.ptr(l2),
            pattern.encode() if pattern is not None else None, C.cast(arr, N.P) if arr is not None else None,
            len(blist) if pattern is None else 0, N.ptr(st), N.ptr(bc), N.ptr(c1), N.ptr(c2), N.ptr(b1), N.ptr(b2),
            N.ptr(cnt), N.ptr(r1), N.ptr(r2)))
        la = np.array(lens if lens else [0], np.int32)
        if io.ccio_fq_write(f, out_prefix.encode(), 0 if pattern is not None else 1, N.ptr(st), N.ptr(bc), EB_BC,
                            N.ptr(c1), N.ptr(c2), N.ptr(b1), N.ptr(b2), N.ptr(la), len(lens) if lens else 0,
                            nthreads) != 0:
            raise IOError(N.io_error())
    finally:
        io.ccio_fq_close(f)
    counts = dict(pairs=n + (1 if stop.value else 0), bad_spacer=int(cnt[0]), bad_barcode=int(cnt[1]),
                  good=int(cnt[2]), written=n)
    if stop.value == -2:
        raise BarcodeAssertion(stop_msg)
    if stop.value:
        raise IOError(stop_msg)
    if pattern is not None:
        return counts, r1[:nh].reshape(len(pattern), 5), r2[:nh].reshape(len(pattern), 5)
    return counts, r1[:nh], r2[:nh]


def extract_barcodes(read1, read2, out_prefix, pattern=None, blist=None, nthreads=0, engine=None):
    """libccio's UMI extraction (extract_barcodes.py:287-405).  Returns (counts dict, r1_hist, r2_hist):
    pattern mode histograms are (len(pattern), 5) over A,C,G,T,N; list mode one count per entry of
    `blist` (distinct barcodes).  Raises BarcodeAssertion where the reference's id assertion fails
    (the pairs before it written).  With an engine the per-pair decisions run on the GPU
    (extract_barcodes_gpu), barcodes beyond its sizes on the host."""
    if pattern is None and not blist:
        raise ValueError("No barcode specifications inputted. Please specify barcode list or pattern.")
    if engine is not None:
        got = extract_barcodes_gpu(engine, read1, read2, out_prefix, pattern, blist, nthreads)
        if got is not None:
            return got
    nh = 5 * len(pattern) if pattern is not None else len(blist)
    h1 = np.zeros(max(nh, 1), np.int64)
    h2 = np.zeros(max(nh, 1), np.int64)
    cnt = np.zeros(4, np.int64)
    nw = np.zeros(1, np.int64)
    arr = None
    if pattern is None:
        arr = (C.c_char_p * len(blist))(*[b.encode() for b in blist])
    rc = N.io().ccio_extract_barcodes(read1.encode(), read2.encode(), out_prefix.encode(),
                                      pattern.encode() if pattern is not None else None,
                                      C.cast(arr, N.P) if arr is not None else None,
                                      len(blist) if blist else 0, nthreads, N.ptr(cnt), N.ptr(h1), N.ptr(h2),
                                      N.ptr(nw))
    counts = dict(pairs=int(cnt[0]), bad_spacer=int(cnt[1]), bad_barcode=int(cnt[2]), good=int(cnt[3]),
                  written=int(nw[0]))
    if rc == -2:
        raise BarcodeAssertion(N.io_error())
    if rc != 0:
        raise IOError(N.io_error())
    if pattern is not None:
        return counts, h1[:nh].reshape(len(pattern), 5), h2[:nh].reshape(len(pattern), 5)
    return counts, h1[:nh], h2[:nh]
