"""One sample's consensus pipeline over several GPUs, split along the bed regions.

The reference processes its bed regions one after another (SSCS_maker.py:265-281,
DCS_maker.py:204-218, singleton_correction.py:203-229; consensus_helper.py:38-54), with pair_dict
persisting across regions.  A family, its duplex partner and its singleton-correction complement
share their coordinates, so they complete in one region; the regions therefore split into
contiguous blocks, one per rank, and every stage of the sample uses the same block plan.

Each rank holds only the records at its block's positions (its device tables are about 1/N of
the sample):
  * the input BAM is read through its BAI, only the block's regions (ccio_bam_open_regions);
  * a pair whose two ends fall to different ranks completes at its later-streamed end: the rank
    holding the first-streamed end moves that record (raw BAM bytes) to the completing rank, where
    it enters the stream as a foreign entry (region -(r+1)) before the rank's own entries and pairs
    by coordinates like the rest; the sender keeps its entry marked CC_REGION_MOVED (not paired
    there, counted once over the ranks, listed as a bad read only by the sender: cc_read_bam);
  * every stage output record goes to the rank owning its position (a consensus of a foreign end
    sits in another block), and each rank stably sorts what it receives in sender order: exactly
    its part of the whole-sample sorted file the next stage of the reference reads (the samtools
    stand-in's stable sort of the rank-order concatenation), without that file on the critical
    path.  The next stage runs on these rank-local inputs.
The exchanges are host-side and small (cross-block pairs only).  The stats.txt / read_families.txt
quantities are reduced once per stage (the path's one collective: over RCCL through
cc_reduce_stats on GPUs, gloo on CPU), rank 0 writes the side outputs, and at the end rank 0
merges the ranks' sorted parts into the reference's output files (ties in rank order, which is
the whole-sample sort's order).

Two drivers run the same code: LocalComm runs the ranks one after another in this process on one
GPU (tests: the outputs equal the single-pass pipeline's byte for byte); TorchComm is one process
per GPU under torch.distributed.
"""
import os
import shutil
import time

import numpy as np

from .consensus_helper import region_list, region_runs
from .engine import (MODE_DUPLEX, MODE_SSCS, Bam, Interner, MemorySink, Stream, bed_stream, concat_bams, flush_writes,
                     index_bam, merge_bams, merge_kept)
from . import native as N
from .shard import (BLOCK_LO, TAIL_KEY, overlap_safe_blocks, overlap_safe_cuts, plan_blocks, position_keys, position_windows,
                    region_of_positions, region_overlaps, window_blocks)
from .stages import DCSRun, SCRun, SSCSRun, dcs_side, sc_side, sscs_side, warm_plotting

COUNTER_KEYS = ("COUNTER", "UNMAPPED", "UNMAPPED_MATE", "MULTIPLE_MAPPING", "BAD_SPACER", "PAIRS", "READ_ENDS",
                "FAMILIES", "ENTRIES", "UNPAIRED", "ORPHAN_TAGS", "DROPPED", "BAD_LISTED", "FOREIGN")
SCALARS = ("sscs", "singletons", "never_emitted", "dcs", "sscs_singletons", "processed", "sscs_correction",
           "singleton_correction", "uncorrected", "mapped_own")


def combine_parts(parts):
    """The reduction of the per-rank stage parts (rank order): counters and stage counts summed;
    read_families' Counter (SSCS_maker.py:401-408) merged in first-seen order over the ranks'
    creation orders, i.e. ordered by (first rank holding the size, its place in that rank's table)."""
    out = {"counters": {k: sum(p["counters"].get(k, 0) for p in parts) for k in parts[0]["counters"]}}
    for k in SCALARS:
        if k in parts[0]:
            out[k] = sum(p[k] for p in parts)
    if "families" in parts[0]:
        order, cnt = [], {}
        for p in parts:
            for size, n in p["families"]:
                if size not in cnt:
                    order.append(size)
                    cnt[size] = 0
                cnt[size] += n
        out["families"] = [(s, cnt[s]) for s in order]
    if "mapped" in parts[0]:
        out["mapped"] = parts[0]["mapped"]
    return out


class LocalComm(object):
    """world ranks run one after another in this process (one GPU)."""

    def __init__(self, world):
        self.world = world
        self.rank = 0
        self.ranks = list(range(world))

    def each(self, fn):
        return {r: fn(r) for r in self.ranks}

    def exchange(self, sends):
        """sends[r][d]: what rank r sends rank d -> received[d][s] from every rank s."""
        return {d: [sends[s][d] for s in range(self.world)] for d in self.ranks}

    def reduce(self, parts):
        return combine_parts([parts[r] for r in range(self.world)])

    def broadcast_obj(self, obj):
        return obj

    def barrier(self):
        pass

    def close(self):
        pass


_DT = {0: np.dtype(np.uint8), 1: np.dtype(np.int32), 2: np.dtype(np.int64)}


def _encode(arrays):
    """A tuple of uint8 / int32 / int64 arrays as bytes: count, then (dtype code, length, data) each."""
    code = {v: k for k, v in _DT.items()}
    parts = [np.array([len(arrays)], np.int64)]
    for a in arrays:
        a = np.ascontiguousarray(a)
        parts.append(np.array([code[a.dtype], a.nbytes], np.int64))
        parts.append(a)
    return np.concatenate([x.view(np.uint8) for x in parts])


def _decode(buf):
    n = int(buf[:8].view(np.int64)[0])
    out, o = [], 8
    for _ in range(n):
        c, nb = buf[o:o + 16].view(np.int64)
        o += 16
        out.append(buf[o:o + int(nb)].copy().view(_DT[int(c)]))
        o += int(nb)
    return tuple(out)


class RankFailed(RuntimeError):
    """Another rank raised inside a phase of the sharded pipeline."""


class TorchComm(object):
    """One process per GPU under torch.distributed (RCCL as backend "nccl" on ROCm, gloo on CPU).
    Every phase ends in a MAX-reduce of a failure flag, so an exception on one rank stops every rank
    instead of leaving the others blocked in a collective.  With an engine on a "nccl" group the
    stats reduction is cc_reduce_stats over the engine's own RCCL communicator."""

    def __init__(self, group=None, engine=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.ranks = [self.rank]
        self.engine = engine
        self.cc_comm = None
        if engine is not None and dist.get_backend(group) == "nccl":
            from .engine import comm_unique_id
            uid = self.broadcast_obj(comm_unique_id() if self.rank == 0 else None)
            self.cc_comm = engine.comm_init(self.world, self.rank, uid)

    def close(self):
        if self.cc_comm is not None:
            N.amd().cc_comm_destroy(self.cc_comm)
            self.cc_comm = None

    def _device(self):
        import torch
        if self.dist.get_backend(self.group) == "nccl":
            return torch.device("cuda", torch.cuda.current_device())
        return torch.device("cpu")

    def _any(self, flag):
        import torch
        t = torch.tensor([1 if flag else 0], dtype=torch.int64, device=self._device())
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.group)
        return bool(t.item())

    def each(self, fn):
        err = None
        try:
            res = fn(self.rank)
        except BaseException as e:   # noqa: B902 -- re-raised below, after the other ranks learn of it
            err = e
        if self._any(err is not None):
            if err is not None:
                raise err
            raise RankFailed("another rank failed in this phase of the sharded pipeline")
        return {self.rank: res}

    def exchange(self, sends):
        """all_to_all of each rank's payloads (tuples of numpy arrays) over the process group; a
        rank's payload to itself stays in place (nothing of it crosses the collective)."""
        import torch
        dev = self._device()
        mine = sends[self.rank]
        blobs = [_encode(x) if d != self.rank else np.zeros(0, np.uint8) for d, x in enumerate(mine)]
        n_out = torch.tensor([len(b) for b in blobs], dtype=torch.int64, device=dev)
        n_in = torch.zeros(self.world, dtype=torch.int64, device=dev)
        self.dist.all_to_all_single(n_in, n_out, group=self.group)
        out = torch.from_numpy(np.concatenate(blobs)).to(dev)
        inp = torch.zeros(int(n_in.sum().item()), dtype=torch.uint8, device=dev)
        self.dist.all_to_all_single(inp, out, output_split_sizes=n_in.tolist(), input_split_sizes=n_out.tolist(),
                                    group=self.group)
        buf = inp.cpu().numpy()
        got, o = [], 0
        for s_, k in enumerate(n_in.tolist()):
            got.append(mine[s_] if s_ == self.rank else _decode(buf[o:o + k]))
            o += k
        return {self.rank: got}

    def reduce(self, parts):
        return self.reduce_part(parts[self.rank])

    def reduce_part(self, part):
        """combine_parts over the ranks with collectives: one SUM of the counter/count vector, and for
        the family table a MAX of its length, a SUM of the per-size counts and a MIN of each size's
        first-seen key (rank << 40 | place)."""
        ckeys = sorted(part["counters"])
        skeys = [k for k in SCALARS if k in part]
        vec = np.array([part["counters"][k] for k in ckeys] + [part[k] for k in skeys], np.int64)
        fam = part.get("families")
        top = np.array([max([s for s, _ in fam], default=0) if fam is not None else 0], np.int64)
        self._allreduce(top, "max")
        n = int(top[0]) + 1 if fam is not None else 0
        cnt = np.zeros(n, np.int64)
        first = np.full(n, 1 << 62, np.int64)
        if fam:
            sizes = np.array([s for s, _ in fam], np.int64)
            cnt[sizes] = [c for _, c in fam]
            first[sizes] = (self.rank << 40) + np.arange(len(fam), dtype=np.int64)
        if self.cc_comm is not None:
            self.engine.reduce_stats(self.cc_comm, vec, cnt if n else None, first if n else None)
        else:
            self._allreduce(vec, "sum")
            if n:
                self._allreduce(cnt, "sum")
                self._allreduce(first, "min")
        out = {"counters": dict(zip(ckeys, vec[:len(ckeys)].tolist()))}
        out.update(zip(skeys, vec[len(ckeys):].tolist()))
        if fam is not None:
            present = np.nonzero(cnt)[0]
            out["families"] = [(int(s), int(cnt[s])) for s in present[np.argsort(first[present], kind="stable")]]
        if "mapped" in part:
            out["mapped"] = part["mapped"]
        return out

    def _allreduce(self, a, op):
        if self.cc_comm is not None and op == "max":
            self.engine.allreduce_max(self.cc_comm, a)
            return
        import torch
        t = torch.from_numpy(a).to(self._device())
        self.dist.all_reduce(t, op={"sum": self.dist.ReduceOp.SUM, "max": self.dist.ReduceOp.MAX,
                                    "min": self.dist.ReduceOp.MIN}[op], group=self.group)
        a[:] = t.cpu().numpy()

    def broadcast_obj(self, obj):
        lst = [obj]
        self.dist.broadcast_object_list(lst, src=0, group=self.group)
        return lst[0]

    def barrier(self):
        self.dist.barrier(group=self.group)


# ------------------------------------------------------------------ the sample's region geometry
class _Cores(object):
    """tid / pos columns of a record set (what bed_stream reads)."""

    def __init__(self, bam):
        self.tid, self.pos, self.mtid, self.mpos, _ = bam.cores()
        self.n = bam.n


class Geometry(object):
    """The bed regions of a sample, their owner ranks (a block plan of contiguous regions) and the
    per-rank streams and exchanges.  Without a bed file (bedfile None, the reference's -b False: the
    whole file is one region) the blocks are position ranges [lo, hi) of shard.position_keys and
    every stream entry is in region 0 (shard.TAIL_KEY: the unplaced tail, in the last block)."""

    def __init__(self, refs, bedfile, blocks, cuts=None):
        self.bedfile = bedfile
        self.refs = refs
        self.names = {n: i for i, (n, _) in enumerate(refs)}
        self.positional = bedfile is None
        if self.positional:
            self.regions = []
            self.blocks = [(int(lo), int(hi)) for lo, hi in blocks]
            if any(self.blocks[k][1] != self.blocks[k + 1][0] for k in range(len(self.blocks) - 1)) or \
                    self.blocks[0][0] > BLOCK_LO or self.blocks[-1][1] <= TAIL_KEY:
                raise ValueError("position blocks must be contiguous and cover every position")
            self.cuts = np.array([lo for lo, _ in self.blocks[1:]], np.int64)
            self.world = len(self.blocks)
            self.run = np.zeros(1, np.int32)
            self.keys = None
            return
        self.regions = region_list(bedfile)
        n = len(self.regions)
        if cuts is None:
            # overlapping regions stay in one block (shard.overlap_safe_blocks)
            rb = overlap_safe_blocks(blocks, self.regions)
            self.adjusted = [tuple(b) for b in rb] != [tuple(b) for b in blocks]
            cuts = [(int(lo), BLOCK_LO) for lo, _ in rb[1:]]
        else:
            # the world - 1 stream points (region, position key) where the next rank begins; key
            # BLOCK_LO is the region's start (shard.region_cuts: a hot region split between two
            # position groups, never a region that overlaps another)
            # a region-start cut between two overlapping regions moves forward past them, as
            # overlap_safe_blocks moves a block boundary (both regions stream the shared records)
            cuts, self.adjusted = overlap_safe_cuts([(int(r), int(k)) for r, k in cuts], self.regions)
            for r, k in cuts:
                if k > BLOCK_LO and region_overlaps(self.regions, r):
                    raise ValueError("a bed region that overlaps another cannot be split")
        if any(cuts[j] > cuts[j + 1] for j in range(len(cuts) - 1)):
            raise ValueError("block cuts must be in stream order")
        self.cut_r = np.array([r for r, _ in cuts], np.int64)
        self.cut_k = np.array([k for _, k in cuts], np.int64)
        self.world = len(cuts) + 1
        # each block's regions [lo, hi), a split region in both blocks
        ends = [r + (1 if k > BLOCK_LO else 0) for r, k in cuts] + [n]
        starts = [0] + [r for r, _ in cuts]
        self.blocks = [(min(starts[j], ends[j]), ends[j]) for j in range(self.world)]
        self.split = any(k > BLOCK_LO for _, k in cuts)
        self.run = np.array(region_runs(self.regions), np.int32)
        self.keys = [x[0] for x in self.regions]

    def owner_of_keys(self, keys):
        """The rank whose position block holds each key (positional geometry)."""
        return np.searchsorted(self.cuts, np.asarray(keys, np.int64), "right").astype(np.int64)

    def owner_of(self, reg, keys):
        """The rank owning each stream point (bed region, position key); region -1: rank 0."""
        reg = np.asarray(reg, np.int64)
        keys = np.asarray(keys, np.int64)
        o = np.zeros(len(reg), np.int64)
        for r, k in zip(self.cut_r, self.cut_k):
            o += (reg > r) | ((reg == r) & (keys >= k))
        return o

    def block(self, rank):
        """(tids, begs, ends) of rank's regions (an unknown contig raises, as pysam's fetch does); a
        position block as one range per contig it touches, tid -1 for the unplaced tail."""
        lo, hi = self.blocks[rank]
        if self.positional:
            t, b, e = [], [], []
            for i, (_, ln) in enumerate(self.refs):
                a = max(lo, i << 32) - (i << 32)
                z = min(hi, (i << 32) + max(int(ln), 0) + 1) - (i << 32)
                if z > a:
                    t.append(i)
                    b.append(a)
                    e.append(z)
            if hi > TAIL_KEY:
                t.append(-1)
                b.append(0)
                e.append(1)
            return t, b, e
        out = []
        # a split region: its part from the block's start cut / up to its end cut
        k0 = int(self.cut_k[rank - 1]) if rank > 0 and self.cut_k[rank - 1] > BLOCK_LO else None
        k1 = int(self.cut_k[rank]) if rank < self.world - 1 and self.cut_k[rank] > BLOCK_LO else None
        for r in range(lo, hi):
            _, chrom, start, end = self.regions[r]
            if chrom not in self.names:
                raise ValueError("invalid contig `%s`" % chrom)
            if r == lo and k0 is not None:
                start = max(start, k0 & 0xffffffff)
            if r == hi - 1 and k1 is not None:
                end = min(end, k1 & 0xffffffff)
            out.append((self.names[chrom], start, end))
        return ([x[0] for x in out], [x[1] for x in out], [x[2] for x in out])

    def own_stream(self, cores, rank):
        """The rank's own stream over its record set: its regions in bed order, start <= pos < end;
        without a bed file its block's records in table (file) order, region 0."""
        if self.positional:
            lo, hi = self.blocks[rank]
            k = position_keys(cores.tid, cores.pos)
            rec = np.flatnonzero((k >= lo) & (k < hi)).astype(np.int32)
            return rec, np.zeros(len(rec), np.int32)
        st = bed_stream(cores, self.refs, self.bedfile, block=self.blocks[rank])
        if not self.split:
            return st.rec, st.region
        mine = self.owner_of(st.region, position_keys(cores.tid[st.rec], cores.pos[st.rec])) == rank
        return st.rec[mine], st.region[mine]

    def sent(self, cores, own, rank):
        """Which of rank's own stream entries are first-streamed ends of pairs completing in another
        rank's block (shard_streams' rule, the mate's region from the record's mate coordinates), and
        each one's destination rank.  A single block sends nothing.  Position blocks: the mate's
        position key is later in the file and owned by another rank."""
        rec, reg = own
        if self.world == 1:
            return np.zeros(len(rec), bool), np.zeros(len(rec), np.int64)
        if self.positional:
            mk = position_keys(cores.mtid[rec], cores.mpos[rec])
            ok = position_keys(cores.tid[rec], cores.pos[rec])
            to = self.owner_of_keys(mk)
            return (cores.mtid[rec] >= 0) & (mk > ok) & (to != rank), to
        if not self._overlapping():
            # one native pass (ccio_stream_sent) over the entries: the same rule as below
            lo, hi, ivr = self._intervals()
            n = len(rec)
            send = np.zeros(max(n, 1), np.uint8)
            to = np.zeros(max(n, 1), np.int64)
            c = lambda a, t: np.ascontiguousarray(a, t)  # noqa: E731
            arrs = [c(rec, np.int32), c(reg, np.int32), c(cores.tid, np.int32), c(cores.pos, np.int32),
                    c(cores.mtid, np.int32), c(cores.mpos, np.int32)]
            N.io().ccio_stream_sent(n, *[N.ptr(a) for a in arrs], len(lo), N.ptr(lo), N.ptr(hi), N.ptr(ivr),
                                    len(self.cut_r), N.ptr(c(self.cut_r, np.int64)), N.ptr(c(self.cut_k, np.int64)),
                                    int(rank), N.ptr(send), N.ptr(to))
            return send[:n].astype(bool), to[:n]
        mate_reg = region_of_positions(self.regions, self.names, cores.mtid[rec], cores.mpos[rec], hint=reg)
        mk = position_keys(cores.mtid[rec], cores.mpos[rec])
        to = np.where(mate_reg >= 0, self.owner_of(mate_reg, mk), -1)
        # later-streamed: a later region, or later in the same region (a split region's other part)
        later = (mate_reg > reg) | ((mate_reg == reg) & (mk > position_keys(cores.tid[rec], cores.pos[rec])))
        return later & (to >= 0) & (to != rank), to

    def routes(self, bam, cores, own, rank, sent=None):
        """What rank sends each rank: the first-streamed ends of its pairs completing in the other's
        block (raw records, their regions), in stream order.  They are moved: the receiver pairs and
        counts them, the sender's entries carry CC_REGION_MOVED (stage_input)."""
        rec, reg = own
        send, to = sent if sent is not None else self.sent(cores, own, rank)
        out = []
        for d in range(self.world):
            m = send & (to == d)
            out.append((bam.pack(rec[m]) if m.any() else np.zeros(0, np.uint8), reg[m].astype(np.int32)))
        return out

    def stage_input(self, bam, own, received, mode, delim, it, moved=None, engine=None):
        """The rank's table (its records and the foreign ends, sorted by position) decoded, and its
        stream: the foreign entries in global stream order (sender rank, then the sender's stream
        order), then its own entries (those moved to another rank marked CC_REGION_MOVED)."""
        blobs = [b for b, _ in received if len(b)]
        fregs = np.concatenate([r for _, r in received]).astype(np.int64) if received else np.zeros(0, np.int64)
        rec, reg = own
        nf = len(fregs)
        srec = np.empty(nf + len(rec), np.int32)
        if blobs:
            # each combined record's place (the inverse of the combine's origin), int32 throughout
            table = Bam.combine([bam], blobs, key=0)
            inv = np.empty(table.n, np.int32)
            inv[table.origin()] = np.arange(table.n, dtype=np.int32)
            srec[:nf] = inv[bam.n:bam.n + nf]
            np.take(inv, rec, out=srec[nf:])
        else:   # the table is the rank's own records: the stream's records as they are
            table = bam
            srec[nf:] = rec
        sreg = np.empty(nf + len(rec), np.int32)
        sreg[:nf] = -(fregs + 1)
        sreg[nf:] = reg
        if moved is not None:
            sreg[nf:][np.asarray(moved, bool)] |= N.REGION_MOVED
        if engine is not None and engine.decode_device:   # (its table is built with it: stages._upload)
            records = engine.unpack(table, it, mode, delim)[0]
        else:
            records = table.decode(it, mode, delim)
        return table, records, Stream(srec, sreg, self.run, self.keys)

    def owners(self, b):
        """The rank owning each record's position (records at no region's position: rank 0)."""
        t, p, _, _, _ = b.cores()
        if self.world == 1:
            return np.zeros(len(t), np.int64)
        if self.positional:
            return self.owner_of_keys(position_keys(t, p))
        k = position_keys(t, p)
        if len(k) > 1 and b.is_sorted(1) and not self._overlapping():
            # a sorted record set: each region's records are one run of the keys (a search per region
            # instead of one per record); records at no region's position stay with rank 0
            out = np.zeros(len(k), np.int64)
            for r, (_, chrom, start, end) in enumerate(self.regions):
                tt = self.names.get(chrom)
                if tt is None or end <= max(start, 0):
                    continue
                i0, i1 = np.searchsorted(k, [(tt << 32) + max(start, 0), (tt << 32) + end])
                if i1 <= i0:
                    continue
                if self.split and r in self._split_regions():
                    out[i0:i1] = self.owner_of(np.full(i1 - i0, r, np.int64), k[i0:i1])
                else:   # a whole region: one owner
                    out[i0:i1] = int(self.owner_of(np.array([r]), np.array([BLOCK_LO]))[0])
            return out
        reg = region_of_positions(self.regions, self.names, t, p)
        return np.where(reg >= 0, self.owner_of(reg, k), 0)

    def _intervals(self):
        """The bed regions as sorted position-key intervals [lo, hi) and their region indices
        (shard.region_of_positions' table; regions of unknown contigs or empty ones left out)."""
        if not hasattr(self, "_iv"):
            iv = sorted((self.names[c], max(s0, 0), e, r) for r, (_, c, s0, e) in enumerate(self.regions)
                        if c in self.names and e > max(s0, 0))
            self._iv = (np.array([(t << 32) + a for t, a, _, _ in iv], np.int64),
                        np.array([(t << 32) + e for t, _, e, _ in iv], np.int64),
                        np.array([r for _, _, _, r in iv], np.int32))
        return self._iv

    def _split_regions(self):
        """The regions a cut falls inside (their records have owners on both sides of it)."""
        return {int(r) for r, k in zip(self.cut_r, self.cut_k) if k > BLOCK_LO}

    def _overlapping(self):
        """Whether two bed regions of one contig intersect (cytoband tables: never)."""
        if not hasattr(self, "_ovl"):
            iv = sorted((self.names.get(c, -1), max(s0, 0), e) for _, c, s0, e in self.regions if e > max(s0, 0))
            self._ovl = any(a[0] == b[0] and b[1] < a[2] for a, b in zip(iv, iv[1:]))
        return self._ovl

    def split_by_position(self, b, rank):
        """A rank's records (a Bam in memory) split by the rank owning each record's position: the raw
        records for every other rank, and the mask of the records it keeps."""
        to = self.owners(b)
        sends = []
        for d in range(self.world):
            idx = np.flatnonzero(to == d) if d != rank else np.zeros(0, np.int64)
            sends.append((b.pack(idx) if len(idx) else np.zeros(0, np.uint8),))
        return sends, to == rank


def _part(path, rank):
    d, b = os.path.split(path)
    return os.path.join(d, ".shard%d" % rank, b)


def _indexed_input(bam, workdir):
    """The path to read `bam` through, with a current BAI: its own index when one exists and is not
    older than the BAM (htslib warns about an older one; a stale index names the wrong blocks);
    otherwise a link to the BAM in the output directory, indexed there (a user's index next to the
    input, stale or absent, is never written over)."""
    bai = bam + ".bai"
    if os.path.exists(bai) and os.path.getmtime(bai) >= os.path.getmtime(bam):
        return bam
    os.makedirs(workdir, exist_ok=True)
    link = os.path.join(workdir, ".input." + os.path.basename(bam))
    if os.path.lexists(link):
        os.remove(link)
    os.symlink(os.path.abspath(bam), link)
    index_bam(link)
    return link


PLAN_WINDOW = 1 << 16   # bp per weight window of a position plan (the BAI's linear-index grain is 16 kb)


def region_plan(bam_path, bedfile, world):
    """The sample's block plan: contiguous region blocks with near-equal compressed bytes, from the
    input's BAI (no decode); without a bed file, position blocks cut at PLAN_WINDOW windows."""
    hdr = Bam.open_regions(bam_path, [], [], [])

    def weights(t, b, e):
        w = np.zeros(len(t), np.int64)
        if len(t) and N.io().ccio_bai_region_bytes(bam_path.encode(), len(t), N.ptr(np.ascontiguousarray(t, np.int32)),
                                                    N.ptr(np.ascontiguousarray(b, np.int64)),
                                                    N.ptr(np.ascontiguousarray(e, np.int64)), N.ptr(w)) != 0:
            raise IOError(N.io_error())
        return w
    if bedfile is None:
        t, b, e = position_windows(hdr.refs, PLAN_WINDOW)
        return window_blocks(hdr.refs, weights(t, b, e), PLAN_WINDOW, world)
    names = {n: i for i, (n, _) in enumerate(hdr.refs)}
    regions = region_list(bedfile)
    t = np.array([names.get(c, -1) for _, c, _, _ in regions], np.int32)
    b = np.array([s for _, _, s, _ in regions], np.int64)
    e = np.array([x for _, _, _, x in regions], np.int64)
    w = weights(t, b, e)
    blocks = plan_blocks(w, world)
    # regions split between position groups: one holding more than 1/world of the input, or one that a
    # cut would fall inside holding more than 1/(4 world) (a region-boundary cut would leave the blocks
    # that far apart); a region that overlaps another is never split (shard.overlap_safe_blocks)
    cum = np.concatenate([[0], np.cumsum(w)])
    tot = float(cum[-1])
    straddle = {int(np.searchsorted(cum, tot * k / world, "right")) - 1 for k in range(1, world)}
    hot = [r for r in range(len(regions))
           if world > 1 and t[r] >= 0 and not region_overlaps(regions, r) and
           (w[r] * world > tot or (r in straddle and w[r] * 4 * world > tot))]
    if not hot:
        return blocks
    # a region holding more than 1/world of the input is planned by its position groups: rank 0 reads
    # its records' coordinates (the BAI cannot resolve below 16 kb, and a deep locus is a few hundred
    # bp), each group weighted by its records' share of the region's bytes
    units = []   # (region, position key or None, weight)
    for r in range(len(regions)):
        if r in hot:
            h = Bam.open_regions(bam_path, [int(t[r])], [int(b[r])], [int(e[r])])
            ht, hp, _, _, _ = h.cores()
            uk, cnt = np.unique(position_keys(ht, hp), return_counts=True)
            per = float(w[r]) / max(int(cnt.sum()), 1)
            units += [(r, int(k), float(c) * per) for k, c in zip(uk, cnt)]
            h.close()
        else:
            units.append((r, None, float(w[r])))
    cuts = []
    for lo, _ in plan_blocks([u[2] for u in units], world)[1:]:
        if lo >= len(units):
            cuts.append((len(regions), BLOCK_LO))
        else:
            r, k, _ = units[lo]
            first = k is None or lo == 0 or units[lo - 1][0] != r
            cuts.append((r, BLOCK_LO if first else k))
    # a region-boundary cut never separates two overlapping regions (Geometry applies the same rule)
    return {"cuts": overlap_safe_cuts(cuts, regions)[0]}


def to_owners(comm, geo, parts):
    """Records by position owner: each rank's records (parts[r]: a Bam in memory, e.g. a stage output
    kept by MemorySink, or a BAM path) split by the rank owning each record's position, exchanged, and
    stably sorted in sender order with the samtools stand-in key: each rank's part of the whole-sample
    sorted file.  A rank's own records never leave it (placed at its sender position), and at world
    size 1 nothing moves: a part already in that order is returned as it is."""
    def opened(r):
        return Bam(parts[r]) if isinstance(parts[r], str) else parts[r]
    if comm.world == 1:
        def one(r):
            b = opened(r)
            return b if b.is_sorted(1) else b.route(None, (), 0, key=1)
        return comm.each(one)
    held = comm.each(opened)
    split = comm.each(lambda r: geo.split_by_position(held[r], r))
    recv = comm.exchange({r: split[r][0] for r in split})

    def place(r):
        keep, blobs = split[r][1], [x[0] for x in recv[r]]
        # nothing leaves or reaches this rank: a part already in order is its own place
        if keep.all() and not any(len(b) for b in blobs) and held[r].is_sorted(1):
            return held[r]
        return held[r].route(keep, blobs, own_at=r, key=1)
    return comm.each(place)


def sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff=0.7, bdelim="|", scorrect="True", level=6,
                     verbose=False, blocks=None, held=None, refs=None, keep=None, finalize=True, timings=None,
                     cuts=None, bgzf="host", inflate="host", decode="host", bgzf_effort=1, resident="host",
                     crc="host", assemble="host", names="host", out_resident="host", names_resident="host",
                     merge="host", ids="host"):
    """ids: "host" (the default) or "device": this rank's record unpacker takes its id columns and record
    flags from the engine's interner kernels (Engine.device_ids; only with decode="device").
    merge: "host" (the default) or "device": this rank's merges of sorted record sets go to the engine's
    merge kernels where every input holds its records in place (Engine.device_merge; merges of combined
    and routed views, and of more than 8 inputs, stay on the host as before).
    names_resident: "host" (the default) or "device": this rank's formatted names stay on the device
    for the assembler and its SSCS names come from the group's own buffers (Engine.device_names_resident;
    only with names="device" and assemble="device"; a rank's combined and routed views take the fetched
    blob as before).
    out_resident: "host" (the default) or "device": this rank's assembled output streams stay on
    the device for the encoder and the index (Engine.device_out_resident; only with assemble="device"
    and bgzf="device"; a rank's outputs kept in memory are downloaded as before).
    names: "host" (the default) or "device": this rank's consensus read names formatted by the
    engine's name formatter (Engine.device_names).  assemble: "host" (the default) or "device": this rank's stage outputs assembled by the engine's
    record assembler where their sources hold their records in place (Engine.device_assemble; a
    rank's combined and routed views are assembled on the host as before).
    bgzf: "host" (the default) or "device": this rank's output files deflated by the engine's BGZF
    encoder, at bgzf_effort 1 (the default) or 2 (2 needs bgzf="device").  inflate: "host" (the default) or "device": this rank's reads inflated by the engine's
    BGZF inflater.  decode: "host" (the default) or "device": this rank's stage tables built by the
    engine's record unpacker.  resident: "host" (the default) or "device": a whole-file read's inflated
    bytes stay on the device for the unpacker (Engine.device_resident; only with inflate="device" and
    decode="device", and only for whole-file opens: a rank's region reads and combined handles are
    uploaded as before).  crc: "host" (the default) or "device": this rank's device inflater and encoder
    take their CRC32s from the device (Engine.device_crc; only with inflate="device" or bgzf="device").
    These are pipeline.consensus_pipeline's options; see _sharded_pipeline."""
    if ids not in ("host", "device"):
        raise ValueError('ids must be "host" or "device"')
    if ids == "device":
        was_ids = engine.device_ids(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident, crc, assemble, names, out_resident, names_resident, merge)
        finally:
            engine.device_ids(was_ids)
    if merge not in ("host", "device"):
        raise ValueError('merge must be "host" or "device"')
    if merge == "device":
        was_mrg = engine.device_merge(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident, crc, assemble, names, out_resident, names_resident)
        finally:
            engine.device_merge(was_mrg)
    if names_resident not in ("host", "device"):
        raise ValueError('names_resident must be "host" or "device"')
    if names_resident == "device":
        was_nres = engine.device_names_resident(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident, crc, assemble, names, out_resident)
        finally:
            engine.device_names_resident(was_nres)
    if out_resident not in ("host", "device"):
        raise ValueError('out_resident must be "host" or "device"')
    if out_resident == "device":
        was_res = engine.device_out_resident(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident, crc, assemble, names)
        finally:
            engine.device_out_resident(was_res)
    if names not in ("host", "device"):
        raise ValueError('names must be "host" or "device"')
    if names == "device":
        was_names = engine.device_names(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident, crc, assemble)
        finally:
            engine.device_names(was_names)
    if assemble not in ("host", "device"):
        raise ValueError('assemble must be "host" or "device"')
    if assemble == "device":
        was_asm = engine.device_assemble(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident, crc)
        finally:
            engine.device_assemble(was_asm)
    if crc not in ("host", "device"):
        raise ValueError('crc must be "host" or "device"')
    if crc == "device":
        was_crc = engine.device_crc(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort, resident)
        finally:
            engine.device_crc(was_crc)
    if bgzf not in ("host", "device"):
        raise ValueError('bgzf must be "host" or "device"')
    if bgzf_effort not in (1, 2):
        raise ValueError("bgzf_effort must be 1 or 2")
    if bgzf_effort != 1 and bgzf != "device":
        raise ValueError('bgzf_effort=2 needs bgzf="device"')
    if inflate not in ("host", "device"):
        raise ValueError('inflate must be "host" or "device"')
    if decode not in ("host", "device"):
        raise ValueError('decode must be "host" or "device"')
    if resident not in ("host", "device"):
        raise ValueError('resident must be "host" or "device"')
    if resident == "device":
        was_res = engine.device_resident(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate, decode,
                                    bgzf_effort)
        finally:
            engine.device_resident(was_res)
    if decode == "device":
        was_dec = engine.device_decode(True)
        try:
            return sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                    blocks, held, refs, keep, finalize, timings, cuts, bgzf, inflate,
                                    bgzf_effort=bgzf_effort)
        finally:
            engine.device_decode(was_dec)
    if bgzf == "host" and inflate == "host":
        return _sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                 blocks, held, refs, keep, finalize, timings, cuts)
    was_effort = engine.bgzf_effort
    was = engine.device_bgzf(True, effort=bgzf_effort) if bgzf == "device" else None
    try:
        was_in = engine.device_inflate(True) if inflate == "device" else None
        try:
            return _sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose,
                                     blocks, held, refs, keep, finalize, timings, cuts)
        finally:
            if was_in is not None:
                engine.device_inflate(was_in)
    finally:
        if was is not None:
            engine.device_bgzf(was, effort=was_effort)


def _sharded_pipeline(bam, c_output, bedfile, comm, engine, cutoff, bdelim, scorrect, level, verbose, blocks, held,
                      refs, keep, finalize, timings, cuts):
    """ConsensusCruncher.py:127-346 with every stage split over comm.world region shards.  Same files
    and contents as pipeline.consensus_pipeline; rank 0 returns the output paths.

    Every stage output stays in memory (engine.MemorySink, in samtools-sort order as it is assembled)
    and moves to the ranks owning its positions (to_owners) for the next stage; nothing is written
    and read back between stages.  The reference's output files are written once, at the end: at
    world size 1 straight from the records (sorted, indexed, compressed in the background), at more
    ranks as a merge of the ranks' sorted parts (ties in rank order, the whole-sample sort's order).

    held / refs / blocks: the ranks' record sets are given (bench.py: per-rank generated samples, already
    at their owners) instead of read from bam through its BAI; keep: a dict that receives the stage runs
    ({stage: {rank: run}}) resident on the GPU instead of closing them; finalize=False skips the output
    files (bench.py: the stage runs are what it times); timings: a dict that receives this rank's
    host phases in seconds (bench.py's end-to-end breakdown)."""
    if bedfile in (None, "False"):
        bedfile = None   # the whole file as one region (-b False): position blocks
    world = comm.world
    root = comm.rank == 0
    if root:
        warm_plotting()   # (rank 0 draws the family-size plot after the SSCS stage)
    identifier = os.path.basename(bam).split('.bam', 1)[0]
    sd = '{}/{}'.format(c_output, identifier)
    subs = ("sscs", "dcs", "sscs_sc", "dcs_sc")
    for sub in subs:
        os.makedirs(os.path.join(sd, sub), exist_ok=True)
    if held is None:
        # the ranks read their regions through the input's BAI (rank 0 indexes it when needed)
        got = comm.each(lambda r: _indexed_input(bam, c_output) if r == 0 else None)
        bam = comm.broadcast_obj(got[0] if root else None)
        refs = Bam.open_regions(bam, [], [], []).refs
        if blocks is None and cuts is None:
            blocks = comm.broadcast_obj(region_plan(bam, bedfile, world) if root else None)
    if isinstance(blocks, dict):   # region_plan's cuts (a hot region split)
        blocks, cuts = None, blocks["cuts"]
    geo = Geometry(refs, bedfile, blocks, cuts=cuts)
    clock = [time.time()]

    def lap(name):
        if timings is not None:
            now = time.time()
            timings[name] = round(timings.get(name, 0.0) + now - clock[0], 3)
            clock[0] = now
    if held is not None and not geo.positional and geo.adjusted:
        # the given record sets were placed for `blocks`; a plan moved for overlapping regions
        # (overlap_safe_blocks) would put records at the wrong ranks
        raise ValueError("held record sets need a block plan that keeps overlapping regions together")
    start = time.time()
    P = lambda sub, name: '{}/{}/{}.{}'.format(sd, sub, identifier, name)  # noqa: E731
    srt = lambda p: '{}.sorted.bam'.format(p.split('.bam', 1)[0])  # noqa: E731
    finals = []   # (output path, {rank: sorted records}) of the reference's sorted output files

    def done(stage, r, run):
        """a stage run after its emit: kept resident (bench) or closed"""
        if keep is not None:
            keep.setdefault(stage, {})[r] = run
        else:
            run.close()

    def routed(helds, mode, delim, it_of):
        """Each rank's stage tables and streams for the record sets helds[k][r] (k: the stage's inputs)."""
        cores = comm.each(lambda r: [_Cores(h[r]) for h in helds])
        own = comm.each(lambda r: [geo.own_stream(c, r) for c in cores[r]])
        out = []
        for k, h in enumerate(helds):
            sent = comm.each(lambda r: geo.sent(cores[r][k], own[r][k], r))
            recv = comm.exchange(comm.each(lambda r: geo.routes(h[r], cores[r][k], own[r][k], r, sent[r])))
            out.append(comm.each(lambda r: geo.stage_input(h[r], own[r][k], recv[r], mode, delim, it_of[r],
                                                           sent[r][0], engine=engine)))
        return out

    def on_root(fn):
        """rank 0's host work between stages; a raise there reaches every rank (comm.each)"""
        comm.each(lambda r: fn() if r == 0 else None)

    def move(a, b):   # the stats / time-tracker moves of ConsensusCruncher.py:200-203,225-228,275-278
        os.rename(P(a, "stats.txt"), P(b, "stats.txt"))
        os.rename(P(a, "time_tracker.txt"), P(b, "time_tracker.txt"))

    def emitted(paths, fn):
        """Each rank's run of fn(rank, sink) with its outputs kept in memory: {path: {rank: Bam}} for the
        stage's output paths (the sorted ones under their sorted names) and fn's results."""
        sinks = comm.each(lambda r: MemorySink(fused=[p for p, fused in paths if fused]))
        res = comm.each(lambda r: fn(r, sinks[r]))
        out = {}
        for pth, fused in paths:
            name = srt(pth) if fused else pth
            out[name] = comm.each(lambda r: sinks[r].take(name))
        return out, res

    # ---- SSCS
    if held is None:
        held = comm.each(lambda r: Bam.open_regions(bam, *geo.block(r)))
    lap("open")
    its = comm.each(lambda r: Interner())
    (inp,) = routed([held], MODE_SSCS, bdelim, its)
    lap("sscs.route+decode")
    sscs = P("sscs", "sscs.bam")
    prefix = sscs.split('.sscs')[0]

    def sscs1(r, sink):
        table, rec, stream = inp[r]
        run = SSCSRun(engine, None, cutoff, bedfile, bdelim, src=(table, its[r], rec, stream))
        lap("sscs.gpu")
        try:
            return run.emit(sscs, level, verbose=False, side=False, plot=False, sink=sink)
        finally:
            if timings is not None:
                timings.update({"sscs." + k: round(v, 3) for k, v in run.times.items() if k.startswith("emit_")})
            done("sscs", r, run)
    outs, parts = emitted([(sscs, True), (prefix + '.singleton.bam', True), (prefix + '.badReads.bam', False)], sscs1)
    lap("sscs.emit")
    tot = comm.reduce(parts)
    bad = outs[prefix + '.badReads.bam']   # unsorted: the reference writes it in stream (rank) order
    del inp, held

    def sscs2():
        # AlignmentFile.mapped (printed in the verbose QC lines only) from the BAI's pseudo-bins;
        # without them (an index that does not write them) the whole input's mapped records are
        # counted; without the input file (bench.py's generated record sets) the mapped records the
        # ranks streamed
        tot["mapped"] = int(N.io().ccio_bai_mapped(bam.encode())) if os.path.exists(bam + ".bai") else -1
        if tot["mapped"] < 0 and verbose and os.path.exists(bam):
            tot["mapped"] = int((Bam(bam).cores()[4] & 4 == 0).sum())
        if tot["mapped"] < 0:
            tot["mapped"] = tot.get("mapped_own", -1)
        sscs_side(prefix, tot, geo.keys, start, verbose)
    on_root(sscs2)
    lap("sscs.side")
    sscs_loc = to_owners(comm, geo, outs[srt(sscs)])
    sing_loc = to_owners(comm, geo, outs[srt(prefix + '.singleton.bam')])
    lap("sscs.to_owners")
    del outs
    finals += [(P("sscs", "sscs.sorted.bam"), sscs_loc), (P("sscs", "singleton.sorted.bam"), sing_loc)]
    on_root(lambda: move("sscs", "dcs"))

    # ---- DCS (and DCS+SC below)
    def dcs_stage(src_loc, outfile):
        its_d = comm.each(lambda r: Interner())
        (din,) = routed([src_loc], MODE_DUPLEX, None, its_d)
        lap("dcs.route+decode")
        single = ('{}.sscs.sc.singleton.bam'.format(outfile.split('.dcs.sc')[0]) if '.dcs.sc' in outfile
                  else '{}.sscs.singleton.bam'.format(outfile.split('.dcs')[0]))

        def p1(r, sink):
            table, rec, stream = din[r]
            run = DCSRun(engine, None, bedfile, src=(table, its_d[r], rec, stream))
            lap("dcs.gpu")
            try:
                return run.emit(outfile, level, verbose=False, side=False, sink=sink)
            finally:
                if timings is not None and '.dcs.sc' not in outfile:
                    timings.update({"dcs." + k: round(v, 3) for k, v in run.times.items() if k.startswith("emit_")})
                done("dcs_sc" if '.dcs.sc' in outfile else "dcs", r, run)
        o, parts_ = emitted([(outfile, True), (single, True)], p1)
        lap("dcs.emit")
        t = comm.reduce(parts_)
        on_root(lambda: dcs_side(outfile, t, start, verbose))
        got = to_owners(comm, geo, o[srt(outfile)]), to_owners(comm, geo, o[srt(single)])
        lap("dcs.to_owners")
        return got

    dcs_loc, ss_loc = dcs_stage(sscs_loc, P("dcs", "dcs.bam"))
    finals += [(P("dcs", "dcs.sorted.bam"), dcs_loc), (P("dcs", "sscs.singleton.sorted.bam"), ss_loc)]
    del dcs_loc, ss_loc
    out = dict(badreads=prefix + '.badReads.bam')
    if scorrect != 'False':
        on_root(lambda: move("dcs", "sscs"))
        # ---- SC: singletons against the SSCS, both rank-local
        its_c = comm.each(lambda r: Interner())
        s_in, x_in = routed([sing_loc, sscs_loc], MODE_DUPLEX, None, its_c)
        lap("sc.route+decode")
        base = P("sscs", "singleton.sorted.bam").split('.singleton')[0]
        names = ("sscs.correction", "singleton.correction", "uncorrected")

        def sc1(r, sink):
            (st, sr, ss), (xt, xr, xs) = s_in[r], x_in[r]
            run = SCRun(engine, base + '.singleton.sorted.bam', bedfile, src=(its_c[r], (st, sr, ss), (xt, xr, xs)))
            lap("sc.gpu")
            try:
                return run.emit(level, verbose=False, side=False, sink=sink)
            finally:
                done("sc", r, run)
        o, parts_ = emitted([('{}.{}.bam'.format(base, nm), True) for nm in names], sc1)
        lap("sc.emit")
        t = comm.reduce(parts_)
        del s_in, x_in
        on_root(lambda: sc_side(base, t, verbose))
        sc_loc = {}
        for nm in names:
            sc_loc[nm] = to_owners(comm, geo, o['{}.{}.sorted.bam'.format(base, nm)])
            finals.append((P("sscs_sc", nm + ".sorted.bam"), sc_loc[nm]))
        del o
        # merge(sscs.sorted, sscs.correction.sorted, singleton.correction.sorted) + sort, per rank
        sscs_sc_loc = comm.each(lambda r: merge_kept(None, [sscs_loc[r], sc_loc["sscs.correction"][r],
                                                            sc_loc["singleton.correction"][r]], memory=True))
        finals.append((P("sscs_sc", "sscs.sc.sorted.bam"), sscs_sc_loc))
        lap("sc.to_owners+merge")
        del sscs_loc, sing_loc
        on_root(lambda: move("sscs", "dcs_sc"))
        dsc_loc, ssc_loc = dcs_stage(sscs_sc_loc, P("dcs_sc", "dcs.sc.bam"))
        au = comm.each(lambda r: merge_kept(None, [dsc_loc[r], ssc_loc[r], sc_loc["uncorrected"][r]], memory=True))
        lap("merge")
        finals += [(P("dcs_sc", "dcs.sc.sorted.bam"), dsc_loc), (P("dcs_sc", "sscs.sc.singleton.sorted.bam"), ssc_loc),
                   (P("dcs_sc", "all.unique.dcs.sorted.bam"), au)]
        del dsc_loc, ssc_loc, au, sc_loc, sscs_sc_loc

    def finish():
        if scorrect != 'False':
            os.rename(P("dcs_sc", "stats.txt"), '{}/{}.stats.txt'.format(sd, identifier))
            os.rename(P("dcs_sc", "time_tracker.txt"), '{}/{}.time_tracker.txt'.format(sd, identifier))
        else:
            os.rename(P("dcs", "stats.txt"), '{}/{}.stats.txt'.format(sd, identifier))
            os.rename(P("dcs", "time_tracker.txt"), '{}/{}.time_tracker.txt'.format(sd, identifier))
        png = '{}/sscs/{}_tag_fam_size.png'.format(sd, identifier)
        if os.path.exists(png):
            os.rename(png, '{}/{}_tag_fam_size.png'.format(sd, identifier))
        os.rename(P("sscs", "read_families.txt"), '{}/{}.read_families.txt'.format(sd, identifier))
    if finalize:
        write_outputs(comm, finals, (prefix + '.badReads.bam', bad), sd, subs, level)
        on_root(finish)
        lap("write")
    del finals, bad
    out.update(sscs=P("sscs", "sscs.sorted.bam"), singleton=P("sscs", "singleton.sorted.bam"),
               dcs=P("dcs", "dcs.sorted.bam"), sscs_singleton=P("dcs", "sscs.singleton.sorted.bam"))
    if scorrect != 'False':
        out.update(sscs_correction=P("sscs_sc", "sscs.correction.sorted.bam"),
                   singleton_correction=P("sscs_sc", "singleton.correction.sorted.bam"),
                   uncorrected=P("sscs_sc", "uncorrected.sorted.bam"), sscs_sc=P("sscs_sc", "sscs.sc.sorted.bam"),
                   dcs_sc=P("dcs_sc", "dcs.sc.sorted.bam"), sscs_sc_singleton=P("dcs_sc", "sscs.sc.singleton.sorted.bam"),
                   all_unique=P("dcs_sc", "all.unique.dcs.sorted.bam"))
    out["stats"] = '{}/{}.stats.txt'.format(sd, identifier)
    out["read_families"] = '{}/{}.read_families.txt'.format(sd, identifier)
    return out if root else None


def write_outputs(comm, finals, bad, sd, subs, level):
    """The reference's output files from the ranks' records in memory, once: the sorted outputs
    (+ .bai) merged over the ranks with ties in rank order, badReads concatenated in rank order.  With
    every rank in this process (LocalComm) or at world size 1 the files are written straight from the
    records (compressed in the background); ranks in other processes write their parts next to the
    outputs and rank 0 merges them."""
    bad_path, bad_loc = bad
    if isinstance(comm, LocalComm) or comm.world == 1:
        def one(r):
            if r != 0:
                return
            for path, loc in finals:
                if comm.world == 1:
                    loc[0].write(path, level, index=True, async_write=True)
                else:
                    merge_kept(path, [loc[k] for k in range(comm.world)], level, keep=False, async_writes=True)
            if comm.world == 1:
                bad_loc[0].write(bad_path, level, async_write=True)
            else:
                Bam.combine([bad_loc[k] for k in range(comm.world)], [], key=2).write(bad_path, level)
            flush_writes()
        comm.each(one)
        return
    # ranks in processes of their own: parts next to the outputs, merged by rank 0
    for sub in subs:
        os.makedirs(os.path.join(sd, sub, ".shard%d" % comm.rank), exist_ok=True)

    def parts(r):
        for path, loc in finals + [(bad_path, bad_loc)]:
            loc[r].write(_part(path, r), level, async_write=True)
        flush_writes()
    comm.each(parts)
    comm.barrier()

    def merge(r):
        if r != 0:
            return
        concat_bams(bad_path, [_part(bad_path, k) for k in range(comm.world)], level)
        for path, _ in finals:
            merge_bams(path, [_part(path, k) for k in range(comm.world)], level)
            index_bam(path)
        for sub in subs:
            for k in range(comm.world):
                shutil.rmtree(os.path.join(sd, sub, ".shard%d" % k), ignore_errors=True)
    comm.each(merge)


def main(argv=None):
    """`ConsensusCruncher.py consensus` (its argv :461-518; consensus() :127-346) on the GPUs of one
    node: one process per GPU under torch.distributed.run (RCCL), the stages split over the bed regions;
    a single process runs pipeline.consensus_pipeline on GPU 0.

        python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
            -m consensuscruncher_amd.sharded -i sample.sorted.bam -o out -g hg38
    """
    import argparse
    from .pipeline import cleanup, consensus_pipeline, genome_bedfile
    from .stages import get_engine
    p = argparse.ArgumentParser(prog="consensuscruncher_amd.sharded")
    p.add_argument('-i', '--input', dest='bam', required=True, type=str)
    p.add_argument('-o', '--output', dest='c_output', required=True, type=str)
    p.add_argument('--scorrect', choices=['True', 'False'], default='True')
    p.add_argument('-g', '--genome', dest='genome', choices=['hg19', 'hg38', 'hg38_noAlt'], default='hg19')
    # the reference's default bed is its bundled hg19 cytobands (ConsensusCruncher.py:413-433)
    p.add_argument('-b', '--bedfile', type=str, default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                     "data", "hg19_cytoBand.txt"))
    p.add_argument('--cutoff', type=float, default=0.7)
    p.add_argument('-d', '--bdelim', type=str, default='|')
    p.add_argument('--cleanup', choices=['True', 'False'], default='False')
    args = p.parse_args(argv)
    bedfile = genome_bedfile(args.genome, args.bedfile)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        eng = get_engine()
        consensus_pipeline(args.bam, args.c_output, bedfile=bedfile, cutoff=args.cutoff, bdelim=args.bdelim,
                           scorrect=args.scorrect, engine=eng, cleanup_files=args.cleanup)
        return
    import torch
    import torch.distributed as dist
    from .engine import Engine
    # CC_DIST_BACKEND=gloo with CC_DEVICE=k: every rank on GPU k, the reduction on the CPU (a one-GPU
    # rehearsal of the multi-GPU run; tests/test_gpu_shard.py)
    backend = os.environ.get("CC_DIST_BACKEND", "nccl")
    dev = int(os.environ["CC_DEVICE"]) if "CC_DEVICE" in os.environ else int(os.environ.get("LOCAL_RANK", "0"))
    if backend == "nccl":
        torch.cuda.set_device(dev)
    dist.init_process_group(backend)
    comm = None
    try:
        eng = Engine(dev)
        comm = TorchComm(engine=eng)
        out = sharded_pipeline(args.bam, args.c_output, bedfile, comm, eng, cutoff=args.cutoff,
                               bdelim=args.bdelim, scorrect=args.scorrect)
        if out is not None and args.cleanup == 'True':
            identifier = os.path.basename(args.bam).split('.bam', 1)[0]
            cleanup('{}/{}'.format(args.c_output, identifier), identifier, args.scorrect)
        dist.barrier()
        comm.close()
        eng.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
