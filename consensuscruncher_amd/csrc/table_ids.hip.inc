// cc_table_ids: the interned-id columns of a table's records (barcode, cigar, RG) as local ids in
// order of first occurrence, and all three rflags bits, from kernels over the raw BAM records
// (included by cc_engine.hip after table_unpack.hip.inc).  cc_table_ids_resident: the same from a
// resident stream.  The host then interns only each table's distinct strings (ccio_intern_first).
//   k_ids_keys      a record per thread: the shared parser (unpack_core.h) checks the record, the
//                   shared finders (intern_core.h) give each table's key {off, len} or none and the
//                   flags; per table the key's seeded 64-bit hash (IDS_NONE: no key), and rflags
// then per table (0 barcode, 1 cigar, 2 RG), on the same scratch buffers:
//   sort_pairs      (hash, record) by all 64 bits; stable, so a run of equal hashes is in record order
//                   and its first element is the key's first occurrence
//   k_ids_heads     flags the run heads; scan_launch numbers the runs; k_ids_headrec: head_rec[run]
//   k_ids_assign    each element compares its key bytes with its run head's (length, then bytes; all
//                   reads inside the two records): a mismatch is a hash collision (IE_COLLIDE), a
//                   head with a key sets first[record]
//   scan_launch     first[] in record order: each first occurrence's local id
//   k_ids_local     local[record] = rank[head record] (-1: none), first_rec[local id] = record
// Nothing is read through a record's lengths before k_ids_keys has accepted every record.
#include "intern_core.h"

namespace {

// IE_RANGE: an index a scan or the sort produced lay outside its array (nothing was read through it)
enum : uint32_t { IE_BAD = 1u, IE_AUX = 2u, IE_COLLIDE = 4u, IE_RANGE = 8u };
struct IdsStatus {
    uint32_t err, pad;
    unsigned long long first_bad;   // the smallest refused record index (~0: none)
    uint32_t nd[4];                 // the distinct keys per table (the scans' totals)
};
static_assert(sizeof(IdsStatus) == 32, "status layout");

constexpr int IDS_T = 256;
constexpr uint64_t IDS_NONE = ~0ULL;          // the reserved hash of a record without a key: sorts last
constexpr uint32_t IDS_NO_OFF = 0xffffffffu;  // its key offset
constexpr uint64_t IDS_SEEDS[4] = {0x243F6A8885A308D3ULL, 0x13198A2E03707344ULL, 0xA4093822299F31D0ULL,
                                   0x082EFA98EC4E6C89ULL};

// recs, shift, bytes, rec_off: as k_unpack_sizes.  hash and kl hold the tables one after the other
// (table k's record r at k * n + r).
__global__ __launch_bounds__(IDS_T) void k_ids_keys(const uint8_t* __restrict__ recs, uint64_t shift, uint64_t bytes,
                                                    const uint64_t* __restrict__ rec_off, int64_t n, int mode,
                                                    itn::Delim delim, uint64_t seed, uint64_t hmask,
                                                    uint64_t* __restrict__ hash, uint2* __restrict__ kl,
                                                    uint32_t* __restrict__ idx, uint8_t* __restrict__ rflags,
                                                    IdsStatus* st) {
    const int64_t r = (int64_t)blockIdx.x * IDS_T + threadIdx.x;
    if (r >= n) return;
    const uint64_t rel = rec_off[r];
    bool ok = rel < bytes && (r == 0 || rec_off[r - 1] < rel);
    const uint8_t* rec = recs + shift + rel;   // (read only when rel < bytes)
    upk::Rec f;
    ok = ok && upk::parse(rec, bytes - rel, f);
    uint32_t err = ok ? 0u : IE_BAD;
    itn::Key key[3];
    uint8_t rf = 0;
    if (ok) {
        key[0] = itn::barcode_key(rec, f, mode, delim);
        key[1] = itn::cigar_key(rec, f);
        key[2] = itn::rg_key(rec, f);
        if (key[2].refuse) { err = IE_AUX; ok = false; }
        rf = f.rflags | key[0].flags | key[2].flags;
    }
    idx[r] = (uint32_t)r;
    rflags[r] = rf;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint64_t h = IDS_NONE;
        uint2 ol = make_uint2(IDS_NO_OFF, 0u);
        if (ok && !key[k].none) {
            h = itn::hash_bytes(rec + key[k].off, key[k].len, seed + (uint64_t)k) & hmask;
            if (h == IDS_NONE) h = IDS_NONE - 1;
            ol = make_uint2(key[k].off, key[k].len);
        }
        hash[(int64_t)k * n + r] = h;
        kl[(int64_t)k * n + r] = ol;
    }
    if (err) {
        atomicOr(&st->err, err);
        atomicMin(&st->first_bad, (unsigned long long)r);
    }
}

__global__ __launch_bounds__(IDS_T) void k_ids_heads(const uint64_t* __restrict__ skey, int64_t n,
                                                     uint32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * IDS_T + threadIdx.x;
    if (i < n) head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1u : 0u;
}

// run = the exclusive scan of head[]: a head's own run number
__global__ __launch_bounds__(IDS_T) void k_ids_headrec(const uint32_t* __restrict__ head, const uint32_t* __restrict__ run,
                                                       const uint32_t* __restrict__ sval, int64_t n,
                                                       uint32_t* __restrict__ head_rec) {
    const int64_t i = (int64_t)blockIdx.x * IDS_T + threadIdx.x;
    if (i < n && head[i] && (int64_t)run[i] < n) head_rec[run[i]] = sval[i];
}

// sval is a permutation of 0 .. n - 1 (the sort of idx), so every record's first[] and hrec[] are
// written exactly once; run[i] - 1 < n indexes head_rec, whose entries are records.  Each of these
// is checked all the same before it indexes anything (a scan that gave up leaves garbage behind).
__global__ __launch_bounds__(IDS_T) void k_ids_assign(const uint8_t* __restrict__ recs, uint64_t shift,
                                                      const uint64_t* __restrict__ rec_off, const uint2* __restrict__ kl,
                                                      const uint32_t* __restrict__ head, const uint32_t* __restrict__ run,
                                                      const uint32_t* __restrict__ sval,
                                                      const uint32_t* __restrict__ head_rec, int64_t n,
                                                      uint32_t* __restrict__ first, uint32_t* __restrict__ hrec,
                                                      IdsStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * IDS_T + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = sval[i];
    if ((int64_t)r >= n) { atomicOr(&st->err, IE_RANGE); return; }
    const uint32_t hd = head[i];
    const uint2 a = kl[r];
    uint32_t h = r, fst = 0;
    if (a.x != IDS_NO_OFF) {
        if (hd) {
            fst = 1;
        } else {
            const uint32_t ru = run[i] - 1u;
            h = (int64_t)ru < n ? head_rec[ru] : 0xffffffffu;
            if ((int64_t)h >= n) {
                atomicOr(&st->err, IE_RANGE);
                first[r] = 0;
                hrec[r] = r;
                return;
            }
            const uint2 b = kl[h];
            bool same = b.x != IDS_NO_OFF && b.y == a.y;
            if (same) {
                const uint8_t* pa = recs + shift + rec_off[r] + a.x;
                const uint8_t* pb = recs + shift + rec_off[h] + b.x;
                for (uint32_t k = 0; k < a.y; ++k)
                    if (pa[k] != pb[k]) { same = false; break; }
            }
            if (!same) {
                atomicOr(&st->err, IE_COLLIDE);
                h = r;
            }
        }
    }
    first[r] = fst;
    hrec[r] = h;
}

// rank = the exclusive scan of first[] in record order
__global__ __launch_bounds__(IDS_T) void k_ids_local(const uint2* __restrict__ kl, const uint32_t* __restrict__ first,
                                                     const uint32_t* __restrict__ rank, const uint32_t* __restrict__ hrec,
                                                     int64_t n, int32_t* __restrict__ local, int32_t* __restrict__ first_rec,
                                                     IdsStatus* st) {
    const int64_t r = (int64_t)blockIdx.x * IDS_T + threadIdx.x;
    if (r >= n) return;
    const uint32_t h = hrec[r];
    if ((int64_t)h >= n || (first[r] && (int64_t)rank[r] >= n)) {
        atomicOr(&st->err, IE_RANGE);
        local[r] = -1;
        return;
    }
    local[r] = kl[r].x == IDS_NO_OFF ? -1 : (int32_t)rank[h];
    if (first[r]) first_rec[rank[r]] = (int32_t)r;
}

// the call's allocations, freed when it returns (nothing enqueued still uses them then)
struct IdsBufs {
    cc_ctx* ctx;
    std::vector<void*> p;
    ~IdsBufs() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* q : p) (void)hipFree(q);
    }
};

// cc_table_ids' and cc_table_ids_resident's work: the records are recs[0 .. bytes) in host memory
// (resident null: uploaded here) or the resident buffer's bytes [shift, shift + bytes).
int table_ids(cc_ctx* ctx, const uint8_t* recs, const uint8_t* resident, uint64_t shift, uint64_t bytes,
              const uint64_t* rec_off, int64_t n, int mode, const char* delim, int32_t* local_bc, int32_t* local_cigar,
              int32_t* local_rg, uint8_t* rflags, int32_t* first_bc, int32_t* first_cigar, int32_t* first_rg,
              int32_t* nd) {
    if (!ctx || !nd || n < 0) return CC_E_INVALID;
    nd[0] = nd[1] = nd[2] = 0;
    if (mode != 0 && mode != 1) { ctx->err = "cc_table_ids: mode 0 or 1"; return CC_E_INVALID; }
    if (n > 0 && ((!recs && !resident) || !rec_off || !local_bc || !local_cigar || !local_rg || !rflags || !first_bc ||
                  !first_cigar || !first_rg)) {
        ctx->err = "cc_table_ids: null argument";
        return CC_E_INVALID;
    }
    if (n > (int64_t)INT32_MAX) { ctx->err = "cc_table_ids: more than 2^31 - 1 records"; return CC_E_UNSUPPORTED; }
    itn::Delim dl{};
    const size_t dlen = delim ? strlen(delim) : 0;
    if (dlen > (size_t)itn::DELIM_MAX) {
        ctx->err = "cc_table_ids: a barcode delimiter of more than 16 bytes";
        return CC_E_UNSUPPORTED;
    }
    if (dlen) memcpy(dl.b, delim, dlen);
    dl.len = (int32_t)dlen;
    RC(enter(ctx));
    if (n == 0) return 0;
    IdsBufs bufs{ctx};
    const uint8_t* d_recs = resident;
    if (!resident) {
        uint8_t* up = nullptr;
        RC(dev_alloc(ctx, bufs.p, &up, (int64_t)bytes));
        ProfScope ps(ctx, "ids_stream_upload");
        HIPCHK(hipMemcpyAsync(up, recs, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
        d_recs = up;
    }
    uint64_t *d_off = nullptr, *hash = nullptr, *skey = nullptr;
    uint2* kl = nullptr;
    uint32_t *idx = nullptr, *sval = nullptr, *head = nullptr, *run = nullptr, *head_rec = nullptr, *first = nullptr,
             *hrec = nullptr, *rank = nullptr;
    int32_t *local = nullptr, *first_rec = nullptr;
    uint8_t* d_rf = nullptr;
    IdsStatus* d_st = nullptr;
    RC(upload(ctx, bufs.p, &d_off, rec_off, n));
    RC(dev_alloc(ctx, bufs.p, &hash, 3 * n));
    RC(dev_alloc(ctx, bufs.p, &kl, 3 * n));
    RC(dev_alloc(ctx, bufs.p, &skey, n));
    RC(dev_alloc(ctx, bufs.p, &idx, n));
    RC(dev_alloc(ctx, bufs.p, &sval, n));
    RC(dev_alloc(ctx, bufs.p, &head, n, 64));
    RC(dev_alloc(ctx, bufs.p, &run, n, 64));
    RC(dev_alloc(ctx, bufs.p, &head_rec, n));
    RC(dev_alloc(ctx, bufs.p, &first, n, 64));
    RC(dev_alloc(ctx, bufs.p, &hrec, n));
    RC(dev_alloc(ctx, bufs.p, &rank, n, 64));
    RC(dev_alloc(ctx, bufs.p, &local, 3 * n));
    RC(dev_alloc(ctx, bufs.p, &first_rec, 3 * n));
    RC(dev_alloc(ctx, bufs.p, &d_rf, n));
    RC(dev_alloc(ctx, bufs.p, &d_st, 1));
    IdsStatus* h_st = reinterpret_cast<IdsStatus*>((uint8_t*)ctx->h_pinned + 768);
    const int hb = ctx->ids_hash_bits;
    const uint64_t hmask = hb >= 64 ? ~0ULL : (1ULL << hb) - 1;
    const unsigned nb = nblk(n, IDS_T);
    EngineSwitches saved = ctx->sw;
    struct Restore { cc_ctx* c; EngineSwitches s; ~Restore() { c->sw = s; } } restore{ctx, saved};
    // a hash collision runs the call again with the next seed; a look-back scan that waited past its
    // bound runs it again with the two-launch scans (the same seed)
    for (int seed = 0; seed < 4;) {
        *h_st = IdsStatus{};
        h_st->first_bad = ~0ULL;
        HIPCHK(hipMemcpyAsync(d_st, h_st, sizeof(IdsStatus), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_err, 0, 4, ctx->stream));
        klaunch(ctx, "ids_keys", k_ids_keys, nb, IDS_T, d_recs, shift, bytes, d_off, n, mode, dl, IDS_SEEDS[seed], hmask,
                hash, kl, idx, d_rf, d_st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(IdsStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_st->err & (IE_BAD | IE_AUX)) {
            char buf[200];
            snprintf(buf, sizeof buf, "cc_table_ids: record %lld: %s", (long long)h_st->first_bad,
                     (h_st->err & IE_BAD) ? "offset out of range or out of order, or lengths that do not fit block_size "
                                            "or the stream"
                                          : "an aux value that does not lie inside the record");
            ctx->err = buf;
            return CC_E_INVALID;
        }
        for (int k = 0; k < 3; ++k) {
            RC(sort_pairs(ctx, hash + (int64_t)k * n, skey, idx, sval, n, "ids_sort"));
            klaunch(ctx, "ids_heads", k_ids_heads, nb, IDS_T, skey, n, head);
            RC(scan_launch(ctx, head, n, &d_st->nd[3], "ids_scan", ScanStore{run}));
            klaunch(ctx, "ids_heads", k_ids_headrec, nb, IDS_T, head, run, sval, n, head_rec);
            klaunch(ctx, "ids_assign", k_ids_assign, nb, IDS_T, d_recs, shift, d_off, kl + (int64_t)k * n, head, run, sval,
                    head_rec, n, first, hrec, d_st);
            RC(scan_launch(ctx, first, n, &d_st->nd[k], "ids_scan", ScanStore{rank}));
            klaunch(ctx, "ids_assign", k_ids_local, nb, IDS_T, kl + (int64_t)k * n, first, rank, hrec, n,
                    local + (int64_t)k * n, first_rec + (int64_t)k * n, d_st);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(IdsStatus), hipMemcpyDeviceToHost, ctx->stream));
        uint32_t bits = 0;
        RC(read_err(ctx, &bits));   // (waits for the stream)
        if (bits & EB_SCANWAIT) {
            if (ctx->sw.scan1 == 0) { ctx->err = "cc_table_ids: scan look-back wait bound exceeded"; return CC_E_INVALID; }
            ctx->sw.scan1 = 0;
            continue;
        }
        if (bits) return err_code(ctx, bits);
        if (h_st->err & IE_RANGE) { ctx->err = "cc_table_ids: a run or rank index outside its array"; return CC_E_INVALID; }
        if (!(h_st->err & IE_COLLIDE)) break;
        if (++seed == 4) {
            ctx->err = "cc_table_ids: 64-bit key hash collision under four seeds";
            return CC_E_COLLISION;
        }
    }
    int32_t* lo[3] = {local_bc, local_cigar, local_rg};
    int32_t* fo[3] = {first_bc, first_cigar, first_rg};
    {
        ProfScope ps(ctx, "ids_download");
        for (int k = 0; k < 3; ++k) {
            if (h_st->nd[k] > (uint64_t)n) { ctx->err = "cc_table_ids: more distinct keys than records"; return CC_E_INVALID; }
            HIPCHK(hipMemcpyAsync(lo[k], local + (int64_t)k * n, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost,
                                  ctx->stream));
            if (h_st->nd[k])
                HIPCHK(hipMemcpyAsync(fo[k], first_rec + (int64_t)k * n, sizeof(int32_t) * (size_t)h_st->nd[k],
                                      hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipMemcpyAsync(rflags, d_rf, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 3; ++k) nd[k] = (int32_t)h_st->nd[k];
    return 0;
}

}  // namespace

extern "C" {

int cc_table_ids(cc_ctx* ctx, const uint8_t* recs, uint64_t bytes, const uint64_t* rec_off, int64_t n, int mode,
                 const char* delim, int32_t* local_bc, int32_t* local_cigar, int32_t* local_rg, uint8_t* rflags,
                 int32_t* first_bc, int32_t* first_cigar, int32_t* first_rg, int32_t* nd) {
    return table_ids(ctx, recs, nullptr, 0, bytes, rec_off, n, mode, delim, local_bc, local_cigar, local_rg, rflags,
                     first_bc, first_cigar, first_rg, nd);
}

int cc_table_ids_resident(cc_ctx* ctx, int64_t id, uint64_t base, uint64_t bytes, const uint64_t* rec_off, int64_t n,
                          int mode, const char* delim, int32_t* local_bc, int32_t* local_cigar, int32_t* local_rg,
                          uint8_t* rflags, int32_t* first_bc, int32_t* first_cigar, int32_t* first_rg, int32_t* nd) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    // held throughout: the stream cannot be freed, nor the inflater run, while the kernels read it
    std::lock_guard<std::mutex> lk(E->mu);
    const Resident* R = resident_find(E, id);
    if (!R) { ctx->err = "cc_table_ids_resident: unknown id"; return CC_E_INVALID; }
    if (base > R->total || bytes > R->total - base) {
        ctx->err = "cc_table_ids_resident: the records do not lie inside the stream";
        return CC_E_INVALID;
    }
    if (E->broken) { ctx->err = E->err; return CC_E_HIP; }
    HIPCHK(hipSetDevice(ctx->device));
    for (int b = 0; b < 2; ++b)   // the inflater's and the patches' writes are done before the first kernel
        if (E->st[b]) HIPCHK(hipStreamSynchronize(E->st[b]));
    return table_ids(ctx, nullptr, R->p, base, bytes, rec_off, n, mode, delim, local_bc, local_cigar, local_rg, rflags,
                     first_bc, first_cigar, first_rg, nd);
}

// test hook: the key hashes truncated to their low `bits` bits (1 .. 64; 64 is the default), so that
// small inputs collide
int cc_debug_ids_hash_bits(cc_ctx* ctx, int32_t bits) {
    if (!ctx || bits < 1 || bits > 64) return CC_E_INVALID;
    ctx->ids_hash_bits = bits;
    return 0;
}

}  // extern "C"
