// cc_table_unpack: a table's record columns and blobs built on the device from raw BAM records
// (included by cc_engine.hip after cc_table_upload, whose result it reproduces byte for byte).
// cc_table_unpack_resident: the same from records that already lie on the device, in a resident
// stream the inflater left there (bgzf_inflate.hip.inc).
//   k_unpack_sizes  a record per thread: the shared parser (unpack_core.h) checks the record and gives
//                   its fields; the integer columns, qlen, qn_len, rflags, rdig, the slot sizes in
//                   16-B (payload) and 8-B (qname) units, and per block the largest l_seq and tid
//   scan_launch x2  the slot sizes' exclusive scans: pay_off / 16 and qn_off / 8, their totals
//   k_unpack_copy   16 lanes per record: every 16-B chunk of the payload slot and every 8-B chunk of
//                   the qname slot, padding included, from aligned loads funnel-shifted to the
//                   record's byte alignment
//   k_derive        the derived columns, as for any table uploaded without the decoder's layout
// Nothing is read through a record's lengths before the sizes kernel has accepted every record: the
// copy kernel is only launched when no error bit is set.
#include "unpack_core.h"

namespace {

enum : uint32_t { UE_BAD = 1u, UE_TOO_LONG = 2u, UE_RFLAGS = 4u };
struct UnpackStatus {
    uint32_t err, pad;
    unsigned long long first_bad;     // the smallest record index with an error bit (~0: none)
    int32_t max_len, max_tid;
    unsigned long long sum16, sum8;   // the slot sizes summed in 64 bits (the scans' totals are 32-bit)
    uint32_t tot16, tot8;             // the scans' totals
};
static_assert(sizeof(UnpackStatus) == 48, "status layout");

constexpr int UPK_T = 256;      // threads per block, both kernels
constexpr int UPK_LANES = 16;   // lanes per record in the copy kernel (a slot of L = 150 is 16 chunks)

// A record's bytes from aligned loads of the padded stream (base is 16-B aligned and at least
// align16(bytes) + 32 long, so the aligned words around any valid byte lie inside the buffer).
struct DevSrc {
    const uint8_t* base;
    uint64_t off;   // the record's block_size word
    // 16 bytes at stream offset a, bytes from `valid` (1..16) on zero
    __device__ __forceinline__ upk::W16 fetch(uint64_t a, uint32_t valid) const {
        const uint4* p = reinterpret_cast<const uint4*>(base + (a & ~15ull));
        const uint32_t sh = (uint32_t)a & 15u;
        const uint4 v0 = p[0];
        uint4 v1 = make_uint4(0u, 0u, 0u, 0u);
        if (sh + valid > 16u) v1 = p[1];
        // shift by whole words (two select stages), then by bytes (alignbyte)
        const bool s2 = (sh & 8u) != 0, s1 = (sh & 4u) != 0;
        const uint32_t x0 = s2 ? v0.z : v0.x, x1 = s2 ? v0.w : v0.y, x2 = s2 ? v1.x : v0.z, x3 = s2 ? v1.y : v0.w,
                       x4 = s2 ? v1.z : v1.x, x5 = s2 ? v1.w : v1.y;
        const uint32_t y0 = s1 ? x1 : x0, y1 = s1 ? x2 : x1, y2 = s1 ? x3 : x2, y3 = s1 ? x4 : x3, y4 = s1 ? x5 : x4;
        const uint32_t bsh = sh & 3u;
        upk::W16 o;
        o.w[0] = __builtin_amdgcn_alignbyte(y1, y0, bsh);
        o.w[1] = __builtin_amdgcn_alignbyte(y2, y1, bsh);
        o.w[2] = __builtin_amdgcn_alignbyte(y3, y2, bsh);
        o.w[3] = __builtin_amdgcn_alignbyte(y4, y3, bsh);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int32_t nb = (int32_t)valid - 4 * i;
            o.w[i] = nb >= 4 ? o.w[i] : (nb <= 0 ? 0u : (o.w[i] & ((1u << (8 * nb)) - 1u)));
        }
        return o;
    }
    __device__ __forceinline__ upk::W16 bytes16(uint32_t i, uint32_t valid) const { return fetch(off + i, valid); }
    __device__ __forceinline__ upk::W8 bytes8(uint32_t i, uint32_t valid) const {
        const upk::W16 w = fetch(off + i, valid);
        return upk::W8{{w.w[0], w.w[1]}};
    }
    // 8 bytes at record core offset i, bytes from `valid` (0..8) on zero
    __device__ __forceinline__ uint64_t word(uint32_t i, uint32_t valid) const {
        if (valid == 0) return 0;
        const uint64_t a = off + 4 + i;
        const uint64_t* p = reinterpret_cast<const uint64_t*>(base + (a & ~7ull));
        const uint32_t sh = ((uint32_t)a & 7u) * 8u;
        uint64_t w = p[0] >> sh;
        if (sh + 8u * valid > 64u) w |= p[1] << (64u - sh);   // (sh > 0 here)
        return valid >= 8 ? w : (w & ((1ULL << (8 * valid)) - 1ULL));
    }
};

// recs is the 16-B aligned base of the padded buffer; the records are its bytes [shift, shift + bytes)
// and rec_off counts from shift (0 for an uploaded stream, the first record's offset in a resident one)
__global__ __launch_bounds__(UPK_T) void k_unpack_sizes(const uint8_t* __restrict__ recs, uint64_t shift, uint64_t bytes,
                                                        const uint64_t* __restrict__ rec_off, int64_t n,
                                                        const uint8_t* __restrict__ rf_host, DevTable T,
                                                        uint32_t* __restrict__ sz16, uint32_t* __restrict__ sz8,
                                                        UnpackStatus* st) {
    __shared__ int s_len, s_tid;
    __shared__ uint32_t s_err;
    __shared__ unsigned long long s_16, s_8;
    if (threadIdx.x == 0) { s_len = 0; s_tid = -1; s_err = 0; s_16 = 0; s_8 = 0; }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * UPK_T + threadIdx.x;
    if (r < n) {
        const uint64_t rel = rec_off[r];
        bool ok = rel < bytes && (r == 0 || rec_off[r - 1] < rel);
        const uint64_t off = shift + rel;   // (used only when rel < bytes)
        upk::Rec f;
        ok = ok && upk::parse(recs + off, bytes - rel, f);
        uint32_t err = ok ? 0u : UE_BAD, p16 = 0, q8 = 0;
        if (ok && f.lseq > 0xffff) { err = UE_TOO_LONG; ok = false; }
        if (ok) {
            const uint8_t rfl = rf_host[r];
            if ((rfl & upk::RF_QUAL_MISSING) != f.rflags) err = UE_RFLAGS;
            T.tid[r] = f.tid; T.pos[r] = f.pos; T.mtid[r] = f.mtid; T.mpos[r] = f.mpos; T.tlen[r] = f.tlen;
            T.flag[r] = (uint16_t)f.flag;
            T.mapq[r] = (uint8_t)f.mapq;
            T.lseq[r] = f.lseq;
            T.qlen[r] = f.qlen;
            T.qn_len[r] = (uint16_t)f.qn_len;
            T.rflags[r] = rfl | f.rflags;
            T.rdig[r] = upk::rec_digest(DevSrc{recs, off}, f.bs);
            p16 = (uint32_t)(upk::pay_slot(f.lseq) >> 4);
            q8 = upk::qn_slot((uint32_t)f.l_read_name) >> 3;
            atomicMax(&s_len, f.lseq);
            atomicMax(&s_tid, f.tid);
            atomicAdd(&s_16, (unsigned long long)p16);
            atomicAdd(&s_8, (unsigned long long)q8);
        }
        sz16[r] = p16;
        sz8[r] = q8;
        if (err) {
            atomicOr(&s_err, err);
            atomicMin(&st->first_bad, (unsigned long long)r);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_err) atomicOr(&st->err, s_err);
        atomicMax(&st->max_len, s_len);
        atomicMax(&st->max_tid, s_tid);
        atomicAdd(&st->sum16, s_16);
        atomicAdd(&st->sum8, s_8);
    }
}

// UPK_LANES lanes per record, UPK_T / UPK_LANES records per block; every record was accepted by
// k_unpack_sizes, and off16 / off8 are the scans of the sizes it wrote, so each slot lies in its blob.
__global__ __launch_bounds__(UPK_T) void k_unpack_copy(const uint8_t* __restrict__ recs, uint64_t shift,
                                                       const uint64_t* __restrict__ rec_off, int64_t n, DevTable T,
                                                       const uint32_t* __restrict__ off16,
                                                       const uint32_t* __restrict__ off8) {
    const int64_t r = (int64_t)blockIdx.x * (UPK_T / UPK_LANES) + (threadIdx.x / UPK_LANES);
    const uint32_t j = threadIdx.x % UPK_LANES;
    if (r >= n) return;
    const uint64_t off = shift + rec_off[r];
    const int32_t lseq = T.lseq[r];
    const int32_t qn_len = T.qn_len[r];
    const uint8_t* rec = recs + off;
    const uint32_t lqn = rec[12], ncig = (uint32_t)rec[16] | ((uint32_t)rec[17] << 8);
    const uint32_t seq_off = 36u + lqn + 4u * ncig, qual_off = seq_off + (uint32_t)((lseq + 1) / 2);
    const uint64_t po = (uint64_t)off16[r] << 4, qo = (uint64_t)off8[r] << 3;
    if (j == 0) {
        T.pay_off[r] = po;
        T.qn_off[r] = qo;
    }
    const DevSrc s{recs, off};
    const uint32_t np = (uint32_t)(upk::pay_slot(lseq) >> 4);
    uint4* pd = reinterpret_cast<uint4*>(T.payload + po);
    for (uint32_t c = j; c < np; c += UPK_LANES) {
        const upk::W16 w = upk::pay_chunk(s, qual_off, seq_off, lseq, c);
        pd[c] = make_uint4(w.w[0], w.w[1], w.w[2], w.w[3]);
    }
    const uint32_t nq = upk::qn_slot(lqn) >> 3;
    uint2* qd = reinterpret_cast<uint2*>(T.qn_blob + qo);
    for (uint32_t c = j; c < nq; c += UPK_LANES) {
        const upk::W8 w = upk::qn_chunk(s, qn_len, c);
        qd[c] = make_uint2(w.w[0], w.w[1]);
    }
}

// the call's allocations: the temporaries always freed, the table's unless the call succeeded
struct UnpackGuard {
    cc_ctx* ctx;
    int32_t id;
    std::vector<void*> tmp;
    bool keep = false;
    ~UnpackGuard() {
        (void)hipStreamSynchronize(ctx->stream);   // nothing enqueued still uses them
        for (void* p : tmp) (void)hipFree(p);
        if (!keep) {
            for (void* p : ctx->table_allocs[id]) (void)hipFree(p);
            ctx->table_allocs.erase(id);
        }
    }
};

template <class T>
int dev_alloc(cc_ctx* ctx, std::vector<void*>& allocs, T** dst, int64_t count, size_t extra = 0) {
    HIPCHK(hipMalloc((void**)dst, (size_t)std::max<int64_t>(count, 1) * sizeof(T) + extra));
    allocs.push_back(*dst);
    return 0;
}

// cc_table_unpack's and cc_table_unpack_resident's work.  The records are either recs[0 .. bytes) in
// host memory (resident null: uploaded here into a padded buffer of the call's own) or the resident
// buffer's bytes [shift, shift + bytes), read in place.
int table_unpack(cc_ctx* ctx, const uint8_t* recs, const uint8_t* resident, uint64_t shift, uint64_t bytes,
                 const uint64_t* rec_off, int64_t n, const int32_t* cigar_id, const int32_t* bc_id, const int32_t* rg_id,
                 const uint8_t* rflags, int32_t* max_len, int32_t* table_id) {
    if (!ctx || !max_len || !table_id || n < 0) return CC_E_INVALID;
    if (n > 0 && ((!recs && !resident) || !rec_off || !cigar_id || !bc_id || !rg_id || !rflags)) {
        ctx->err = "cc_table_unpack: null argument";
        return CC_E_INVALID;
    }
    if (n > (int64_t)INT32_MAX) { ctx->err = "cc_table_unpack: more than 2^31 - 1 records"; return CC_E_UNSUPPORTED; }
    RC(enter(ctx));
    const int32_t id = ctx->next_id++;
    std::vector<void*>& al = ctx->table_allocs[id];
    UnpackGuard guard{ctx, id};
    DevTable T{};
    T.guard = ctx->d_err + ERR_GUARD;
    T.n = n;
    RC(dev_alloc(ctx, al, &T.tid, n));
    RC(dev_alloc(ctx, al, &T.pos, n));
    RC(dev_alloc(ctx, al, &T.mtid, n));
    RC(dev_alloc(ctx, al, &T.mpos, n));
    RC(dev_alloc(ctx, al, &T.tlen, n));
    RC(dev_alloc(ctx, al, &T.flag, n));
    RC(dev_alloc(ctx, al, &T.mapq, n));
    RC(upload(ctx, al, &T.cig, cigar_id, n));
    RC(dev_alloc(ctx, al, &T.qlen, n));
    RC(dev_alloc(ctx, al, &T.lseq, n));
    RC(upload(ctx, al, &T.bc, bc_id, n));
    RC(upload(ctx, al, &T.rg, rg_id, n));
    RC(dev_alloc(ctx, al, &T.rflags, n));
    RC(dev_alloc(ctx, al, &T.qn_off, n));
    RC(dev_alloc(ctx, al, &T.qn_len, n));
    RC(dev_alloc(ctx, al, &T.qn_ol, n));
    RC(dev_alloc(ctx, al, &T.pay_off, n));
    RC(dev_alloc(ctx, al, &T.rdig, n));
    UnpackStatus* h_st = reinterpret_cast<UnpackStatus*>((uint8_t*)ctx->h_pinned + 768);
    *h_st = UnpackStatus{};
    h_st->first_bad = ~0ULL;
    h_st->max_tid = -1;
    const uint8_t* d_recs = resident;
    uint8_t* d_rf = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t *sz16 = nullptr, *sz8 = nullptr, *off16 = nullptr, *off8 = nullptr;
    if (n > 0) {
        if (!resident) {
            // the stream, padded so the aligned 16-B words around its last bytes lie inside the buffer
            const size_t padded = (size_t)((bytes + 15) & ~15ull) + 32;
            uint8_t* up = nullptr;
            RC(dev_alloc(ctx, guard.tmp, &up, (int64_t)padded));
            ProfScope ps(ctx, "unpack_stream_upload");
            HIPCHK(hipMemcpyAsync(up, recs, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemsetAsync(up + bytes, 0, padded - (size_t)bytes, ctx->stream));
            d_recs = up;
        }
        RC(upload(ctx, guard.tmp, &d_off, rec_off, n));
        RC(upload(ctx, guard.tmp, &d_rf, rflags, n));
        RC(dev_alloc(ctx, guard.tmp, &sz16, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &sz8, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &off16, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &off8, n, 64));
        UnpackStatus* d_st = nullptr;
        RC(dev_alloc(ctx, guard.tmp, &d_st, 1));
        HIPCHK(hipMemcpyAsync(d_st, h_st, sizeof(UnpackStatus), hipMemcpyHostToDevice, ctx->stream));
        klaunch(ctx, "k_unpack_sizes", k_unpack_sizes, nblk(n, UPK_T), UPK_T, d_recs, shift, bytes, d_off, n, d_rf, T, sz16,
                sz8, d_st);
        HIPCHK(hipGetLastError());
        RC(scan_launch(ctx, sz16, n, &d_st->tot16, "unpack_scan_pay", ScanStore{off16}));
        RC(scan_launch(ctx, sz8, n, &d_st->tot8, "unpack_scan_qn", ScanStore{off8}));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(UnpackStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_st->err & (UE_BAD | UE_RFLAGS)) {
            char buf[200];
            snprintf(buf, sizeof buf, "cc_table_unpack: record %lld: %s", (long long)h_st->first_bad,
                     (h_st->err & UE_BAD) ? "offset out of range or out of order, or lengths that do not fit block_size "
                                            "or the stream"
                                          : "rflags' CC_RF_QUAL_MISSING bit disagrees with the record");
            ctx->err = buf;
            return CC_E_INVALID;
        }
        if ((h_st->err & UE_TOO_LONG) || h_st->sum16 > 0xffffffffULL || h_st->sum8 > 0xffffffffULL) {
            ctx->err = "record too long for the 16-bit length fields or payload > 64 GiB";
            return CC_E_UNSUPPORTED;
        }
        if (h_st->sum16 != h_st->tot16 || h_st->sum8 != h_st->tot8) {
            ctx->err = "cc_table_unpack: the slot offsets' scan total does not match the sizes";
            return CC_E_INVALID;
        }
    }
    T.pay_bytes = (uint64_t)h_st->tot16 << 4;
    T.qn_bytes = (uint64_t)h_st->tot8 << 3;
    T.max_len = h_st->max_len;
    T.ntid = h_st->max_tid + 1;
    // the blobs with the tails the upload path gives them (+64 / +16), the tails zeroed
    RC(dev_alloc(ctx, al, &T.qn_blob, (int64_t)T.qn_bytes + 16));
    RC(dev_alloc(ctx, al, &T.payload, (int64_t)T.pay_bytes + 64));
    HIPCHK(hipMemsetAsync(T.qn_blob + T.qn_bytes, 0, 16, ctx->stream));
    HIPCHK(hipMemsetAsync(T.payload + T.pay_bytes, 0, 64, ctx->stream));
    if (n > 0) {
        klaunch(ctx, "k_unpack_copy", k_unpack_copy, nblk(n, UPK_T / UPK_LANES), UPK_T, d_recs, shift, d_off, n, T, off16, off8);
        HIPCHK(hipGetLastError());
    }
    // the derived columns: as cc_table_upload without the decoder's layout
    T.qdig_mask = ctx->sw.qdig_bits ? (1ULL << ctx->sw.qdig_bits) - 1 : ~0ULL;
    T.host_layout = false;
    RC(dev_alloc(ctx, al, &T.core, n));
    RC(dev_alloc(ctx, al, &T.meta, n));
    RC(dev_alloc(ctx, al, &T.rkey, n));
    RC(dev_alloc(ctx, al, &T.qdig, n));
    RC(dev_alloc(ctx, al, &T.rdeep, n));
    RC(dev_alloc(ctx, al, &T.dlist, n / DEEP_MIN + 2));
    RC(dev_alloc(ctx, al, &T.ndeep, 4));
    RC(dev_alloc(ctx, al, &T.ebits, 4));
    HIPCHK(hipMemsetAsync(T.ebits, 0, 16, ctx->stream));
    T.n_deep = 0;
    T.derive_pending = false;
    T.bkt_cap = std::max<int64_t>(2 * n + T.ntid, 2 * (int64_t)T.ntid) + 2;
    RC(dev_alloc(ctx, al, &T.ext, std::max(T.ntid, 1)));
    RC(dev_alloc(ctx, al, &T.tbase, T.ntid + 1));
    RC(dev_alloc(ctx, al, &T.geom, 4));
    HIPCHK(hipMemsetAsync(T.ext, 0, sizeof(int32_t) * std::max(T.ntid, 1), ctx->stream));
    RC(derive_table(ctx, T));
    if (n > 0) {
        uint32_t* h_nd = reinterpret_cast<uint32_t*>(h_st + 1);
        HIPCHK(hipMemcpyAsync(h_nd, T.ndeep, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        T.n_deep = *h_nd;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the uploads read caller memory
    if (ctx->sw.trace_upload)
        fprintf(stderr, "[cc] table %d: %lld records, %lld deep groups, unpacked on the device\n", id, (long long)T.n,
                (long long)T.n_deep);
    ctx->tables[id] = T;
    guard.keep = true;
    *max_len = T.max_len;
    *table_id = id;
    return 0;
}

}  // namespace

extern "C" {

int cc_table_unpack(cc_ctx* ctx, const uint8_t* recs, uint64_t bytes, const uint64_t* rec_off, int64_t n,
                    const int32_t* cigar_id, const int32_t* bc_id, const int32_t* rg_id, const uint8_t* rflags,
                    int32_t* max_len, int32_t* table_id) {
    return table_unpack(ctx, recs, nullptr, 0, bytes, rec_off, n, cigar_id, bc_id, rg_id, rflags, max_len, table_id);
}

int cc_table_unpack_resident(cc_ctx* ctx, int64_t id, uint64_t base, uint64_t bytes, const uint64_t* rec_off, int64_t n,
                             const int32_t* cigar_id, const int32_t* bc_id, const int32_t* rg_id, const uint8_t* rflags,
                             int32_t* max_len, int32_t* table_id) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    // held throughout: the stream cannot be freed, nor the inflater run, while the kernels read it
    std::lock_guard<std::mutex> lk(E->mu);
    const Resident* R = resident_find(E, id);
    if (!R) { ctx->err = "cc_table_unpack_resident: unknown id"; return CC_E_INVALID; }
    if (base > R->total || bytes > R->total - base) {
        ctx->err = "cc_table_unpack_resident: the records do not lie inside the stream";
        return CC_E_INVALID;
    }
    if (E->broken) { ctx->err = E->err; return CC_E_HIP; }
    HIPCHK(hipSetDevice(ctx->device));
    for (int b = 0; b < 2; ++b)   // the inflater's and the patches' writes are done before the first kernel
        if (E->st[b]) HIPCHK(hipStreamSynchronize(E->st[b]));
    return table_unpack(ctx, nullptr, R->p, base, bytes, rec_off, n, cigar_id, bc_id, rg_id, rflags, max_len, table_id);
}

}  // extern "C"
