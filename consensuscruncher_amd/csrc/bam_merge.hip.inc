// cc_bam_merge: the merge of up to MRG_MAX_SRC coordinate-sorted record sets (samtools merge stand-in)
// built on the device, byte for byte what ccio_merge_handles gathers on the host (included by
// cc_engine.hip after bam_assemble.hip.inc, whose sources, upload and copy body it shares).  Sorted
// inputs need no sort: a record's place is its index in its own input plus its rank in every other
// input (merge_core.h's place rule).
//   k_merge_keys   a record per thread: the shared check (merge_core.h) accepts the record and gives
//                  its 64-bit key and 32-bit size; each key is compared with its predecessor's in the
//                  same source; the status block gets the first refused record, the first record
//                  out of order, the largest record and the 64-bit byte total
//   k_merge_rank   blocks of MRG_TILE consecutive records of one source (a block never straddles two:
//                  block -> source goes through the prefix table in the arguments).  For each other
//                  source the block bisects once for the window [lower(first key), upper(last key)),
//                  stages it in one reused LDS buffer when it holds at most MRG_WIN keys and bisects
//                  there, else bisects global memory inside the window; org[dest] = concatenation index
//   k_merge_sizes  a slice's sizes in output order
//   scan_launch    their exclusive scan: the slice's 32-bit offsets (the host carries the 64-bit base)
//   k_merge_copy   16 lanes per output record: k_asm_copy's body over the record's source bytes
// Nothing is read through a record's length before the keys kernel has accepted every record: the
// later kernels are only launched when the status is clean.
#include "merge_core.h"

namespace {

using mrg::MRG_MAX_SRC;
using mrg::MRG_TILE;
using mrg::MRG_WIN;

struct MrgStatus {
    unsigned long long first_bad;   // (concatenation index << 8 | refusal code) of the first refused record (~0: none)
    unsigned long long first_ooo;   // concatenation index of the first record whose key is below its predecessor's (~0: none)
    unsigned long long total;       // the sizes summed in 64 bits
    uint32_t max_size, guard;       // guard: an index or offset outside its bounds in the later kernels (never expected)
    uint32_t tot, pad;              // the last scan's total
};
static_assert(sizeof(MrgStatus) == 40, "status layout");
static_assert(MRG_TILE % 64 == 0 && MRG_TILE <= 1024, "a rank block is whole waves");

// where the sources' records and rank blocks begin: source s holds concatenation indices
// [rec[s], rec[s + 1]) and blocks [blk[s], blk[s + 1]); the entries from nsrc on repeat the totals
struct MrgPre {
    int64_t rec[MRG_MAX_SRC + 1];
    int64_t blk[MRG_MAX_SRC + 1];
    int32_t nsrc, pad;
};
// the source whose range of `first` holds x (x below first[MRG_MAX_SRC]; empty sources hold nothing)
__device__ __forceinline__ int mrg_src_of(const int64_t* first, int64_t x) {
    int s = 0;
#pragma unroll
    for (int k = 1; k < MRG_MAX_SRC; ++k) s += x >= first[k] ? 1 : 0;
    return s;
}

__global__ __launch_bounds__(ASM_T) void k_merge_keys(const asmb::Src* __restrict__ src, MrgPre P, int64_t n,
                                                      uint64_t* __restrict__ key, uint32_t* __restrict__ sz, MrgStatus* st) {
    __shared__ unsigned long long s_bad, s_ooo, s_tot;
    __shared__ uint32_t s_max;
    __shared__ uint64_t s_key[ASM_T];
    __shared__ uint8_t s_ok[ASM_T];
    if (threadIdx.x == 0) { s_bad = ~0ULL; s_ooo = ~0ULL; s_tot = 0; s_max = 0; }
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * ASM_T + threadIdx.x;
    bool ok = false;
    uint64_t k = 0;
    int64_t li = 0;
    int s = 0;
    if (g < n) {
        s = mrg_src_of(P.rec, g);
        li = g - P.rec[s];
        const asmb::Src S = src[s];
        uint32_t size = 0;
        const uint32_t e = mrg::record<DevFetch>(S.base, S.shift, S.bytes, S.rec_off[li], &size, &k);
        if (e) {
            atomicMin(&s_bad, ((unsigned long long)g << 8) | e);
            size = 0;
            k = 0;
        } else {
            ok = true;
            atomicAdd(&s_tot, (unsigned long long)size);
            atomicMax(&s_max, size);
        }
        sz[g] = size;
        key[g] = k;
    }
    s_key[threadIdx.x] = k;
    s_ok[threadIdx.x] = ok ? 1 : 0;
    __syncthreads();
    if (ok && li > 0) {   // the predecessor in the same source: the thread before, or the block before's last
        uint64_t pk = 0;
        bool pok;
        if (threadIdx.x > 0) {
            pk = s_key[threadIdx.x - 1];
            pok = s_ok[threadIdx.x - 1] != 0;
        } else {
            const asmb::Src S = src[s];
            uint32_t psize = 0;
            pok = mrg::record<DevFetch>(S.base, S.shift, S.bytes, S.rec_off[li - 1], &psize, &pk) == 0;
        }
        if (pok && k < pk) atomicMin(&s_ooo, (unsigned long long)g);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad != ~0ULL) atomicMin(&st->first_bad, s_bad);
        if (s_ooo != ~0ULL) atomicMin(&st->first_ooo, s_ooo);
        atomicAdd(&st->total, s_tot);
        atomicMax(&st->max_size, s_max);
    }
}

// Every source passed k_merge_keys: its keys are non-decreasing.
__global__ __launch_bounds__(MRG_TILE) void k_merge_rank(MrgPre P, int64_t n, const uint64_t* __restrict__ key,
                                                         uint32_t* __restrict__ org, MrgStatus* st) {
    __shared__ uint64_t s_win[MRG_WIN];
    __shared__ int64_t s_lo, s_hi;
    const int64_t b = blockIdx.x;
    const int s = mrg_src_of(P.blk, b);
    const int64_t n_s = P.rec[s + 1] - P.rec[s];
    const int64_t i0 = (b - P.blk[s]) * MRG_TILE, i1 = min(i0 + (int64_t)MRG_TILE, n_s);
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < i1;
    if (i0 >= i1) return;   // (the whole block: no block is launched for an empty tile)
    const uint64_t* ks = key + P.rec[s];
    const uint64_t kf = ks[i0], kl = ks[i1 - 1], k = in ? ks[i] : 0;
    int64_t d = i;
    for (int s2 = 0; s2 < P.nsrc; ++s2) {
        const int64_t n2 = P.rec[s2 + 1] - P.rec[s2];
        if (s2 == s || n2 == 0) continue;   // (the same for the whole block)
        const uint64_t* k2 = key + P.rec[s2];
        if (threadIdx.x == 0) {
            s_lo = mrg::lower(k2, 0, n2, kf);
            s_hi = mrg::upper(k2, 0, n2, kl);
        }
        __syncthreads();
        const int64_t lo = s_lo, hi = s_hi, w = hi - lo;
        if (w <= MRG_WIN) {
            for (int64_t c = threadIdx.x; c < w; c += MRG_TILE) s_win[c] = k2[lo + c];
            __syncthreads();
            if (in) d += lo + (s2 < s ? mrg::upper(s_win, 0, w, k) : mrg::lower(s_win, 0, w, k));
        } else if (in) {
            d += s2 < s ? mrg::upper(k2, lo, hi, k) : mrg::lower(k2, lo, hi, k);
        }
        __syncthreads();   // the window and its bounds are reused
    }
    if (!in) return;
    if (d < 0 || d >= n) { atomicOr(&st->guard, 1u); return; }   // (never expected)
    org[d] = (uint32_t)(P.rec[s] + i);
}

// ssz[i] = the size of output record o0 + i
__global__ __launch_bounds__(ASM_T) void k_merge_sizes(const uint32_t* __restrict__ sz, const uint32_t* __restrict__ org,
                                                       int64_t n, int64_t o0, int64_t cnt, uint32_t* __restrict__ ssz,
                                                       MrgStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * ASM_T + threadIdx.x;
    if (i >= cnt) return;
    const int64_t g = org[o0 + i];
    if (g >= n) { atomicOr(&st->guard, 1u); ssz[i] = 0; return; }
    ssz[i] = sz[g];
}

// Output records [o0, o0 + cnt): record o0 + i goes to out[base + off32[i] ...).  Every record was accepted
// by k_merge_keys and off32 is the scan of the sizes it wrote, so each record lies inside out[0, total).
__global__ __launch_bounds__(ASM_T) void k_merge_copy(const asmb::Src* __restrict__ src, MrgPre P, int64_t n,
                                                      const uint32_t* __restrict__ org, const uint32_t* __restrict__ sz,
                                                      int64_t o0, int64_t cnt, const uint32_t* __restrict__ off32,
                                                      uint64_t base, uint64_t total, uint8_t* __restrict__ out,
                                                      uint64_t* __restrict__ at, MrgStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * (ASM_T / ASM_LANES) + (threadIdx.x / ASM_LANES);
    const uint32_t j = threadIdx.x % ASM_LANES;
    if (i >= cnt) return;
    const int64_t o = o0 + i;
    const int64_t g = org[o];
    const uint64_t off = base + off32[i];
    const uint32_t size = g < n ? sz[g] : 0u;
    if (g >= n || size < 36u || off > total || size > total - off) {   // (containment: never expected)
        if (j == 0) atomicOr(&st->guard, 1u);
        return;
    }
    if (j == 0) {
        at[o] = off;
        if (o == n - 1) at[n] = off + size;
    }
    const int s = mrg_src_of(P.rec, g);
    const asmb::Src S = src[s];
    const uint64_t rec = S.shift + S.rec_off[g - P.rec[s]];
    asm_copy_record(out + off, (uint32_t)off, size, j,
                    [&](uint32_t a, uint32_t valid) { return DevFetch::fetch(S.base, rec + a, valid); });
}

const char* mrg_refusal(uint32_t code) {
    if (code == mrg::ME_OFF) return "its offset lies outside the source";
    if (code == mrg::ME_SHORT) return "fewer than 4 bytes left for its block_size";
    if (code == mrg::ME_BS) return "block_size < 32";
    return "it runs past the source's bytes";
}

// cc_bam_merge's work, in bam_assemble's shape: the stream's buffer comes from alloc(actx, total) once
// the sizes are known (null alloc without keep: a size query); the caller holds the encoder's mutex
// when a source is resident or with keep, which receives the stream's own padded buffer on success.
int bam_merge(cc_ctx* ctx, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
              const std::vector<const uint8_t*>& resident, cc_asm_alloc_fn alloc, void* actx, uint64_t* at, uint32_t* org,
              uint64_t* total, Resident* keep = nullptr) {
    MrgPre P{};
    int64_t n = 0, nb = 0;
    for (int32_t f = 0; f <= MRG_MAX_SRC; ++f) {
        P.rec[f] = n;
        P.blk[f] = nb;
        if (f < nsrc) {
            n += srcs[f].nrec;
            nb += (srcs[f].nrec + MRG_TILE - 1) / MRG_TILE;
            if (n > (int64_t)INT32_MAX) { ctx->err = "cc_bam_merge: more than 2^31 - 1 records"; return CC_E_UNSUPPORTED; }
        }
    }
    P.nsrc = nsrc;
    RC(enter(ctx));
    AsmGuard guard{ctx};
    MrgStatus* h_st = reinterpret_cast<MrgStatus*>((uint8_t*)ctx->h_pinned + 768);
    *h_st = MrgStatus{};
    h_st->first_bad = h_st->first_ooo = ~0ULL;
    uint64_t sum = header_bytes;
    asmb::Src* d_src = nullptr;
    uint32_t *sz = nullptr, *d_org = nullptr, *ssz = nullptr, *off32 = nullptr;
    uint64_t* key = nullptr;
    MrgStatus* d_st = nullptr;
    if (n > 0) {
        std::vector<asmb::Src> hs((size_t)nsrc);
        for (int32_t f = 0; f < nsrc; ++f) {
            const cc_asm_src& s = srcs[f];
            asmb::Src& d = hs[(size_t)f];
            d.bytes = s.bytes;
            d.nrec = s.nrec;
            if (resident[(size_t)f]) {
                d.base = resident[(size_t)f];
                d.shift = s.base;
            } else {
                ProfScope ps(ctx, "mrg_stream_upload");
                RC(asm_upload_padded(ctx, guard.tmp, &d.base, s.stream, s.bytes));
                d.shift = 0;
            }
            uint64_t* ro = nullptr;
            RC(upload(ctx, guard.tmp, &ro, s.rec_off, s.nrec));
            d.rec_off = ro;
        }
        RC(upload(ctx, guard.tmp, &d_src, hs.data(), (int64_t)hs.size()));
        RC(dev_alloc(ctx, guard.tmp, &sz, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &key, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &d_st, 1));
        HIPCHK(hipMemcpyAsync(d_st, h_st, sizeof(MrgStatus), hipMemcpyHostToDevice, ctx->stream));
        klaunch(ctx, "k_merge_keys", k_merge_keys, nblk(n, ASM_T), ASM_T, d_src, P, n, key, sz, d_st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(MrgStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_st->first_bad != ~0ULL || h_st->first_ooo != ~0ULL) {
            const bool bad = h_st->first_bad != ~0ULL;
            const int64_t g = (int64_t)(bad ? h_st->first_bad >> 8 : h_st->first_ooo);
            int s = 0;
            while (s + 1 < nsrc && g >= P.rec[s + 1]) ++s;
            char buf[240];
            if (bad)
                snprintf(buf, sizeof buf, "cc_bam_merge: source %d record %lld: %s", s, (long long)(g - P.rec[s]),
                         mrg_refusal((uint32_t)(h_st->first_bad & 0xff)));
            else
                snprintf(buf, sizeof buf, "cc_bam_merge: source %d record %lld: its key is below the record's before it (the source is not in key order)",
                         s, (long long)(g - P.rec[s]));
            ctx->err = buf;
            return CC_E_INVALID;
        }
        sum += h_st->total;
    }
    if (total) *total = sum;
    if (!alloc && !keep) return 0;   // a size query
    uint8_t* out = alloc ? alloc(actx, sum) : nullptr;
    if ((alloc && !out) || !at) { ctx->err = "cc_bam_merge: no buffer for the stream"; return CC_E_INVALID; }
    at[0] = header_bytes;
    uint8_t* d_out = nullptr;
    if (keep) {   // `sum` usable bytes, the bytes behind them zero (the resident streams' contract)
        const size_t padded = (size_t)((sum + 15) & ~15ull) + 32;
        HIPCHK(hipMalloc((void**)&guard.kept, padded));
        d_out = guard.kept;
        HIPCHK(hipMemsetAsync(d_out + sum, 0, padded - (size_t)sum, ctx->stream));
    }
    if (n == 0) {
        if (header_bytes && out) memcpy(out, header, (size_t)header_bytes);
        if (keep) {
            if (header_bytes) HIPCHK(hipMemcpyAsync(d_out, header, (size_t)header_bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            *keep = Resident{guard.kept, sum};
            guard.kept = nullptr;
        }
        return 0;
    }
    RC(dev_alloc(ctx, guard.tmp, &d_org, n, 64));
    klaunch(ctx, "k_merge_rank", k_merge_rank, (unsigned)nb, MRG_TILE, P, n, key, d_org, d_st);
    HIPCHK(hipGetLastError());
    // the slices: at most `bound` bytes of records each, so a slice's scan total fits 32 bits
    uint64_t bound = 0xffffffffull;
    if (const char* e = getenv("CC_ASM_SLICE_BYTES")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v > 0 && v < bound) bound = v;
    }
    const int64_t per = asmb::slice_records(bound, h_st->max_size);
    const int64_t cap = std::min(per, n);
    RC(dev_alloc(ctx, guard.tmp, &ssz, cap, 64));
    RC(dev_alloc(ctx, guard.tmp, &off32, cap, 64));
    if (!keep) RC(dev_alloc(ctx, guard.tmp, &d_out, (int64_t)sum, 64));
    uint64_t* d_at = nullptr;
    RC(dev_alloc(ctx, guard.tmp, &d_at, n + 1));
    if (header_bytes) HIPCHK(hipMemcpyAsync(d_out, header, (size_t)header_bytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t base = header_bytes;
    for (int64_t o0 = 0; o0 < n; o0 += per) {
        const int64_t cnt = std::min(per, n - o0);
        klaunch(ctx, "k_merge_sizes", k_merge_sizes, nblk(cnt, ASM_T), ASM_T, sz, d_org, n, o0, cnt, ssz, d_st);
        RC(scan_launch(ctx, ssz, cnt, &d_st->tot, "mrg_scan", ScanStore{off32}));
        klaunch(ctx, "k_merge_copy", k_merge_copy, nblk(cnt, ASM_T / ASM_LANES), ASM_T, d_src, P, n, d_org, sz, o0, cnt, off32,
                base, sum, d_out, d_at, d_st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(MrgStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_st->guard) { ctx->err = "cc_bam_merge: a record outside the stream (guarded)"; return CC_E_INVALID; }
        base += h_st->tot;
    }
    if (base != sum) { ctx->err = "cc_bam_merge: the offsets' scan totals do not match the sizes"; return CC_E_INVALID; }
    if (out) {
        ProfScope ps(ctx, "mrg_download");
        HIPCHK(hipMemcpyAsync(out, d_out, (size_t)sum, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(at, d_at, sizeof(uint64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (org) HIPCHK(hipMemcpyAsync(org, d_org, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (keep) {
        *keep = Resident{guard.kept, sum};
        guard.kept = nullptr;
    }
    return 0;
}

// the arguments checked, the resident sources found (under the encoder's mutex, held until the kernels are done);
// with rid the stream stays on the device, registered in the resident table under *rid (0 after any error)
int bam_merge_locked(cc_ctx* ctx, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                     cc_asm_alloc_fn alloc, void* actx, uint64_t* at, uint32_t* org, uint64_t* total, int64_t* rid = nullptr) {
    if (rid) *rid = 0;
    if (!ctx) return CC_E_INVALID;
    if (nsrc < 0 || (header_bytes && !header) || (nsrc > 0 && !srcs)) {
        ctx->err = "cc_bam_merge: null or negative argument";
        return CC_E_INVALID;
    }
    if (nsrc > MRG_MAX_SRC) { ctx->err = "cc_bam_merge: more than 8 sources"; return CC_E_UNSUPPORTED; }
    std::vector<const uint8_t*> resident((size_t)nsrc, nullptr);
    bool any = false;
    for (int32_t f = 0; f < nsrc; ++f) {
        const cc_asm_src& s = srcs[f];
        if (s.nrec < 0 || (s.nrec > 0 && !s.rec_off) || (!s.stream && !s.resident_id && s.bytes)) {
            ctx->err = "cc_bam_merge: a source without a stream";
            return CC_E_INVALID;
        }
        any = any || s.resident_id;
    }
    if (!any && !rid) return bam_merge(ctx, header, header_bytes, srcs, nsrc, resident, alloc, actx, at, org, total);
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    for (int32_t f = 0; f < nsrc; ++f) {
        const cc_asm_src& s = srcs[f];
        if (!s.resident_id) continue;
        const Resident* R = resident_find(E, s.resident_id);
        if (!R && s.stream) continue;   // freed since: the host stream is uploaded
        if (!R) { ctx->err = "cc_bam_merge: unknown resident id"; return CC_E_INVALID; }
        if (s.base > R->total || s.bytes > R->total - s.base) {
            ctx->err = "cc_bam_merge: the records do not lie inside the resident stream";
            return CC_E_INVALID;
        }
        resident[(size_t)f] = R->p;
    }
    if (E->broken) { ctx->err = E->err; return CC_E_HIP; }   // after a HIP error on the encoder's latch nothing more starts
    HIPCHK(hipSetDevice(ctx->device));
    for (int b = 0; b < 2; ++b)   // the inflater's and the patches' writes are done before the first kernel
        if (E->st[b]) HIPCHK(hipStreamSynchronize(E->st[b]));
    if (!rid) return bam_merge(ctx, header, header_bytes, srcs, nsrc, resident, alloc, actx, at, org, total);
    Resident R;
    RC(bam_merge(ctx, header, header_bytes, srcs, nsrc, resident, alloc, actx, at, org, total, &R));
    if (!E->dec) E->dec = new BgzfDec();   // the table's home (its coder buffers are made by the first inflate)
    *rid = g_resident_next.fetch_add(1);
    E->dec->res[*rid] = R;
    return 0;
}

// libccio's merge hooks (ccio_set_merge_hooks): any failure is a nonzero return, after which libccio
// goes on to its next path
int mrg_hook_fn(void* user, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                cc_asm_alloc_fn alloc, void* actx, uint64_t* at, uint32_t* org, uint64_t* total) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (!ctx || !alloc) return CC_E_INVALID;
    return bam_merge_locked(ctx, header, header_bytes, srcs, nsrc, alloc, actx, at, org, total);
}

int mrg_hook_keep_fn(void* user, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                     cc_asm_alloc_fn alloc, void* actx, int need_host, uint64_t* at, uint32_t* org, uint64_t* total,
                     int64_t* token) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (!ctx || !token || !at || !total || (need_host && !alloc)) return CC_E_INVALID;
    return bam_merge_locked(ctx, header, header_bytes, srcs, nsrc, need_host ? alloc : nullptr, actx, at, org, total, token);
}

}  // namespace

extern "C" {

int cc_bam_merge(cc_ctx* ctx, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                 uint8_t* out, uint64_t cap, uint64_t* at, uint32_t* org, uint64_t* total) {
    AsmFixed f{out, cap};
    const int rc = bam_merge_locked(ctx, header, header_bytes, srcs, nsrc, out ? asm_fixed_alloc : nullptr, &f, at, org, total);
    if (rc == CC_E_INVALID && out && total && *total > cap && ctx) ctx->err = "cc_bam_merge: the buffer is smaller than the stream";
    return rc;
}

int cc_bam_merge_keep(cc_ctx* ctx, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                      uint8_t* out, uint64_t cap, uint64_t* at, uint32_t* org, uint64_t* total, int64_t* resident_id) {
    if (!ctx || !resident_id) return CC_E_INVALID;
    *resident_id = 0;
    if (!at || !total) { ctx->err = "cc_bam_merge_keep: at and total are required"; return CC_E_INVALID; }
    *total = 0;
    AsmFixed f{out, cap};
    const int rc = bam_merge_locked(ctx, header, header_bytes, srcs, nsrc, out ? asm_fixed_alloc : nullptr, &f, at, org, total,
                                    resident_id);
    if (rc == CC_E_INVALID && out && *total > cap) ctx->err = "cc_bam_merge_keep: the buffer is smaller than the stream";
    return rc;
}

int cc_bam_merge_hooks(cc_ctx* ctx, ccio_merge_fn* merge, ccio_merge_keep_fn* keep, void** user) {
    if (!ctx || !merge || !keep || !user) return CC_E_INVALID;
    *merge = mrg_hook_fn;
    *keep = mrg_hook_keep_fn;
    *user = ctx;
    return 0;
}

}  // extern "C"
