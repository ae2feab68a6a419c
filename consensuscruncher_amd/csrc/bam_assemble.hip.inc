// cc_bam_assemble: a stage's output BAM stream (header, then records) built on the device from
// cc_out_spec, byte for byte what ccio_write_bam_ex assembles on the host (included by cc_engine.hip
// after table_unpack.hip.inc, whose DevSrc it reads its sources with).
//   k_asm_sizes   a spec per thread: the shared layout (assemble_core.h) checks the spec and gives its
//                 output size and samtools-sort key; the status block gets the first refused spec, the
//                 largest record, the 64-bit byte total and the OR of the keys
//   sort_pairs    CCIO_W_SORT: (key, spec index), stable, over the digits the keys use
//   k_asm_gather  a slice's sizes in output order
//   scan_launch   their exclusive scan: the slice's 32-bit offsets (the host carries the 64-bit base)
//   k_asm_copy    16 lanes per output record: the head up to the output's next 16-byte line and the
//                 tail behind the last whole line as single bytes, the lines between as aligned
//                 16-byte stores; no lane writes a byte that is not its record's
// Nothing is read through a spec's lengths before the sizes kernel has accepted every spec: the
// copy kernel is only launched when no error bit is set.
#include "assemble_core.h"

namespace {

static_assert(sizeof(asmb::Spec) == sizeof(cc_out_spec), "asmb::Spec is cc_out_spec");
static_assert(sizeof(asmb::Src) == 40 && sizeof(cc_asm_src) == 48, "source layouts");

struct AsmStatus {
    unsigned long long first_bad;   // (spec index << 8 | its refusal bits) of the first refused spec (~0: none)
    unsigned long long total;       // the sizes summed in 64 bits
    unsigned long long key_or;      // OR of every key: the digits the sort needs
    uint32_t max_size, guard;       // guard: a copy-kernel index or offset outside its bounds (never expected)
    uint32_t tot, pad;              // the last scan's total
};
static_assert(sizeof(AsmStatus) == 40, "status layout");

constexpr int ASM_T = 256;      // threads per block, all kernels
constexpr int ASM_LANES = 16;   // lanes per record in the copy kernel

struct DevFetch {
    static __device__ __forceinline__ upk::W16 fetch(const uint8_t* base, uint64_t a, uint32_t valid) {
        return DevSrc{base, 0}.fetch(a, valid);
    }
};

__global__ __launch_bounds__(ASM_T) void k_asm_sizes(asmb::Tables T, const asmb::Spec* __restrict__ spec, int64_t n,
                                                     uint32_t* __restrict__ sz, uint64_t* __restrict__ key,
                                                     uint32_t* __restrict__ val, AsmStatus* st) {
    __shared__ unsigned long long s_bad, s_tot, s_or;
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) { s_bad = ~0ULL; s_tot = 0; s_or = 0; s_max = 0; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * ASM_T + threadIdx.x;
    if (i < n) {
        asmb::Lay y;
        uint64_t k = 0;
        const uint32_t e = asmb::layout(spec[i], T, y, &k);
        if (e) {
            atomicMin(&s_bad, ((unsigned long long)i << 8) | e);
            y.size = 0;
            k = 0;
        } else {
            atomicAdd(&s_tot, (unsigned long long)y.size);
            atomicOr(&s_or, (unsigned long long)k);
            atomicMax(&s_max, y.size);
        }
        sz[i] = y.size;
        key[i] = k;
        val[i] = (uint32_t)i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad != ~0ULL) atomicMin(&st->first_bad, s_bad);
        atomicAdd(&st->total, s_tot);
        atomicOr(&st->key_or, s_or);
        atomicMax(&st->max_size, s_max);
    }
}

// ssz[i] = the size of output record o0 + i (perm null: spec order)
__global__ __launch_bounds__(ASM_T) void k_asm_gather(const uint32_t* __restrict__ sz, const uint32_t* __restrict__ perm,
                                                      int64_t n, int64_t o0, int64_t cnt, uint32_t* __restrict__ ssz,
                                                      AsmStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * ASM_T + threadIdx.x;
    if (i >= cnt) return;
    const int64_t s = perm ? (int64_t)perm[o0 + i] : o0 + i;
    ssz[i] = sz[CC_IDXG(s, n, DS_REC, &st->guard)];
}

// Lane j's (of ASM_LANES) part of one output record of `size` bytes at d, whose stream offset's low
// bits are off_lo: the head up to the stream's next 16-byte line and the tail behind the last whole
// line as single bytes, the lines between as aligned 16-byte stores; no lane writes a byte outside
// d[0, size).  w16(a, valid): the record's bytes [a, a + valid), zero from `valid` on.  (k_asm_copy's
// and k_merge_copy's body.)
template <class W16Of>
__device__ __forceinline__ void asm_copy_record(uint8_t* d, uint32_t off_lo, uint32_t size, uint32_t j, W16Of w16) {
    const uint32_t head = min(size, (16u - (off_lo & 15u)) & 15u);
    const uint32_t lines = (size - head) >> 4, tail_at = head + (lines << 4);
    if (j < head) d[j] = (uint8_t)w16(j, 1u).w[0];
    uint4* dl = reinterpret_cast<uint4*>(d + head);
    for (uint32_t c = j; c < lines; c += ASM_LANES) {
        const upk::W16 w = w16(head + (c << 4), 16u);
        dl[c] = make_uint4(w.w[0], w.w[1], w.w[2], w.w[3]);
    }
    if (tail_at + j < size) d[tail_at + j] = (uint8_t)w16(tail_at + j, 1u).w[0];
}

// Output records [o0, o0 + cnt): record o0 + i goes to out[base + off32[i] ...).  Every spec was accepted
// by k_asm_sizes and off32 is the scan of the sizes it wrote, so each record lies inside out[0, total).
__global__ __launch_bounds__(ASM_T) void k_asm_copy(asmb::Tables T, const asmb::Spec* __restrict__ spec,
                                                    const uint32_t* __restrict__ perm, int64_t n, int64_t o0, int64_t cnt,
                                                    const uint32_t* __restrict__ off32, uint64_t base, uint64_t total,
                                                    uint8_t* __restrict__ out, uint64_t* __restrict__ at, AsmStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * (ASM_T / ASM_LANES) + (threadIdx.x / ASM_LANES);
    const uint32_t j = threadIdx.x % ASM_LANES;
    if (i >= cnt) return;
    const int64_t o = o0 + i;
    const int64_t s = perm ? (int64_t)perm[o] : o;
    asmb::Lay y;
    uint64_t k;
    const uint32_t e = asmb::layout(spec[CC_IDXG(s, n, DS_REC, &st->guard)], T, y, &k);
    const uint64_t off = base + off32[i];
    if (e || off > total || y.size > total - off || (uint64_t)s >= (uint64_t)n) {   // (containment: never expected)
        if (j == 0) atomicOr(&st->guard, 1u);
        return;
    }
    if (j == 0) {
        at[o] = off;
        if (o == n - 1) at[n] = off + y.size;
    }
    asm_copy_record(out + off, (uint32_t)off, y.size, j,
                    [&](uint32_t a, uint32_t valid) { return asmb::out16<DevFetch>(y, T, a, valid); });
}

struct AsmGuard {
    cc_ctx* ctx;
    std::vector<void*> tmp;
    uint8_t* kept = nullptr;   // cc_bam_assemble_keep's stream until the call has succeeded
    ~AsmGuard() {
        (void)hipStreamSynchronize(ctx->stream);   // nothing enqueued still uses them
        for (void* p : tmp) (void)hipFree(p);
        if (kept) (void)hipFree(kept);
    }
};

// host bytes in a 16-B aligned device buffer padded so the aligned words around its last bytes lie inside it
int asm_upload_padded(cc_ctx* ctx, std::vector<void*>& tmp, const uint8_t** dst, const void* src, uint64_t bytes) {
    const size_t padded = (size_t)((bytes + 15) & ~15ull) + 32;
    uint8_t* up = nullptr;
    RC(dev_alloc(ctx, tmp, &up, (int64_t)padded));
    if (bytes) HIPCHK(hipMemcpyAsync(up, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(up + bytes, 0, padded - (size_t)bytes, ctx->stream));
    *dst = up;
    return 0;
}

const char* asm_refusal(uint32_t bits) {
    if (bits & asmb::AE_KIND) return "unknown kind";
    if (bits & asmb::AE_SRC) return "src_file or src_rec out of range";
    if (bits & asmb::AE_TMPL) return "a template whose l_read_name, n_cigar and l_seq do not fit its block_size or its stream";
    if (bits & asmb::AE_NAME) return "name_id out of range";
    if (bits & asmb::AE_LONGNAME) return "a new name longer than 254 bytes";
    if (bits & asmb::AE_CONS) return "cons_off + cons_len outside the consensus arrays";
    return "rg_id outside the RG table";
}

struct AsmArgs {
    const uint8_t* header;
    uint64_t header_bytes;
    const cc_asm_src* srcs;
    int32_t nsrc;
    const cc_out_spec* spec;
    int64_t n;
    const char* names;
    const int64_t* name_off;
    int64_t n_names;
    uint64_t names_bytes;
    const uint8_t* cons_seq;
    uint64_t cons_seq_bytes;
    const uint8_t* cons_qual;
    uint64_t cons_qual_bytes;
    int32_t cons_group;
    const char* rg_blob;
    const int64_t* rg_off;
    int32_t n_rg;
    int flags;
    int64_t names_set = 0;   // a name set read in place of `names` (asm_names_of; 0: the host names)
};

// The name set a call reads: the one cc_bam_assemble_names selected, when the call brings no names of
// its own (names null, names_bytes > 0).  The selection is not consumed: a stage writes several files
// from one set.
int64_t asm_names_of(cc_ctx* ctx, const char* names, uint64_t names_bytes) {
    return ctx && !names && names_bytes > 0 ? ctx->asm_names : 0;
}

// cc_bam_assemble's work.  The stream's buffer comes from alloc(actx, total) once the sizes are known
// (null alloc: a size query, null result: CC_E_INVALID); the caller holds the encoder's mutex when a
// source is resident.  With keep (cc_bam_assemble_keep; the caller holds the mutex) the stream is built
// in a buffer of its own with a resident stream's padding, which *keep receives when the call
// succeeds; it is downloaded only when alloc is given.
int bam_assemble(cc_ctx* ctx, const AsmArgs& a, const std::vector<const uint8_t*>& resident, cc_asm_alloc_fn alloc,
                 void* actx, uint64_t* at, uint64_t* total, Resident* keep = nullptr) {
    const int64_t n = a.n;
    if (n > (int64_t)INT32_MAX) { ctx->err = "cc_bam_assemble: more than 2^31 - 1 records"; return CC_E_UNSUPPORTED; }
    RC(enter(ctx));
    AsmGuard guard{ctx};
    AsmStatus* h_st = reinterpret_cast<AsmStatus*>((uint8_t*)ctx->h_pinned + 768);
    *h_st = AsmStatus{};
    h_st->first_bad = ~0ULL;
    uint64_t sum = a.header_bytes;
    asmb::Tables T{};
    asmb::Spec* d_spec = nullptr;
    uint32_t *sz = nullptr, *val = nullptr, *perm = nullptr, *ssz = nullptr, *off32 = nullptr;
    uint64_t *key = nullptr, *key2 = nullptr;
    AsmStatus* d_st = nullptr;
    if (n > 0) {
        // the tables the specs index: sources, names, consensus arrays, RG values
        std::vector<asmb::Src> hs((size_t)std::max(a.nsrc, 1));
        for (int32_t f = 0; f < a.nsrc; ++f) {
            const cc_asm_src& s = a.srcs[f];
            asmb::Src& d = hs[(size_t)f];
            d.bytes = s.bytes;
            d.nrec = s.nrec;
            if (resident[(size_t)f]) {
                d.base = resident[(size_t)f];
                d.shift = s.base;
            } else {
                ProfScope ps(ctx, "asm_stream_upload");
                RC(asm_upload_padded(ctx, guard.tmp, &d.base, s.stream, s.bytes));
                d.shift = 0;
            }
            uint64_t* ro = nullptr;
            RC(upload(ctx, guard.tmp, &ro, s.rec_off, s.nrec));
            d.rec_off = ro;
        }
        asmb::Src* d_src = nullptr;
        RC(upload(ctx, guard.tmp, &d_src, hs.data(), (int64_t)hs.size()));
        T.src = d_src;
        T.nsrc = a.nsrc;
        T.n_names = a.n_names;
        T.names_bytes = a.names_bytes;
        if (a.names_set) {   // the set's blob and offsets where they lie (bam_assemble_locked checked its extents)
            const NameSet& s = ctx->name_sets[a.names_set];
            T.names = s.blob;
            T.name_off = s.off;
        } else {
            auto names_up = [&]() -> int {
                RC(asm_upload_padded(ctx, guard.tmp, &T.names, a.names, a.names_bytes));
                int64_t* no = nullptr;
                RC(upload(ctx, guard.tmp, &no, a.name_off, a.n_names > 0 ? a.n_names + 1 : 0));
                T.name_off = no;
                return 0;
            };
            if (a.names_bytes) {
                ProfScope ps(ctx, "asm_names_upload");
                RC(names_up());
            } else {
                RC(names_up());
            }
        }
        if (a.cons_group >= 0) {
            Group& g = *ctx->groups[a.cons_group];
            // (the buffers are hipMalloc's own allocations: 16-B aligned, and the aligned words around
            //  their last used bytes lie inside the allocation's granule)
            T.cons_seq = g.ptr<B::cons_seq>();
            T.cons_qual = g.ptr<B::cons_qual>();
            T.cons_seq_bytes = T.cons_seq ? g.buf[(int)B::cons_seq].used : 0;
            T.cons_qual_bytes = T.cons_qual ? g.buf[(int)B::cons_qual].used : 0;
        } else {
            ProfScope ps(ctx, "asm_cons_upload");
            RC(asm_upload_padded(ctx, guard.tmp, &T.cons_seq, a.cons_seq, a.cons_seq_bytes));
            RC(asm_upload_padded(ctx, guard.tmp, &T.cons_qual, a.cons_qual, a.cons_qual_bytes));
            T.cons_seq_bytes = a.cons_seq_bytes;
            T.cons_qual_bytes = a.cons_qual_bytes;
        }
        T.n_rg = a.n_rg;
        T.rg_bytes = a.n_rg > 0 ? (uint64_t)std::max<int64_t>(a.rg_off[a.n_rg], 0) : 0;
        RC(asm_upload_padded(ctx, guard.tmp, &T.rg, a.rg_blob, T.rg_bytes));
        int64_t* ro = nullptr;
        RC(upload(ctx, guard.tmp, &ro, a.rg_off, a.n_rg > 0 ? a.n_rg + 1 : 0));
        T.rg_off = ro;
        RC(upload(ctx, guard.tmp, &d_spec, reinterpret_cast<const asmb::Spec*>(a.spec), n));
        RC(dev_alloc(ctx, guard.tmp, &sz, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &val, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &key, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &d_st, 1));
        HIPCHK(hipMemcpyAsync(d_st, h_st, sizeof(AsmStatus), hipMemcpyHostToDevice, ctx->stream));
        klaunch(ctx, "k_asm_sizes", k_asm_sizes, nblk(n, ASM_T), ASM_T, T, d_spec, n, sz, key, val, d_st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(AsmStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_st->first_bad != ~0ULL) {
            char buf[240];
            snprintf(buf, sizeof buf, "cc_bam_assemble: spec %lld: %s", (long long)(h_st->first_bad >> 8),
                     asm_refusal((uint32_t)(h_st->first_bad & 0xff)));
            ctx->err = buf;
            return CC_E_INVALID;
        }
        sum += h_st->total;
    }
    if (total) *total = sum;
    if (!alloc && !keep) return 0;   // a size query
    uint8_t* out = alloc ? alloc(actx, sum) : nullptr;
    if ((alloc && !out) || !at) { ctx->err = "cc_bam_assemble: no buffer for the stream"; return CC_E_INVALID; }
    at[0] = a.header_bytes;
    uint8_t* d_out = nullptr;
    if (keep) {   // `sum` usable bytes, the bytes behind them zero (the resident streams' contract)
        const size_t padded = (size_t)((sum + 15) & ~15ull) + 32;
        HIPCHK(hipMalloc((void**)&guard.kept, padded));
        d_out = guard.kept;
        HIPCHK(hipMemsetAsync(d_out + sum, 0, padded - (size_t)sum, ctx->stream));
    }
    if (n == 0) {
        if (a.header_bytes && out) memcpy(out, a.header, (size_t)a.header_bytes);
        if (keep) {
            if (a.header_bytes) HIPCHK(hipMemcpyAsync(d_out, a.header, (size_t)a.header_bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            *keep = Resident{guard.kept, sum};
            guard.kept = nullptr;
        }
        return 0;
    }
    if (a.flags & CCIO_W_SORT) {
        unsigned b0 = 0, b1 = 0;
        asmb::key_digits(h_st->key_or, &b0, &b1);
        RC(dev_alloc(ctx, guard.tmp, &key2, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &perm, n, 64));
        RC(sort_pairs(ctx, key, key2, val, perm, n, "asm_sort", b0, b1));
    }
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
    if (a.header_bytes) HIPCHK(hipMemcpyAsync(d_out, a.header, (size_t)a.header_bytes, hipMemcpyHostToDevice, ctx->stream));
    uint64_t base = a.header_bytes;
    for (int64_t o0 = 0; o0 < n; o0 += per) {
        const int64_t cnt = std::min(per, n - o0);
        klaunch(ctx, "k_asm_gather", k_asm_gather, nblk(cnt, ASM_T), ASM_T, sz, perm, n, o0, cnt, ssz, d_st);
        RC(scan_launch(ctx, ssz, cnt, &d_st->tot, "asm_scan", ScanStore{off32}));
        klaunch(ctx, "k_asm_copy", k_asm_copy, nblk(cnt, ASM_T / ASM_LANES), ASM_T, T, d_spec, perm, n, o0, cnt, off32, base, sum,
                d_out, d_at, d_st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(AsmStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_st->guard) { ctx->err = "cc_bam_assemble: a record outside the stream (guarded)"; return CC_E_INVALID; }
        base += h_st->tot;
    }
    if (base != sum) { ctx->err = "cc_bam_assemble: the offsets' scan totals do not match the sizes"; return CC_E_INVALID; }
    if (out) {
        ProfScope ps(ctx, "asm_download");
        HIPCHK(hipMemcpyAsync(out, d_out, (size_t)sum, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(at, d_at, sizeof(uint64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, ctx->stream));
    } else {   // a kept stream nobody wants on the host: the offsets alone
        HIPCHK(hipMemcpyAsync(at, d_at, sizeof(uint64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (keep) {
        *keep = Resident{guard.kept, sum};
        guard.kept = nullptr;
    }
    return 0;
}

// the arguments checked, the resident sources found (under the encoder's mutex, held until the kernels are done);
// with rid the stream stays on the device, registered in the resident table under *rid (0 after any error)
int bam_assemble_locked(cc_ctx* ctx, const AsmArgs& a, cc_asm_alloc_fn alloc, void* actx, uint64_t* at, uint64_t* total,
                        int64_t* rid = nullptr) {
    if (rid) *rid = 0;
    if (!ctx) return CC_E_INVALID;
    if (a.n < 0 || a.nsrc < 0 || a.n_names < 0 || a.n_rg < 0 || (a.header_bytes && !a.header) ||
        (a.n > 0 && (!a.spec || (a.nsrc > 0 && !a.srcs))) || (a.n_names > 0 && !a.name_off && !a.names_set) || (a.names_bytes && !a.names && !a.names_set) ||
        (a.n_rg > 0 && (!a.rg_off || !a.rg_blob)) ||
        (a.cons_group < 0 && ((a.cons_seq_bytes && !a.cons_seq) || (a.cons_qual_bytes && !a.cons_qual)))) {
        ctx->err = "cc_bam_assemble: null or negative argument";
        return CC_E_INVALID;
    }
    if (a.cons_group >= 0 && !ctx->groups.count(a.cons_group)) { ctx->err = "cc_bam_assemble: unknown group"; return CC_E_INVALID; }
    if (a.names_set) {
        const auto it = ctx->name_sets.find(a.names_set);
        if (it == ctx->name_sets.end()) { ctx->err = "cc_bam_assemble: unknown name set"; return CC_E_INVALID; }
        if (a.n_names > it->second.n || a.names_bytes > (uint64_t)it->second.total) {
            ctx->err = "cc_bam_assemble: n_names or names_bytes larger than the name set's";
            return CC_E_INVALID;
        }
    }
    std::vector<const uint8_t*> resident((size_t)a.nsrc, nullptr);
    bool any = false;
    for (int32_t f = 0; f < a.nsrc; ++f) {
        const cc_asm_src& s = a.srcs[f];
        if (s.nrec < 0 || (s.nrec > 0 && !s.rec_off) || (!s.stream && !s.resident_id && s.bytes)) {
            ctx->err = "cc_bam_assemble: a source without a stream";
            return CC_E_INVALID;
        }
        any = any || s.resident_id;
    }
    if (!any && !rid) return bam_assemble(ctx, a, resident, alloc, actx, at, total);
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    for (int32_t f = 0; f < a.nsrc; ++f) {
        const cc_asm_src& s = a.srcs[f];
        if (!s.resident_id) continue;
        const Resident* R = resident_find(E, s.resident_id);
        if (!R && s.stream) continue;   // freed since (the unpacker consumed it): the host stream is uploaded
        if (!R) { ctx->err = "cc_bam_assemble: unknown resident id"; return CC_E_INVALID; }
        if (s.base > R->total || s.bytes > R->total - s.base) {
            ctx->err = "cc_bam_assemble: the records do not lie inside the resident stream";
            return CC_E_INVALID;
        }
        resident[(size_t)f] = R->p;
    }
    if (E->broken) { ctx->err = E->err; return CC_E_HIP; }
    HIPCHK(hipSetDevice(ctx->device));
    for (int b = 0; b < 2; ++b)   // the inflater's and the patches' writes are done before the first kernel
        if (E->st[b]) HIPCHK(hipStreamSynchronize(E->st[b]));
    if (!rid) return bam_assemble(ctx, a, resident, alloc, actx, at, total);
    Resident R;
    RC(bam_assemble(ctx, a, resident, alloc, actx, at, total, &R));
    if (!E->dec) E->dec = new BgzfDec();   // the table's home (its coder buffers are made by the first inflate)
    *rid = g_resident_next.fetch_add(1);
    E->dec->res[*rid] = R;
    return 0;
}

struct AsmFixed {
    uint8_t* out;
    uint64_t cap;
};
uint8_t* asm_fixed_alloc(void* actx, uint64_t total) {
    AsmFixed* f = static_cast<AsmFixed*>(actx);
    return total <= f->cap ? f->out : nullptr;
}

// libccio's assemble hook: the consensus arrays are the host's, or (both null) the group named by the
// last cc_bam_assemble_group, which the call consumes
int asm_hook_fn(void* user, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                const cc_out_spec* spec, int64_t n, const char* names, const int64_t* name_off, int64_t n_names,
                uint64_t names_bytes, const uint8_t* cons_seq, uint64_t cons_seq_bytes, const uint8_t* cons_qual,
                uint64_t cons_qual_bytes, const char* rg_blob, const int64_t* rg_off, int32_t n_rg, int flags,
                cc_asm_alloc_fn alloc, void* actx, uint64_t* at, uint64_t* total) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    int32_t group = -1;
    if (!cons_seq && !cons_qual) {
        group = ctx->asm_group;
        ctx->asm_group = -1;
    }
    AsmArgs a{header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
              cons_seq_bytes, cons_qual, cons_qual_bytes, group, rg_blob, rg_off, n_rg, flags};
    a.names_set = asm_names_of(ctx, names, names_bytes);
    if (!alloc) return CC_E_INVALID;
    return bam_assemble_locked(ctx, a, alloc, actx, at, total);
}

}  // namespace

extern "C" {

int cc_bam_assemble(cc_ctx* ctx, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                    const cc_out_spec* spec, int64_t n, const char* names, const int64_t* name_off, int64_t n_names,
                    uint64_t names_bytes, const uint8_t* cons_seq, uint64_t cons_seq_bytes, const uint8_t* cons_qual,
                    uint64_t cons_qual_bytes, int32_t cons_group, const char* rg_blob, const int64_t* rg_off, int32_t n_rg,
                    int flags, uint8_t* out, uint64_t cap, uint64_t* at, uint64_t* total) {
    AsmArgs a{header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
              cons_seq_bytes, cons_qual, cons_qual_bytes, cons_group, rg_blob, rg_off, n_rg, flags};
    a.names_set = asm_names_of(ctx, names, names_bytes);
    AsmFixed f{out, cap};
    const int rc = bam_assemble_locked(ctx, a, out ? asm_fixed_alloc : nullptr, &f, at, total);
    if (rc == CC_E_INVALID && out && total && *total > cap && ctx) ctx->err = "cc_bam_assemble: the buffer is smaller than the stream";
    return rc;
}

int cc_bam_assemble_keep(cc_ctx* ctx, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                         const cc_out_spec* spec, int64_t n, const char* names, const int64_t* name_off, int64_t n_names,
                         uint64_t names_bytes, const uint8_t* cons_seq, uint64_t cons_seq_bytes, const uint8_t* cons_qual,
                         uint64_t cons_qual_bytes, int32_t cons_group, const char* rg_blob, const int64_t* rg_off, int32_t n_rg,
                         int flags, uint8_t* out, uint64_t cap, uint64_t* at, uint64_t* total, int64_t* resident_id) {
    if (!ctx || !resident_id) return CC_E_INVALID;
    *resident_id = 0;
    if (!at || !total) { ctx->err = "cc_bam_assemble_keep: at and total are required"; return CC_E_INVALID; }
    *total = 0;
    AsmArgs a{header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
              cons_seq_bytes, cons_qual, cons_qual_bytes, cons_group, rg_blob, rg_off, n_rg, flags};
    a.names_set = asm_names_of(ctx, names, names_bytes);
    AsmFixed f{out, cap};
    const int rc = bam_assemble_locked(ctx, a, out ? asm_fixed_alloc : nullptr, &f, at, total, resident_id);
    if (rc == CC_E_INVALID && out && *total > cap) ctx->err = "cc_bam_assemble_keep: the buffer is smaller than the stream";
    return rc;
}

int cc_bam_assemble_group(cc_ctx* ctx, int32_t group_id) {
    if (!ctx || (group_id >= 0 && !ctx->groups.count(group_id))) return CC_E_INVALID;
    ctx->asm_group = group_id;
    return 0;
}

int cc_bam_assemble_names(cc_ctx* ctx, int64_t names_id) {
    if (!ctx) return CC_E_INVALID;
    if (names_id != 0 && !ctx->name_sets.count(names_id)) { ctx->err = "cc_bam_assemble_names: unknown name set"; return CC_E_INVALID; }
    ctx->asm_names = names_id;
    return 0;
}

int cc_bam_assemble_hook(cc_ctx* ctx, ccio_assemble_fn* fn, void** user) {
    if (!ctx || !fn || !user) return CC_E_INVALID;
    *fn = asm_hook_fn;
    *user = ctx;
    return 0;
}

}  // extern "C"
