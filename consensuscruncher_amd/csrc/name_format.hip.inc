// cc_format_csn_names / cc_format_dcs_names: the consensus read names formatted on the device, byte
// for byte what libccio's ccio_format_csn_names / ccio_format_dcs_names give (included by cc_engine.hip
// after bam_assemble.hip.inc, whose DevFetch and padded upload it uses).
//   k_name_sizes_*  a name per thread: the shared rules (name_core.h) check the name's fields and give
//                   its length (dcs: also its packed layout, so the write kernel does not scan the
//                   two names again); the status block gets the first refused name with its reason
//                   and the 64-bit byte total
//   scan_launch     the lengths' exclusive scan: the names' 32-bit offsets
//   k_name_write_*  16 lanes per name: the head up to the blob's next 16-byte line and the tail behind
//                   the last whole line as single bytes, the lines between as aligned 16-byte stores;
//                   no lane writes a byte that is not its name's
// Nothing is read through a name's fields before the sizes kernel has accepted every name: the write
// kernel is only launched when no name was refused.
// The csn kernels are templates over where a name's nine fields and suffix come from: the call's
// uploaded arrays (CsnUploaded, cc_format_csn_names) or a group's emit_ckey / emit_n where the SSCS
// stage left them (CsnGroup, cc_format_csn_names_group).
// The blob and its 64-bit offsets stay with the context until cc_names_read fetches the blob or
// cc_names_keep turns the pair into a name set, which the assembler reads in place
// (cc_bam_assemble_names).
#include "name_core.h"

namespace {

struct NameStatus {
    unsigned long long first_bad;   // (name index << 8 | its refusal bits) of the first refused name (~0: none)
    unsigned long long total;       // the lengths summed in 64 bits (the scan's total is 32-bit)
    uint32_t guard, tot;            // guard: a write-kernel offset outside the blob (never expected); tot: the scan's total
};
static_assert(sizeof(NameStatus) == 24, "status layout");

constexpr int NM_T = 256;      // threads per block, all kernels
constexpr int NM_LANES = 16;   // lanes per name in the write kernels

// a record table's qname slots: 8-byte aligned, zero padded to whole words, 16 zero bytes behind the blob
struct NameTab {
    const uint8_t* blob;
    const uint64_t* qn_off;
    const uint16_t* qn_len;
    uint64_t bytes;
    int64_t n;
};

struct DevNameSrc {
    static __device__ __forceinline__ upk::W16 fetch(const uint8_t* base, uint64_t a, uint32_t valid) {
        return DevFetch::fetch(base, a, valid);
    }
    static __device__ __forceinline__ uint64_t word(const uint8_t* base, uint64_t a, uint32_t valid) {
        const uint64_t w = *reinterpret_cast<const uint64_t*>(base + a);
        return valid >= 8u ? w : (w & ((1ULL << (8u * valid)) - 1ULL));
    }
};

// the block's refusals and byte total folded into the status block
__device__ __forceinline__ void name_status(unsigned long long bad, uint32_t len, NameStatus* st) {
    __shared__ unsigned long long s_bad, s_tot;
    if (threadIdx.x == 0) { s_bad = ~0ULL; s_tot = 0; }
    __syncthreads();
    if (bad != ~0ULL) atomicMin(&s_bad, bad);
    else if (len) atomicAdd(&s_tot, (unsigned long long)len);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad != ~0ULL) atomicMin(&st->first_bad, s_bad);
        atomicAdd(&st->total, s_tot);
    }
}

// a csn name's fields from the call's uploaded arrays: a row of nine and a suffix per name
struct CsnUploaded {
    const int32_t* __restrict__ f9;
    const int64_t* __restrict__ suffix;
    __device__ __forceinline__ const int32_t* fields(int64_t i) const { return f9 + 9 * i; }
    __device__ __forceinline__ int64_t suf(int64_t i) const { return suffix[i]; }
};

// ... from a group's buffers: emit_ckey holds a row per emitted entry, shared by the entry's two names
// (SSCSRun.emit's np.repeat(..., 2)), emit_n the suffix of each name.  The host has checked that
// emit_ckey holds n / 2 rows and emit_n n values before any launch.
struct CsnGroup {
    const int32_t* __restrict__ ckey;
    const int32_t* __restrict__ emit_n;
    __device__ __forceinline__ const int32_t* fields(int64_t i) const { return ckey + 9 * (i >> 1); }
    __device__ __forceinline__ int64_t suf(int64_t i) const { return (int64_t)emit_n[i]; }
};

template <class Src>
__global__ __launch_bounds__(NM_T) void k_name_sizes_csn(Src src, int64_t n, nmc::Strs bc, nmc::Strs cg,
                                                         uint32_t* __restrict__ len, NameStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    unsigned long long bad = ~0ULL;
    uint32_t l = 0;
    if (i < n) {
        nmc::CsnLay y;
        const uint32_t e = nmc::csn_layout(src.fields(i), src.suf(i), bc, cg, y);
        if (e) bad = ((unsigned long long)i << 8) | e;
        else l = y.len;
        len[i] = l;
    }
    name_status(bad, l, st);
}

// the pair's two slots checked against the table; false: refused
__device__ __forceinline__ bool name_slots(const NameTab& T, int64_t rt, int64_t rd, uint64_t* ta, uint32_t* tl, uint64_t* da,
                                           uint32_t* dl) {
    if (rt < 0 || rt >= T.n || rd < 0 || rd >= T.n) return false;
    *ta = T.qn_off[rt];
    *tl = T.qn_len[rt];
    *da = T.qn_off[rd];
    *dl = T.qn_len[rd];
    // (a slot is its name's whole words: nothing is read past them)
    return *tl <= 255u && *dl <= 255u && !(*ta & 7u) && !(*da & 7u) && *ta <= T.bytes && ((*tl + 7u) & ~7u) <= T.bytes - *ta &&
           *da <= T.bytes && ((*dl + 7u) & ~7u) <= T.bytes - *da;
}

__global__ __launch_bounds__(NM_T) void k_name_sizes_dcs(NameTab T, const int64_t* __restrict__ rec_tag,
                                                         const int64_t* __restrict__ rec_ds, int64_t n,
                                                         uint32_t* __restrict__ len, uint64_t* __restrict__ lay,
                                                         NameStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * NM_T + threadIdx.x;
    unsigned long long bad = ~0ULL;
    uint32_t l = 0;
    if (i < n) {
        uint64_t ta, da;
        uint32_t tl, dl;
        nmc::DcsLay y;
        uint32_t e = nmc::NE_REC;
        if (name_slots(T, rec_tag[i], rec_ds[i], &ta, &tl, &da, &dl)) e = nmc::dcs_layout<DevNameSrc>(T.blob, ta, tl, da, dl, y);
        if (e) bad = ((unsigned long long)i << 8) | e;
        else l = y.len;
        len[i] = l;
        lay[i] = e ? 0ull : nmc::dcs_pack(y);
    }
    name_status(bad, l, st);
}

// Lane j of the group that writes a name of `len` bytes to out[off ...): out16(at, valid) gives the
// name's bytes.  The head, up to the blob's next 16-byte line, and the tail go out as single bytes,
// the lines between as aligned 16-byte stores.
template <class Out>
__device__ __forceinline__ void name_store(uint8_t* __restrict__ out, uint64_t off, uint32_t len, uint32_t j, Out out16) {
    uint8_t* d = out + off;
    const uint32_t head = min(len, (16u - ((uint32_t)off & 15u)) & 15u);
    const uint32_t lines = (len - head) >> 4, tail_at = head + (lines << 4);
    uint4* dl = reinterpret_cast<uint4*>(d + head);
    // step 0 the head, step 1 the tail, then the lines NM_LANES at a time (one call site of out16: the
    // name's layout stays in registers)
    const uint32_t steps = 2u + (lines + NM_LANES - 1u) / NM_LANES;
    for (uint32_t s = 0; s < steps; ++s) {
        const bool line = s >= 2u;
        const uint32_t c = (s - 2u) * NM_LANES + j;
        const uint32_t at = line ? head + (c << 4) : (s == 0u ? j : tail_at + j);
        const bool on = line ? c < lines : (s == 0u ? j < head : at < len);
        if (!on) continue;
        const upk::W16 w = out16(at, line ? 16u : 1u);
        if (line) dl[c] = make_uint4(w.w[0], w.w[1], w.w[2], w.w[3]);
        else d[at] = (uint8_t)w.w[0];
    }
}

// Name i goes to out[off32[i] ...).  Every name was accepted by the sizes kernel and off32 is the scan of
// the lengths it wrote, so each name lies inside out[0, total).
template <class Src>
__global__ __launch_bounds__(NM_T) void k_name_write_csn(Src src, int64_t n, nmc::Strs bc, nmc::Strs cg,
                                                         const uint32_t* __restrict__ off32, uint64_t total,
                                                         uint8_t* __restrict__ out, int64_t* __restrict__ off64,
                                                         NameStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * (NM_T / NM_LANES) + (threadIdx.x / NM_LANES);
    const uint32_t j = threadIdx.x % NM_LANES;
    if (i >= n) return;
    const int32_t* f = src.fields(i);
    (void)CC_IDXG(f[0], bc.n, DS_REC, &st->guard);
    (void)CC_IDXG(f[5], cg.n, DS_REC, &st->guard);
    (void)CC_IDXG(f[6], cg.n, DS_REC, &st->guard);
    nmc::CsnLay y;
    const uint32_t e = nmc::csn_layout(f, src.suf(i), bc, cg, y);
    const uint64_t off = off32[i];
    if (e || off > total || y.len > total - off) {   // (containment: never expected)
        if (j == 0) atomicOr(&st->guard, 1u);
        return;
    }
    if (j == 0) {
        off64[i] = (int64_t)off;
        if (i == n - 1) off64[n] = (int64_t)(off + y.len);
    }
    name_store(out, off, y.len, j, [&](uint32_t at, uint32_t valid) NMC_INL { return nmc::csn_out16<DevNameSrc>(y, bc, cg, at, valid); });
}

__global__ __launch_bounds__(NM_T) void k_name_write_dcs(NameTab T, const int64_t* __restrict__ rec_tag,
                                                         const int64_t* __restrict__ rec_ds, const uint64_t* __restrict__ lay,
                                                         int64_t n, const uint32_t* __restrict__ off32, uint64_t total,
                                                         uint8_t* __restrict__ out, int64_t* __restrict__ off64,
                                                         NameStatus* st) {
    const int64_t i = (int64_t)blockIdx.x * (NM_T / NM_LANES) + (threadIdx.x / NM_LANES);
    const uint32_t j = threadIdx.x % NM_LANES;
    if (i >= n) return;
    const int64_t rt = CC_IDXG(rec_tag[i], T.n, DS_REC, &st->guard), rd = CC_IDXG(rec_ds[i], T.n, DS_REC, &st->guard);
    uint64_t ta, da;
    uint32_t tl, dl;
    const bool ok = name_slots(T, rt, rd, &ta, &tl, &da, &dl);
    const nmc::DcsLay y = nmc::dcs_unpack(lay[i]);
    const uint64_t off = off32[i];
    // (containment, never expected: the pieces lie inside the two names as the sizes kernel found them)
    if (!ok || off > total || y.len > total - off || y.tb + 1u + y.cl > tl || y.t1 + 1u + y.tfl > tl || y.db > dl ||
        y.d1 + 1u + y.dfl > dl) {
        if (j == 0) atomicOr(&st->guard, 1u);
        return;
    }
    if (j == 0) {
        off64[i] = (int64_t)off;
        if (i == n - 1) off64[n] = (int64_t)(off + y.len);
    }
    name_store(out, off, y.len, j,
               [&](uint32_t at, uint32_t valid) NMC_INL { return nmc::dcs_out16<DevNameSrc>(y, T.blob, ta, da, at, valid); });
}

const char* name_refusal(uint32_t bits) {
    if (bits & nmc::NE_BC) return "field 0 outside the barcode table";
    if (bits & nmc::NE_CG5) return "field 5 outside the cigar table";
    if (bits & nmc::NE_CG6) return "field 6 outside the cigar table";
    if (bits & nmc::NE_STR) return "a string's offsets outside its blob";
    if (bits & nmc::NE_T_NOUS) return "no '_' in the tag name";
    if (bits & nmc::NE_T_NOCOLON) return "no ':' in the tag name";
    if (bits & nmc::NE_D_NOCOLON) return "no ':' in the partner name";
    return "a record index outside the table";
}

std::atomic<int64_t> g_names_next{1};   // name set ids: positive, unique across contexts

void names_release(cc_ctx* ctx) {
    if (ctx->names_buf || ctx->names_off) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->names_buf) (void)hipFree(ctx->names_buf);
        if (ctx->names_off) (void)hipFree(ctx->names_off);
    }
    ctx->names_buf = nullptr;
    ctx->names_off = nullptr;
    ctx->names_n = 0;
    ctx->names_total = -1;
}

const NameSet* names_find(cc_ctx* ctx, int64_t id) {
    const auto it = id > 0 ? ctx->name_sets.find(id) : ctx->name_sets.end();
    return it != ctx->name_sets.end() ? &it->second : nullptr;
}

// the call's allocations: the temporaries always freed, the blob and its offsets unless the call succeeded
struct NameGuard {
    cc_ctx* ctx;
    std::vector<void*> tmp;
    uint8_t* blob = nullptr;
    int64_t* off = nullptr;
    ~NameGuard() {
        (void)hipStreamSynchronize(ctx->stream);   // nothing enqueued still uses them
        for (void* p : tmp) (void)hipFree(p);
        if (blob) (void)hipFree(blob);
        if (off) (void)hipFree(off);
    }
};

struct NameRun {
    cc_ctx* ctx;
    const char* what;
    NameGuard guard;
    NameStatus* h_st;
    NameStatus* d_st = nullptr;
    uint32_t *len = nullptr, *off32 = nullptr;
    int64_t* d_off = nullptr;
    int64_t n;

    NameRun(cc_ctx* c, const char* w, int64_t n_) : ctx(c), what(w), guard{c}, n(n_) {
        h_st = reinterpret_cast<NameStatus*>((uint8_t*)ctx->h_pinned + 768);
    }
    // before the sizes kernel: the lengths, the offsets and the status block
    int begin() {
        *h_st = NameStatus{};
        h_st->first_bad = ~0ULL;
        RC(dev_alloc(ctx, guard.tmp, &len, n, 64));
        RC(dev_alloc(ctx, guard.tmp, &off32, n, 64));
        HIPCHK(hipMalloc((void**)&guard.off, sizeof(int64_t) * (size_t)(n + 1)));
        d_off = guard.off;
        RC(dev_alloc(ctx, guard.tmp, &d_st, 1));
        HIPCHK(hipMemcpyAsync(d_st, h_st, sizeof(NameStatus), hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    int status() {
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(NameStatus), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    // after the sizes kernel: the refusals, the offsets' scan and the blob's buffer
    int offsets() {
        RC(status());
        if (h_st->first_bad != ~0ULL) {
            char buf[200];
            snprintf(buf, sizeof buf, "%s: name %lld: %s", what, (long long)(h_st->first_bad >> 8),
                     name_refusal((uint32_t)(h_st->first_bad & 0xff)));
            ctx->err = buf;
            return CC_E_INVALID;
        }
        if (h_st->total > 0xffffffffull) {
            ctx->err = std::string(what) + ": a blob of 2^32 bytes or more";
            return CC_E_UNSUPPORTED;
        }
        RC(scan_launch(ctx, len, n, &d_st->tot, "name_scan", ScanStore{off32}));
        RC(status());
        if (h_st->tot != h_st->total) {
            ctx->err = std::string(what) + ": the offsets' scan total does not match the lengths";
            return CC_E_INVALID;
        }
        // (the assembler's read contract, as asm_upload_padded gives it: a name set is read in place)
        const size_t padded = (size_t)((h_st->total + 15) & ~15ull) + 32;
        HIPCHK(hipMalloc((void**)&guard.blob, padded));
        HIPCHK(hipMemsetAsync(guard.blob + h_st->total, 0, padded - (size_t)h_st->total, ctx->stream));
        return 0;
    }
    // after the write kernel: the offsets fetched, the blob handed to the context
    int finish(int64_t* off, int64_t* total) {
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(off, d_off, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, ctx->stream));
        RC(status());
        if (h_st->guard) {
            ctx->err = std::string(what) + ": a name outside the blob (guarded)";
            return CC_E_INVALID;
        }
        if (off[n] != (int64_t)h_st->total) {
            ctx->err = std::string(what) + ": the last offset is not the total";
            return CC_E_INVALID;
        }
        *total = (int64_t)h_st->total;
        ctx->names_buf = guard.blob;
        ctx->names_off = guard.off;
        ctx->names_n = n;
        ctx->names_total = *total;
        guard.blob = nullptr;
        guard.off = nullptr;
        return 0;
    }
};

int names_empty(cc_ctx* ctx, int64_t* off, int64_t* total) {
    off[0] = 0;
    *total = 0;
    ctx->names_total = 0;   // (a blob of no bytes: cc_names_read copies nothing)
    return 0;
}

// a table's strings for the kernels: the blob padded for aligned loads, the offsets as they came
int names_strs(cc_ctx* ctx, std::vector<void*>& tmp, nmc::Strs* s, const char* blob, const int64_t* off, int64_t n) {
    s->n = n;
    s->bytes = n > 0 ? (uint64_t)std::max<int64_t>(off[n], 0) : 0;
    RC(asm_upload_padded(ctx, tmp, &s->blob, blob, s->bytes));
    int64_t* o = nullptr;
    RC(upload(ctx, tmp, &o, off, n > 0 ? n + 1 : 0));
    s->off = o;
    return 0;
}

// cc_format_csn_names' and cc_format_csn_names_group's work once the fields' source is on the device
template <class Src>
int names_csn(NameRun& run, const Src& src, const nmc::Strs& bc, const nmc::Strs& cg, int64_t* off, int64_t* total) {
    cc_ctx* ctx = run.ctx;
    const int64_t n = run.n;
    RC(run.begin());
    klaunch(ctx, "name_sizes", k_name_sizes_csn<Src>, nblk(n, NM_T), NM_T, src, n, bc, cg, run.len, run.d_st);
    RC(run.offsets());
    klaunch(ctx, "name_write", k_name_write_csn<Src>, nblk(n, NM_T / NM_LANES), NM_T, src, n, bc, cg, run.off32,
            (uint64_t)run.h_st->total, run.guard.blob, run.d_off, run.d_st);
    return run.finish(off, total);
}

bool names_tables_bad(const char* bc_blob, const int64_t* bc_off, int64_t n_bc, const char* cg_blob, const int64_t* cg_off,
                      int64_t n_cg) {
    return n_bc < 0 || n_cg < 0 || (n_bc > 0 && !bc_off) || (n_cg > 0 && !cg_off) || (n_bc > 0 && bc_off[n_bc] > 0 && !bc_blob) ||
           (n_cg > 0 && cg_off[n_cg] > 0 && !cg_blob);
}

}  // namespace

extern "C" {

int cc_format_csn_names(cc_ctx* ctx, int64_t n, const int32_t* f9, const int64_t* suffix, const char* bc_blob,
                        const int64_t* bc_off, int64_t n_bc, const char* cg_blob, const int64_t* cg_off, int64_t n_cg,
                        int64_t* off, int64_t* total) {
    if (!ctx) return CC_E_INVALID;
    if (n < 0 || !off || !total || (n > 0 && (!f9 || !suffix)) || names_tables_bad(bc_blob, bc_off, n_bc, cg_blob, cg_off, n_cg)) {
        ctx->err = "cc_format_csn_names: null or negative argument";
        return CC_E_INVALID;
    }
    if (n > (int64_t)INT32_MAX) { ctx->err = "cc_format_csn_names: more than 2^31 - 1 names"; return CC_E_UNSUPPORTED; }
    RC(enter(ctx));
    names_release(ctx);
    if (n == 0) return names_empty(ctx, off, total);
    NameRun run(ctx, "cc_format_csn_names", n);
    nmc::Strs bc{}, cg{};
    RC(names_strs(ctx, run.guard.tmp, &bc, bc_blob, bc_off, n_bc));
    RC(names_strs(ctx, run.guard.tmp, &cg, cg_blob, cg_off, n_cg));
    int32_t* d_f9 = nullptr;
    int64_t* d_suf = nullptr;
    {
        ProfScope ps(ctx, "name_fields_upload");   // (what cc_format_csn_names_group does without)
        RC(upload(ctx, run.guard.tmp, &d_f9, f9, 9 * n));
        RC(upload(ctx, run.guard.tmp, &d_suf, suffix, n));
    }
    return names_csn(run, CsnUploaded{d_f9, d_suf}, bc, cg, off, total);
}

int cc_format_csn_names_group(cc_ctx* ctx, int32_t group_id, const char* bc_blob, const int64_t* bc_off, int64_t n_bc,
                              const char* cg_blob, const int64_t* cg_off, int64_t n_cg, int64_t* off, int64_t* total) {
    if (!ctx) return CC_E_INVALID;
    if (!off || !total || names_tables_bad(bc_blob, bc_off, n_bc, cg_blob, cg_off, n_cg)) {
        ctx->err = "cc_format_csn_names_group: null or negative argument";
        return CC_E_INVALID;
    }
    if (!ctx->groups.count(group_id)) { ctx->err = "cc_format_csn_names_group: unknown group"; return CC_E_INVALID; }
    const Group& g = *ctx->groups[group_id];
    const int32_t* ckey = g.ptr<B::emit_ckey>();
    const int32_t* emit_n = g.ptr<B::emit_n>();
    if (!g.planned[ST_SSCS] || !ckey || !emit_n) {
        ctx->err = "cc_format_csn_names_group: the group holds no cc_consensus_maker output";
        return CC_E_INVALID;
    }
    // the extents the kernels index by, from the buffers' used sizes: a row of emit_ckey per two names
    const size_t ck_used = g.buf[(int)B::emit_ckey].used, en_used = g.buf[(int)B::emit_n].used;
    const int64_t rows = (int64_t)(ck_used / (9 * sizeof(int32_t))), n = (int64_t)(en_used / sizeof(int32_t));
    if (ck_used % (9 * sizeof(int32_t)) || en_used % sizeof(int32_t) || rows * 2 != n) {
        ctx->err = "cc_format_csn_names_group: emit_ckey does not hold a row per two values of emit_n";
        return CC_E_INVALID;
    }
    if (n > (int64_t)INT32_MAX) { ctx->err = "cc_format_csn_names: more than 2^31 - 1 names"; return CC_E_UNSUPPORTED; }
    RC(enter(ctx));
    names_release(ctx);
    if (n == 0) return names_empty(ctx, off, total);
    NameRun run(ctx, "cc_format_csn_names", n);
    nmc::Strs bc{}, cg{};
    RC(names_strs(ctx, run.guard.tmp, &bc, bc_blob, bc_off, n_bc));
    RC(names_strs(ctx, run.guard.tmp, &cg, cg_blob, cg_off, n_cg));
    return names_csn(run, CsnGroup{ckey, emit_n}, bc, cg, off, total);
}

int cc_format_dcs_names(cc_ctx* ctx, int32_t table, int64_t n, const int64_t* rec_tag, const int64_t* rec_ds, int64_t* off,
                        int64_t* total) {
    if (!ctx) return CC_E_INVALID;
    if (n < 0 || !off || !total || (n > 0 && (!rec_tag || !rec_ds))) {
        ctx->err = "cc_format_dcs_names: null or negative argument";
        return CC_E_INVALID;
    }
    if (!ctx->tables.count(table)) { ctx->err = "cc_format_dcs_names: unknown table"; return CC_E_INVALID; }
    if (n > (int64_t)INT32_MAX) { ctx->err = "cc_format_dcs_names: more than 2^31 - 1 names"; return CC_E_UNSUPPORTED; }
    RC(enter(ctx));
    names_release(ctx);
    if (n == 0) return names_empty(ctx, off, total);
    const DevTable& D = ctx->tables[table];
    const NameTab T{D.qn_blob, D.qn_off, D.qn_len, D.qn_bytes, D.n};
    NameRun run(ctx, "cc_format_dcs_names", n);
    int64_t *d_t = nullptr, *d_d = nullptr;
    uint64_t* lay = nullptr;
    RC(upload(ctx, run.guard.tmp, &d_t, rec_tag, n));
    RC(upload(ctx, run.guard.tmp, &d_d, rec_ds, n));
    RC(dev_alloc(ctx, run.guard.tmp, &lay, n));
    RC(run.begin());
    klaunch(ctx, "name_sizes", k_name_sizes_dcs, nblk(n, NM_T), NM_T, T, d_t, d_d, n, run.len, lay, run.d_st);
    RC(run.offsets());
    klaunch(ctx, "name_write", k_name_write_dcs, nblk(n, NM_T / NM_LANES), NM_T, T, d_t, d_d, lay, n, run.off32,
            (uint64_t)run.h_st->total, run.guard.blob, run.d_off, run.d_st);
    return run.finish(off, total);
}

int cc_names_read(cc_ctx* ctx, char* blob, int64_t cap) {
    if (!ctx) return CC_E_INVALID;
    if (ctx->names_total < 0) { ctx->err = "cc_names_read: no formatted names to read"; return CC_E_INVALID; }
    if (cap < ctx->names_total || (ctx->names_total > 0 && !blob)) {
        ctx->err = "cc_names_read: the buffer is smaller than the blob";
        return CC_E_INVALID;
    }
    RC(enter(ctx));
    if (ctx->names_total > 0) {
        ProfScope ps(ctx, "name_download");
        HIPCHK(hipMemcpyAsync(blob, ctx->names_buf, (size_t)ctx->names_total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    names_release(ctx);
    return 0;
}

int cc_names_keep(cc_ctx* ctx, int64_t* names_id) {
    if (!ctx || !names_id) return CC_E_INVALID;
    *names_id = 0;
    if (ctx->names_total < 0) { ctx->err = "cc_names_keep: no formatted names to keep"; return CC_E_INVALID; }
    RC(enter(ctx));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the format call waited already)
    const int64_t id = g_names_next.fetch_add(1);
    ctx->name_sets[id] = NameSet{ctx->names_buf, ctx->names_off, ctx->names_n, ctx->names_total};
    ctx->names_buf = nullptr;   // the set's from here on
    ctx->names_off = nullptr;
    names_release(ctx);
    *names_id = id;
    return 0;
}

int64_t cc_names_fetch(cc_ctx* ctx, int64_t names_id, char* blob, int64_t cap) {
    if (!ctx) return CC_E_INVALID;
    const NameSet* s = names_find(ctx, names_id);
    if (!s) { ctx->err = "cc_names_fetch: unknown name set"; return CC_E_INVALID; }
    if (!blob) return s->total;
    if (cap < s->total) { ctx->err = "cc_names_fetch: the buffer is smaller than the blob"; return CC_E_INVALID; }
    RC(enter(ctx));
    if (s->total > 0) {
        ProfScope ps(ctx, "name_download");
        HIPCHK(hipMemcpyAsync(blob, s->blob, (size_t)s->total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return s->total;
}

int cc_names_free(cc_ctx* ctx, int64_t names_id) {
    if (!ctx) return CC_E_INVALID;
    const NameSet* s = names_find(ctx, names_id);
    if (!s) { ctx->err = "cc_names_free: unknown name set"; return CC_E_INVALID; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);   // no assemble still reads it
    if (s->blob) (void)hipFree(s->blob);
    if (s->off) (void)hipFree(s->off);
    ctx->name_sets.erase(names_id);
    if (ctx->asm_names == names_id) ctx->asm_names = 0;
    return 0;
}

int64_t cc_names_count(cc_ctx* ctx) { return ctx ? (int64_t)ctx->name_sets.size() : CC_E_INVALID; }

}  // extern "C"
