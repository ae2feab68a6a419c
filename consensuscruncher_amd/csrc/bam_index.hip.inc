// cc_index_fields: what the BAI needs of each record of a resident stream, read where the stream
// lies (included by cc_engine.hip after table_unpack.hip.inc, whose DevSrc it reads with).
//   k_index_fields   a record per lane: index_core.h's field() checks the record's span, block_size and
//                    cigar extent before it reads through them, sums the reference length of the
//                    cigar 16 bytes (four ops) at a time and stores one 16-byte cc_index_field; the
//                    status word gets the first refused record.  The loads are DevSrc's aligned 16-byte
//                    words around the bytes asked for, which the resident streams' padding covers;
//                    bytes outside [at[i], at[i + 1]) are masked off before anything looks at them.
// A lane's cigar may hold 65,535 ops (16,384 loads); the other lanes of its wave wait for it, the
// grid does not.  The call runs on the coders' first stream under the encoder's mutex, so it may come
// from a writer thread while the context's own stream is busy.
#include "index_core.h"

namespace {

static_assert(sizeof(idx::Field) == sizeof(cc_index_field), "idx::Field is cc_index_field");

constexpr int IX_T = 256;

struct IxSrc {
    const uint8_t* base;
    __device__ __forceinline__ idx::W16 fetch(uint64_t a, uint32_t valid) const {
        const upk::W16 w = DevSrc{base, 0}.fetch(a, valid);
        return idx::W16{{w.w[0], w.w[1], w.w[2], w.w[3]}};
    }
};

// first_bad: (record index << 8 | its refusal bits) of the first refused record (~0: none)
__global__ __launch_bounds__(IX_T) void k_index_fields(const uint8_t* __restrict__ base, uint64_t total,
                                                       const uint64_t* __restrict__ at, int64_t n,
                                                       uint4* __restrict__ out, unsigned long long* first_bad) {
    const int64_t i = (int64_t)blockIdx.x * IX_T + threadIdx.x;
    if (i >= n) return;
    idx::Field f{0, 0, 0u, 0u};
    const uint32_t e = idx::field(IxSrc{base}, at[i], at[i + 1], total, f);
    if (e) {
        atomicMin(first_bad, ((unsigned long long)i << 8) | e);
        f = idx::Field{0, 0, 0u, 0u};
    }
    out[i] = make_uint4((uint32_t)f.tid, (uint32_t)f.pos, f.block_size, f.rl);
}

// cc_index_fields' work (the caller holds the encoder's mutex)
int index_fields(cc_ctx* ctx, BgzfEnc* E, int64_t id, const uint64_t* at, int64_t n, cc_index_field* fields) {
    const Resident* R = resident_find(E, id);
    if (!R) { E->err = "cc_index_fields: unknown id"; return CC_E_INVALID; }
    if (n < 0 || !at || (n > 0 && !fields)) { E->err = "cc_index_fields: null argument or a negative record count"; return CC_E_INVALID; }
    if (at[n] > R->total) { E->err = "cc_index_fields: at[n] lies past the stream"; return CC_E_INVALID; }
    if (n == 0) return 0;
    if (E->broken) return CC_E_HIP;
    BGCHK(hipSetDevice(ctx->device));
    RC(bgzf_streams(E));
    const bool prof = ctx->profiling;
    uint64_t* d_at = nullptr;
    uint4* d_out = nullptr;
    unsigned long long* d_bad = nullptr;
    unsigned long long bad = ~0ULL;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipMalloc((void**)&d_at, sizeof(uint64_t) * (size_t)(n + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, sizeof(uint4) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void**)&d_bad, sizeof bad);
    for (int k = 0; k < 2 && prof && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess) e = hipMemcpyAsync(d_at, at, sizeof(uint64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, E->st[0]);
    if (e == hipSuccess) e = hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, E->st[0]);
    if (e == hipSuccess && prof) e = hipEventRecord(ev[0], E->st[0]);
    if (e == hipSuccess) {
        klaunch(E->st[0], k_index_fields, nblk(n, IX_T), IX_T, R->p, R->total, d_at, n, d_out, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess && prof) e = hipEventRecord(ev[1], E->st[0]);
    if (e == hipSuccess) e = hipMemcpyAsync(fields, d_out, sizeof(uint4) * (size_t)n, hipMemcpyDeviceToHost, E->st[0]);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, E->st[0]);
    const hipError_t es = hipStreamSynchronize(E->st[0]);   // (also after a failure: the buffers are freed below)
    if (e == hipSuccess) e = es;
    float ms = 0;
    if (e == hipSuccess && prof) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (e == hipSuccess && prof) { E->idx_ms += ms; E->idx_n += 1; }
    for (int k = 0; k < 2; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (d_at) (void)hipFree(d_at);
    if (d_out) (void)hipFree(d_out);
    if (d_bad) (void)hipFree(d_bad);
    BGCHK(e);
    if (bad != ~0ULL) {
        char buf[200];
        snprintf(buf, sizeof buf, "cc_index_fields: record %lld: %s", (long long)(bad >> 8), idx::refusal((uint32_t)(bad & 0xff)));
        E->err = buf;
        return CC_E_INVALID;
    }
    return 0;
}

// ---- libccio's resident output callbacks over a context (ccio_set_out_resident): any failure is a
// nonzero return, after which libccio falls back as its header says
int outres_assemble_fn(void* user, const uint8_t* header, uint64_t header_bytes, const cc_asm_src* srcs, int32_t nsrc,
                       const cc_out_spec* spec, int64_t n, const char* names, const int64_t* name_off, int64_t n_names,
                       uint64_t names_bytes, const uint8_t* cons_seq, uint64_t cons_seq_bytes, const uint8_t* cons_qual,
                       uint64_t cons_qual_bytes, const char* rg_blob, const int64_t* rg_off, int32_t n_rg, int flags,
                       cc_asm_alloc_fn alloc, void* actx, int need_host, uint64_t* at, uint64_t* total, int64_t* token) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (!ctx || !token || !at || !total) return CC_E_INVALID;
    int32_t group = -1;
    if (!cons_seq && !cons_qual) {
        group = ctx->asm_group;
        ctx->asm_group = -1;
    }
    AsmArgs a{header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes, cons_seq,
              cons_seq_bytes, cons_qual, cons_qual_bytes, group, rg_blob, rg_off, n_rg, flags};
    a.names_set = asm_names_of(ctx, names, names_bytes);   // (not consumed: the plain hook finds it too)
    if (need_host && !alloc) return CC_E_INVALID;
    const int rc = bam_assemble_locked(ctx, a, need_host ? alloc : nullptr, actx, at, total, token);
    if (rc) ctx->asm_group = group;   // the plain hook, which libccio tries next, still finds it
    return rc;
}

int outres_deflate_fn(void* user, int64_t token, uint64_t off, uint64_t n, uint8_t* stage, uint64_t slot, uint32_t* out_len,
                      int64_t pieces) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (!ctx) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return bgzf_encode_resident(ctx, E, token, off, n, stage, slot, out_len, pieces) == pieces ? 0 : 1;
}

int outres_fields_fn(void* user, int64_t token, const uint64_t* at, int64_t n, cc_index_field* fields) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (!ctx) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return index_fields(ctx, E, token, at, n, fields) ? 1 : 0;
}

int outres_fetch_fn(void* user, int64_t token, uint64_t off, uint64_t n, uint8_t* dst) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (!ctx) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return resident_fetch_range(ctx, E, token, off, n, dst) ? 1 : 0;
}

void outres_release_fn(void* user, int64_t token) {
    cc_ctx* ctx = static_cast<cc_ctx*>(user);
    if (ctx) (void)cc_resident_free(ctx, token);
}

}  // namespace

extern "C" {

int cc_index_fields(cc_ctx* ctx, int64_t id, const uint64_t* at, int64_t n, cc_index_field* fields) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int rc = index_fields(ctx, E, id, at, n, fields);
    if (rc) ctx->err = E->err;
    return rc;
}

int cc_out_resident_hooks(cc_ctx* ctx, ccio_out_resident* cb, void** user) {
    if (!ctx || !cb || !user) return CC_E_INVALID;
    cb->assemble_keep = outres_assemble_fn;
    cb->deflate = outres_deflate_fn;
    cb->index_fields = outres_fields_fn;
    cb->fetch = outres_fetch_fn;
    cb->release = outres_release_fn;
    *user = ctx;
    return 0;
}

}  // extern "C"
