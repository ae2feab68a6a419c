// The device BGZF inflater (cc_bgzf_inflate, cc_bgzf_inflate_hook) and the resident streams it can
// leave on the device (cc_bgzf_inflate_keep, cc_resident_*): included by cc_engine.hip after
// bgzf_deflate.hip.inc, whose streams, mutex and "nothing more on the device after a HIP error" latch
// they share.  With a crc pointer (cc_bgzf_inflate_crc, cc_bgzf_inflate_keep_crc) every round is followed
// by k_crc32 (bgzf_crc32.hip.inc); cc_crc32 and cc_resident_crc32, that kernel's function-level entry
// points, are at the end of this file because they need the streams and the resident table.
//
// k_bgzf_inflate: one wave (a 64-thread workgroup) per member, many members in flight.  DEFLATE is
// serial in bit order, so a member advances in batches of three steps:
//   stage:  all lanes copy the next compressed words into a 2 KiB LDS ring (coalesced 4-byte loads);
//   decode: lane 0 runs inflate_core.h's ifl::run over the staged bytes with the tables in LDS.
//           Literals go to a small LDS buffer, a match becomes a token (literals before it | length
//           | distance).  The batch ends after 254 tokens, 1536 literals, or when fewer staged bytes
//           are left than a block header needs;
//   copy:   all lanes walk the tokens in order: the literal run goes to the window and to global,
//           the match is read from the window at pos - dist + (i mod dist) (so overlapping matches,
//           distance 1 included, come out right) and written to the window and to global.
// The window is the last 32768 output bytes in LDS, a ring: output byte q takes the slot byte
// q - 32768 had.  The copy step writes strictly in output order, so the byte a write replaces lies
// more than 32768 behind everything still to come, and no later match can name it.  A match never
// reads global memory, so no store-to-load ordering on global memory is needed.
//
// Bounds: compressed words are read inside [coff, coff + round_up(clen, 16)), which the host side
// allocates (every member starts at a 16-byte multiple of the upload buffer); every LDS index is
// masked to its ring or checked against its buffer; a global store goes to ooff + produced + i with
// produced + len <= ulen checked by the core before the token exists.  A member the core refuses,
// or one that makes no progress in a batch, ends with status 0; nothing can loop without consuming
// input bits.
#include "inflate_core.h"

namespace {

constexpr int BI_T = 64;                  // one wave per member
constexpr int BI_RING = 32768;            // the output window in LDS
constexpr int BI_IN = 2048;               // the compressed bytes' ring in LDS
constexpr int BI_TOK = 256;               // tokens per batch
constexpr int BI_LIT = 1536;              // literals per batch
constexpr int BI_ROUND = 1024;            // members per launch
constexpr uint32_t BI_MEMBER = 0x10000;   // a BGZF member's bounds, compressed and inflated
constexpr size_t BI_IN_CAP = (size_t)32 << 20;                 // upload bytes per round
constexpr size_t BI_OUT_CAP = (size_t)BI_ROUND * BI_MEMBER;    // download bytes per round
static_assert(BI_IN >= 2 * ifl::HEADER_BYTES + 8, "a freshly staged ring holds a whole block header");

// The staged compressed bytes: byte i lives at ring byte i mod BI_IN.  word() reads the aligned word
// that holds byte i and so relies on i being a multiple of 4.  ifl::Bits keeps it one: pos starts at
// 0 and refill() advances it by 4 except for the last, partial word, which it can only take when
// avail == end (the kernel's avail is a multiple of 4 whenever it is below clen), and after which
// pos == avail, so no further word is asked for.
struct BiSrc {
    const uint32_t* ring;
    __host__ __device__ uint32_t word(uint32_t i, uint32_t valid) const {
        const uint32_t w = ring[(i >> 2) & (BI_IN / 4 - 1)];
        return valid >= 4 ? w : w & ((1u << (8 * valid)) - 1);
    }
};

struct BiSink {   // lane 0's outputs: literals and tokens for the copy step
    uint8_t* litbuf;
    uint32_t* tok;
    uint32_t ntok, lits, nlit;
    bool over;
    __host__ __device__ void push(uint32_t t) {
        if (ntok < (uint32_t)BI_TOK) tok[ntok++] = t;
        else over = true;   // unreachable while full() is asked before every symbol; fails the member
        lits = 0;
    }
    __host__ __device__ bool full(uint32_t) const { return ntok >= (uint32_t)BI_TOK - 2 || nlit >= (uint32_t)BI_LIT; }
    __host__ __device__ void lit(uint8_t c, uint32_t) {
        if (nlit < (uint32_t)BI_LIT) litbuf[nlit++] = c;
        else over = true;
        if (++lits == 255) push(lits << 24);
    }
    __host__ __device__ void match(uint32_t len, uint32_t dist, uint32_t) { push((dist - 1) | (len << 15) | (lits << 24)); }
    __host__ __device__ void flush() { if (lits) push(lits << 24); }
};

struct BiCtl {   // a member's state between batches
    ifl::State st;
    uint32_t pos, cnt, staged, ntok, rc;
    uint64_t buf;
};

// desc[j] = {offset in `in`, clen, offset in `out`, ulen}; status[j] = 1 when member j is good.  `out`
// is the round's base: the round's own output buffer, or the round's lowest offset in a resident
// stream (the stores are byte stores, so neither it nor a member's offset need be aligned).
__global__ __launch_bounds__(BI_T) void k_bgzf_inflate(const uint8_t* __restrict__ in, const uint4* __restrict__ desc,
                                                       uint8_t* __restrict__ out, uint32_t* __restrict__ status,
                                                       int members) {
    __shared__ uint32_t s_out[BI_RING / 4];
    __shared__ uint32_t s_in[BI_IN / 4];
    __shared__ uint32_t s_tok[BI_TOK];
    __shared__ uint32_t s_lit[BI_LIT / 4];
    __shared__ ifl::Huff<ifl::NLIT> s_L;
    __shared__ ifl::Huff<ifl::NDIST> s_D;
    __shared__ uint8_t s_lens[ifl::LENS];
    __shared__ uint16_t s_offs[ifl::MAXBITS + 1];
    __shared__ BiCtl s_ctl;
    const int j = (int)blockIdx.x;
    if (j >= members) return;
    const uint32_t lane = threadIdx.x;
    const uint4 d = desc[j];
    const uint32_t clen = d.y, ulen = d.w;
    const uint8_t* src = in + d.x;   // 16-byte aligned
    uint8_t* og = out + d.z;
    uint8_t* win = (uint8_t*)s_out;
    uint8_t* litbuf = (uint8_t*)s_lit;
    if (lane == 0) {
        s_ctl.st = ifl::State{ifl::P_HEAD, 0, 0, 0, ulen};
        s_ctl.pos = s_ctl.cnt = s_ctl.staged = s_ctl.ntok = 0;
        s_ctl.rc = ifl::R_PAUSE;
        s_ctl.buf = 0;
    }
    __syncthreads();
    const uint32_t cwords_end = (clen + 3) & ~3u;
    uint32_t opos = 0;   // output bytes copied so far (the same in every lane)
    uint32_t rc;
    for (;;) {
        // ---- stage: words [staged, target) of the member; the slots they take held bytes below pos
        const uint32_t staged = s_ctl.staged;
        const uint32_t base = s_ctl.pos & ~3u;
        uint32_t target = base + (uint32_t)BI_IN;
        if (target > cwords_end) target = cwords_end;
        for (uint32_t w = staged + 4 * lane; w < target; w += 4 * BI_T)
            s_in[(w >> 2) & (BI_IN / 4 - 1)] = *(const uint32_t*)(src + w);
        __syncthreads();
        // ---- decode: lane 0, until the batch is full, the staged bytes run low, or the member ends
        if (lane == 0) {
            const uint32_t now = target > staged ? target : staged;
            ifl::Bits<BiSrc> b;
            b.src.ring = s_in;
            b.pos = s_ctl.pos;
            b.end = clen;
            b.avail = now < clen ? now : clen;
            b.cnt = s_ctl.cnt;
            b.buf = s_ctl.buf;
            ifl::State st = s_ctl.st;
            const ifl::Tables T = {&s_L, &s_D, s_lens, s_offs};
            BiSink k = {litbuf, s_tok, 0, 0, 0, false};
            const uint64_t before = (uint64_t)b.pos * 8 - b.cnt;
            uint32_t r = (uint32_t)ifl::run(st, b, T, k);
            k.flush();
            if (k.over) r = ifl::R_FAIL;
            // a batch that neither consumed a bit nor ended the member would repeat for ever
            if (r == ifl::R_PAUSE && k.ntok == 0 && (uint64_t)b.pos * 8 - b.cnt == before) r = ifl::R_FAIL;
            s_ctl.st = st;
            s_ctl.pos = b.pos;
            s_ctl.cnt = b.cnt;
            s_ctl.buf = b.buf;
            s_ctl.staged = now;
            s_ctl.ntok = k.ntok;
            s_ctl.rc = r;
        }
        __syncthreads();
        rc = s_ctl.rc;
        if (rc == ifl::R_FAIL) break;
        // ---- copy: the tokens in order, 64 bytes a step
        const uint32_t ntok = s_ctl.ntok;
        uint32_t lpos = 0;   // literals of this batch copied so far
        for (uint32_t t = 0; t < ntok; ++t) {
            const uint32_t tk = s_tok[t];
            const uint32_t lits = tk >> 24, len = (tk >> 15) & 511, dist = (tk & 32767) + 1;
            if (lits) {
                for (uint32_t i = lane; i < lits; i += BI_T) {
                    const uint8_t c = litbuf[(lpos + i) % BI_LIT];   // lpos + lits <= BI_LIT by the sink's count
                    win[(opos + i) & (BI_RING - 1)] = c;
                    og[opos + i] = c;
                }
                opos += lits;
                lpos += lits;
                __syncthreads();   // a later match may read these literals from the window
            }
            if (len) {
                for (uint32_t i = lane; i < len; i += BI_T) {
                    const uint32_t k = dist < len ? i % dist : i;
                    const uint8_t c = win[(opos - dist + k) & (BI_RING - 1)];   // below opos: never a byte of this match
                    win[(opos + i) & (BI_RING - 1)] = c;
                    og[opos + i] = c;
                }
                opos += len;
                __syncthreads();   // the next token may read what these lanes wrote to the window
            }
        }
        if (rc == ifl::R_DONE) break;
        __syncthreads();   // the tokens and literals are read, and the window written, before the next batch
    }
    if (lane == 0) status[j] = rc == ifl::R_DONE ? 1u : 0u;
}

}  // namespace

// A resident stream: the inflated file at its own offsets in a device buffer the context owns.
// `total` usable bytes, align16(total) + 32 allocated, the bytes behind total zero (DevSrc's contract
// in table_unpack.hip.inc).  Ids are unique across contexts, so another context's id is unknown here.
struct Resident {
    uint8_t* p = nullptr;
    uint64_t total = 0;
};
std::atomic<int64_t> g_resident_next{1};

struct BgzfDec {
    bool ready = false;
    std::map<int64_t, Resident> res;   // under the encoder's mutex
    uint8_t* h_in[2] = {nullptr, nullptr};
    uint8_t* h_out[2] = {nullptr, nullptr};
    uint4* h_desc[2] = {nullptr, nullptr};
    uint32_t* h_ok[2] = {nullptr, nullptr};
    uint8_t* d_in[2] = {nullptr, nullptr};
    uint8_t* d_out[2] = {nullptr, nullptr};
    uint4* d_desc[2] = {nullptr, nullptr};
    uint32_t* d_ok[2] = {nullptr, nullptr};
    hipEvent_t ev[2][6] = {};   // per stream: around the kernel, the upload, the download
    bool timed[2] = {false, false};
    double prof_ms = 0, h2d_ms = 0, d2h_ms = 0;   // scopes bgzf_inflate, bgzf_in_upload, bgzf_in_download
    int64_t prof_n = 0;
    CrcBufs cb;   // the members' CRCs (made by the first round that is asked for them)
};

namespace {

inline size_t bi_align(size_t v) { return (v + 15) & ~(size_t)15; }

int bgzf_dec_init(BgzfEnc* E, BgzfDec* D) {
    RC(bgzf_streams(E));
    for (int b = 0; b < 2; ++b) {
        BGCHK(hipHostMalloc((void**)&D->h_in[b], BI_IN_CAP));
        BGCHK(hipHostMalloc((void**)&D->h_out[b], BI_OUT_CAP));
        BGCHK(hipHostMalloc((void**)&D->h_desc[b], BI_ROUND * sizeof(uint4)));
        BGCHK(hipHostMalloc((void**)&D->h_ok[b], BI_ROUND * sizeof(uint32_t)));
        BGCHK(hipMalloc((void**)&D->d_in[b], BI_IN_CAP));
        BGCHK(hipMalloc((void**)&D->d_out[b], BI_OUT_CAP));
        BGCHK(hipMalloc((void**)&D->d_desc[b], BI_ROUND * sizeof(uint4)));
        BGCHK(hipMalloc((void**)&D->d_ok[b], BI_ROUND * sizeof(uint32_t)));
        for (int k = 0; k < 6; ++k) BGCHK(hipEventCreate(&D->ev[b][k]));
    }
    D->ready = true;
    return 0;
}

void bgzf_dec_free(BgzfDec* D) {   // the streams are idle (bgzf_free synchronised them)
    if (!D) return;
    for (int b = 0; b < 2; ++b) {
        if (D->h_in[b]) (void)hipHostFree(D->h_in[b]);
        if (D->h_out[b]) (void)hipHostFree(D->h_out[b]);
        if (D->h_desc[b]) (void)hipHostFree(D->h_desc[b]);
        if (D->h_ok[b]) (void)hipHostFree(D->h_ok[b]);
        if (D->d_in[b]) (void)hipFree(D->d_in[b]);
        if (D->d_out[b]) (void)hipFree(D->d_out[b]);
        if (D->d_desc[b]) (void)hipFree(D->d_desc[b]);
        if (D->d_ok[b]) (void)hipFree(D->d_ok[b]);
        for (int k = 0; k < 6; ++k)
            if (D->ev[b][k]) (void)hipEventDestroy(D->ev[b][k]);
    }
    for (auto& r : D->res) (void)hipFree(r.second.p);
    crc_bufs_free(&D->cb);
    delete D;
}

void bgzf_dec_prof(cc_ctx* ctx, bool reset, double* ms, int64_t* n, double* h2d, double* d2h) {
    BgzfEnc* E;
    {
        std::lock_guard<std::mutex> lk(ctx->bgzf_mu);
        E = ctx->bgzf;
    }
    if (!E) return;
    std::lock_guard<std::mutex> lk(E->mu);
    BgzfDec* D = E->dec;
    if (!D) return;
    if (reset) { D->prof_ms = D->h2d_ms = D->d2h_ms = 0; D->prof_n = 0; }
    if (ms) *ms = D->prof_ms;
    if (n) *n = D->prof_n;
    if (h2d) *h2d = D->h2d_ms;
    if (d2h) *d2h = D->d2h_ms;
}

// the device (and the inflater's buffers) ready for a call on the encoder's streams
int bgzf_dec_enter(cc_ctx* ctx, BgzfEnc* E) {
    if (E->broken) return CC_E_HIP;
    BGCHK(hipSetDevice(ctx->device));   // (not enter(): a reader's thread, the switches are the engine thread's)
    if (!E->dec) E->dec = new BgzfDec();
    if (!E->dec->ready) RC(bgzf_dec_init(E, E->dec));
    return 0;
}

Resident* resident_find(BgzfEnc* E, int64_t id) {
    if (!E->dec) return nullptr;
    auto it = E->dec->res.find(id);
    return it == E->dec->res.end() ? nullptr : &it->second;
}

// cc_bgzf_inflate's work.  Rounds of at most BI_ROUND members (and BI_IN_CAP / BI_OUT_CAP bytes)
// alternate between the two streams, each with its own pinned and device buffers: while one round's
// kernel runs, the previous round's bytes are copied out to the caller and the next one's are packed.
// With a resident stream R (cc_bgzf_inflate_keep) the kernel writes member j at R's byte uoff[j]
// instead of into the round's output buffer: the round's base is its first member's uoff, desc.z the
// 32-bit distance from it, and the round's download is its span of R.
// With crc (cc_bgzf_inflate_crc, cc_bgzf_inflate_keep_crc) every round's k_bgzf_inflate is followed on
// its stream by k_crc32 over the same descriptors and output base, and crc[j], the CRC32 of the bytes
// the device wrote for member j, comes back with the status words (0 where ok[j] == 0).
int64_t bgzf_decode(cc_ctx* ctx, BgzfEnc* E, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen,
                    const uint64_t* uoff, const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok,
                    const Resident* R = nullptr, uint32_t* crc = nullptr) {
    if (members == 0) return 0;
    if (members < 0 || !comp || !coff || !clen || !uoff || !ulen || !out || !ok) {
        E->err = "cc_bgzf_inflate: null argument or a negative member count";
        return CC_E_INVALID;
    }
    RC(bgzf_dec_enter(ctx, E));
    BgzfDec* D = E->dec;
    const bool prof = ctx->profiling;
    if (crc) BGCHK(crc_bufs_init(&D->cb, BI_ROUND));
    // the rounds: [first[k], first[k + 1]) of the members the device takes (BGZF's bounds; others stay ok = 0)
    std::vector<int64_t> idx, first;
    std::vector<uint64_t> rbase, rspan;   // with R: each round's lowest byte of R and the bytes it spans
    {
        size_t in_b = 0, out_b = 0;
        uint64_t base = 0;
        int n = 0;
        first.push_back(0);
        for (int64_t j = 0; j < members; ++j) {
            ok[j] = 0;
            if (crc) crc[j] = 0;
            if (clen[j] > BI_MEMBER || ulen[j] > BI_MEMBER) continue;
            const size_t ib = bi_align(clen[j]);
            // the round's output bytes with this member: packed 16-B slots, or with R the span from its base
            const bool below = R && uoff[j] < base;
            auto with = [&](size_t have, uint64_t from) {
                return R ? std::max(have, (size_t)(uoff[j] - from) + ulen[j]) : have + bi_align(ulen[j]);
            };
            if (n > 0 && (n == BI_ROUND || in_b + ib > BI_IN_CAP || below || with(out_b, base) > BI_OUT_CAP)) {
                first.push_back((int64_t)idx.size());
                rbase.push_back(base);
                rspan.push_back(out_b);
                in_b = out_b = 0;
                n = 0;
            }
            if (n == 0) base = uoff[j];
            idx.push_back(j);
            in_b += ib;
            out_b = with(out_b, base);
            ++n;
        }
        first.push_back((int64_t)idx.size());
        rbase.push_back(base);
        rspan.push_back(out_b);
    }
    const int64_t rounds = (int64_t)first.size() - 1;
    if (idx.empty()) return members;
    auto launch = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        const int n = (int)(first[k + 1] - first[k]);
        size_t in_b = 0, out_b = 0;
        for (int i = 0; i < n; ++i) {
            const int64_t j = idx[(size_t)(first[k] + i)];
            memcpy(D->h_in[b] + in_b, comp + coff[j], clen[j]);
            D->h_desc[b][i] = make_uint4((uint32_t)in_b, clen[j], R ? (uint32_t)(uoff[j] - rbase[k]) : (uint32_t)out_b, ulen[j]);
            in_b += bi_align(clen[j]);
            out_b += bi_align(ulen[j]);
        }
        uint8_t* const d_base = R ? R->p + rbase[k] : D->d_out[b];
        if (R) out_b = (size_t)rspan[k];
        D->timed[b] = prof;
        if (prof) BGCHK(hipEventRecord(D->ev[b][2], E->st[b]));
        if (in_b) BGCHK(hipMemcpyAsync(D->d_in[b], D->h_in[b], in_b, hipMemcpyHostToDevice, E->st[b]));
        BGCHK(hipMemcpyAsync(D->d_desc[b], D->h_desc[b], (size_t)n * sizeof(uint4), hipMemcpyHostToDevice, E->st[b]));
        if (prof) BGCHK(hipEventRecord(D->ev[b][3], E->st[b]));
        if (prof) BGCHK(hipEventRecord(D->ev[b][0], E->st[b]));
        klaunch(E->st[b], k_bgzf_inflate, (unsigned)n, BI_T, D->d_in[b], D->d_desc[b], d_base, D->d_ok[b], n);
        BGCHK(hipGetLastError());
        if (prof) BGCHK(hipEventRecord(D->ev[b][1], E->st[b]));
        if (crc) {
            D->cb.timed[b] = prof;
            BGCHK(crc_launch(E->st[b], prof ? D->cb.ev[b] : nullptr, d_base, D->d_desc[b], CR_MEMBER, 0, D->cb.d[b], n));
        }
        if (prof) BGCHK(hipEventRecord(D->ev[b][4], E->st[b]));
        if (out_b) BGCHK(hipMemcpyAsync(D->h_out[b], d_base, out_b, hipMemcpyDeviceToHost, E->st[b]));
        BGCHK(hipMemcpyAsync(D->h_ok[b], D->d_ok[b], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st[b]));
        if (crc) BGCHK(hipMemcpyAsync(D->cb.h[b], D->cb.d[b], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st[b]));
        if (prof) BGCHK(hipEventRecord(D->ev[b][5], E->st[b]));
        return 0;
    };
    int64_t good = 0;
    auto finish = [&](int64_t k) -> int {
        const int b = (int)(k & 1);
        const int n = (int)(first[k + 1] - first[k]);
        BGCHK(hipStreamSynchronize(E->st[b]));
        if (D->timed[b]) {
            float ms = 0;
            BGCHK(hipEventElapsedTime(&ms, D->ev[b][0], D->ev[b][1]));
            D->prof_ms += ms;
            D->prof_n += 1;
            BGCHK(hipEventElapsedTime(&ms, D->ev[b][2], D->ev[b][3]));
            D->h2d_ms += ms;
            BGCHK(hipEventElapsedTime(&ms, D->ev[b][4], D->ev[b][5]));
            D->d2h_ms += ms;
        }
        if (crc) RC(crc_prof_add(E, &D->cb, b));
        for (int i = 0; i < n; ++i) {
            if (D->h_ok[b][i] != 1) continue;
            const int64_t j = idx[(size_t)(first[k] + i)];
            memcpy(out + uoff[j], D->h_out[b] + D->h_desc[b][i].z, ulen[j]);
            if (crc) crc[j] = D->cb.h[b][i];
            ok[j] = 1;
            ++good;
        }
        return 0;
    };
    // on any failure both streams are drained before the buffers can be touched again
    auto drained = [&](int rc) {
        if (rc)
            for (int b = 0; b < 2; ++b) (void)hipStreamSynchronize(E->st[b]);
        return rc;
    };
#define BIRC(x) do { int rc_ = drained(x); if (rc_) return rc_; } while (0)
    for (int64_t k = 0; k < rounds; ++k) {
        BIRC(launch(k));
        if (k >= 1) BIRC(finish(k - 1));
    }
    BIRC(finish(rounds - 1));
#undef BIRC
    return members - good;
}

// cc_bgzf_inflate_keep's work: the members' ranges checked against total and each other, a resident
// stream allocated (its tail zeroed) and bgzf_decode run into it.  Without device memory for it the
// call is cc_bgzf_inflate's and *id stays 0.
int64_t bgzf_decode_keep(cc_ctx* ctx, BgzfEnc* E, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen,
                         const uint64_t* uoff, const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok,
                         uint64_t total, int64_t* id, uint32_t* crc = nullptr) {
    *id = 0;
    if (members < 0 || (members > 0 && (!comp || !coff || !clen || !uoff || !ulen || !out || !ok))) {
        E->err = "cc_bgzf_inflate_keep: null argument or a negative member count";
        return CC_E_INVALID;
    }
    bool ordered = true;   // (the readers' members come in file order: no sort then)
    for (int64_t j = 0; j < members; ++j) {
        if (uoff[j] > total || ulen[j] > total - uoff[j]) {
            E->err = "cc_bgzf_inflate_keep: member " + std::to_string((long long)j) + " does not lie inside total";
            return CC_E_INVALID;
        }
        if (j > 0 && uoff[j] < uoff[j - 1] + ulen[j - 1]) ordered = false;
    }
    if (!ordered) {
        std::vector<int64_t> by;
        for (int64_t j = 0; j < members; ++j)
            if (ulen[j]) by.push_back(j);
        std::sort(by.begin(), by.end(), [&](int64_t a, int64_t b) { return uoff[a] < uoff[b]; });
        for (size_t i = 1; i < by.size(); ++i)
            if (uoff[by[i]] < uoff[by[i - 1]] + ulen[by[i - 1]]) {
                E->err = "cc_bgzf_inflate_keep: members " + std::to_string((long long)by[i - 1]) + " and " +
                         std::to_string((long long)by[i]) + " overlap";
                return CC_E_INVALID;
            }
    }
    RC(bgzf_dec_enter(ctx, E));
    Resident R;
    R.total = total;
    const size_t padded = bi_align((size_t)total) + 32;
    if (hipMalloc((void**)&R.p, padded) != hipSuccess) {
        (void)hipGetLastError();   // (out of memory is no reason for the latch)
        return bgzf_decode(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, nullptr, crc);
    }
    int64_t r = CC_E_HIP;
    hipError_t e = hipMemsetAsync(R.p + total, 0, padded - (size_t)total, E->st[0]);
    if (e == hipSuccess) e = hipStreamSynchronize(E->st[0]);
    if (e != hipSuccess) {
        E->err = std::string("HIP error ") + hipGetErrorString(e) + " zeroing a resident stream's tail";
        E->broken = true;
    } else {
        r = bgzf_decode(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, &R, crc);
    }
    if (r < 0) {   // (bgzf_decode drained both streams)
        (void)hipFree(R.p);
        return r;
    }
    *id = g_resident_next.fetch_add(1);
    E->dec->res[*id] = R;
    return r;
}

int resident_patch(cc_ctx* ctx, BgzfEnc* E, int64_t id, uint64_t off, const uint8_t* bytes, uint64_t n) {
    const Resident* R = resident_find(E, id);
    if (!R || off > R->total || n > R->total - off || (n > 0 && !bytes)) {
        E->err = R ? "cc_resident_patch: the range does not lie inside the stream" : "cc_resident_patch: unknown id";
        return CC_E_INVALID;
    }
    if (n == 0) return 0;
    RC(bgzf_dec_enter(ctx, E));
    BGCHK(hipMemcpyAsync(R->p + off, bytes, (size_t)n, hipMemcpyHostToDevice, E->st[0]));
    BGCHK(hipStreamSynchronize(E->st[0]));
    return 0;
}

// ccio_inflate_fn over a context: a HIP failure is a nonzero return (the readers then use the host codec)
int bgzf_inflate_hook_fn(void* user, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen, const uint64_t* uoff,
                         const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok) {
    cc_ctx* ctx = (cc_ctx*)user;
    if (!ctx) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return bgzf_decode(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok) < 0 ? 1 : 0;
}

// ccio_inflate_keep_fn and ccio_resident_patch_fn over a context, likewise
int bgzf_keep_hook_fn(void* user, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen, const uint64_t* uoff,
                      const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok, uint64_t total, int64_t* token) {
    cc_ctx* ctx = (cc_ctx*)user;
    if (!ctx || !token) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return bgzf_decode_keep(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, total, token) < 0 ? 1 : 0;
}

// ccio_inflate_crc_fn and ccio_inflate_keep_crc_fn over a context: the two above with the members' CRCs
int bgzf_inflate_crc_hook_fn(void* user, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen,
                             const uint64_t* uoff, const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok,
                             uint32_t* crc) {
    cc_ctx* ctx = (cc_ctx*)user;
    if (!ctx || !crc) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return bgzf_decode(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, nullptr, crc) < 0 ? 1 : 0;
}

int bgzf_keep_crc_hook_fn(void* user, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen, const uint64_t* uoff,
                          const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok, uint64_t total, int64_t* token,
                          uint32_t* crc) {
    cc_ctx* ctx = (cc_ctx*)user;
    if (!ctx || !token || !crc) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return bgzf_decode_keep(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, total, token, crc) < 0 ? 1 : 0;
}

// cc_crc32's and cc_resident_crc32's work: the CRC32 of n ranges of the device bytes [base, base +
// limit), whose allocation covers every aligned 16-byte word that overlaps them.  A range longer
// than a segment is cut on the host and its segments' CRCs are joined with crc_core.h's combine.
int crc_ranges(cc_ctx* ctx, BgzfEnc* E, const char* who, const uint8_t* base, uint64_t limit, const uint64_t* off,
               const uint64_t* len, int64_t n, uint32_t* out) {
    std::vector<uint4> seg;
    for (int64_t i = 0; i < n; ++i) {
        if (off[i] > limit || len[i] > limit - off[i]) {
            E->err = std::string(who) + ": range " + std::to_string((long long)i) + " does not lie inside the bytes";
            return CC_E_INVALID;
        }
        for (uint64_t o = 0; o < len[i]; o += crc::SEGMENT) {
            const uint64_t a = off[i] + o;
            seg.push_back(make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)std::min<uint64_t>(crc::SEGMENT, len[i] - o), 0));
        }
    }
    if (seg.size() > 0x7fffffffu) {
        E->err = std::string(who) + ": too many segments for one call";
        return CC_E_INVALID;
    }
    std::vector<uint32_t> got(seg.size());
    if (!seg.empty()) {
        const bool prof = ctx->profiling;
        uint4* d_seg = nullptr;
        uint32_t* d_crc = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        hipError_t e = hipMalloc((void**)&d_seg, seg.size() * sizeof(uint4));
        if (e == hipSuccess) e = hipMalloc((void**)&d_crc, seg.size() * sizeof(uint32_t));
        for (int k = 0; k < 2 && prof && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
        if (e == hipSuccess) e = hipMemcpyAsync(d_seg, seg.data(), seg.size() * sizeof(uint4), hipMemcpyHostToDevice, E->st[0]);
        if (e == hipSuccess) e = crc_launch(E->st[0], prof ? ev : nullptr, base, d_seg, CR_SEG, 0, d_crc, (int)seg.size());
        if (e == hipSuccess) e = hipMemcpyAsync(got.data(), d_crc, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st[0]);
        const hipError_t es = hipStreamSynchronize(E->st[0]);   // (also after a failure: the buffers are freed below)
        if (e == hipSuccess) e = es;
        float ms = 0;
        if (e == hipSuccess && prof) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        if (e == hipSuccess && prof) { E->crc_ms += ms; E->crc_n += 1; }
        for (int k = 0; k < 2; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        if (d_seg) (void)hipFree(d_seg);
        if (d_crc) (void)hipFree(d_crc);
        BGCHK(e);
    }
    size_t s = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t c = 0;
        for (uint64_t o = 0; o < len[i]; o += crc::SEGMENT, ++s)
            c = o ? crc::combine(c, got[s], std::min<uint64_t>(crc::SEGMENT, len[i] - o)) : got[s];
        out[i] = c;
    }
    return 0;
}

// cc_bgzf_deflate_resident's work: the range checked against the stream, then bgzf_encode over the
// device bytes themselves (the caller holds the mutex)
int64_t bgzf_encode_resident(cc_ctx* ctx, BgzfEnc* E, int64_t id, uint64_t off, uint64_t n, uint8_t* stage, uint64_t slot,
                             uint32_t* out_len, int64_t cap) {
    const Resident* R = resident_find(E, id);
    if (!R) { E->err = "cc_bgzf_deflate_resident: unknown id"; return CC_E_INVALID; }
    if (off % 256) { E->err = "cc_bgzf_deflate_resident: off is not a multiple of 256"; return CC_E_INVALID; }
    if (off > R->total || n > R->total - off) {
        E->err = "cc_bgzf_deflate_resident: the range does not lie inside the stream";
        return CC_E_INVALID;
    }
    return bgzf_encode(ctx, E, nullptr, n, stage, slot, out_len, cap, R->p + off);
}

// cc_resident_put's work: host bytes as a resident stream (the caller holds the mutex)
int resident_put(cc_ctx* ctx, BgzfEnc* E, const uint8_t* bytes, uint64_t n, int64_t* id) {
    *id = 0;
    if (n > 0 && !bytes) { E->err = "cc_resident_put: null bytes"; return CC_E_INVALID; }
    if (E->broken) return CC_E_HIP;
    BGCHK(hipSetDevice(ctx->device));
    RC(bgzf_streams(E));
    Resident R;
    R.total = n;
    const size_t padded = bi_align((size_t)n) + 32;
    if (hipMalloc((void**)&R.p, padded) != hipSuccess) {
        (void)hipGetLastError();   // (out of memory is no reason for the latch)
        E->err = "cc_resident_put: no device memory for the stream";
        return CC_E_HIP;
    }
    const bool prof = ctx->profiling;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && prof && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    if (e == hipSuccess && prof) e = hipEventRecord(ev[0], E->st[0]);
    if (e == hipSuccess && n) e = hipMemcpyAsync(R.p, bytes, (size_t)n, hipMemcpyHostToDevice, E->st[0]);
    if (e == hipSuccess) e = hipMemsetAsync(R.p + n, 0, padded - (size_t)n, E->st[0]);
    if (e == hipSuccess && prof) e = hipEventRecord(ev[1], E->st[0]);
    const hipError_t es = hipStreamSynchronize(E->st[0]);
    if (e == hipSuccess) e = es;
    float ms = 0;
    if (e == hipSuccess && prof) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    if (e == hipSuccess && prof) { E->put_ms += ms; E->put_n += 1; }
    for (int k = 0; k < 2; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (e != hipSuccess) {
        (void)hipFree(R.p);
        BGCHK(e);
    }
    if (!E->dec) E->dec = new BgzfDec();
    *id = g_resident_next.fetch_add(1);
    E->dec->res[*id] = R;
    return 0;
}

// [off, off + n) of a resident stream copied to dst (the caller holds the mutex)
int resident_fetch_range(cc_ctx* ctx, BgzfEnc* E, int64_t id, uint64_t off, uint64_t n, uint8_t* dst) {
    const Resident* R = resident_find(E, id);
    if (!R || off > R->total || n > R->total - off || (n > 0 && !dst)) {
        E->err = R ? "cc_resident_fetch: the range does not lie inside the stream" : "cc_resident_fetch: unknown id";
        return CC_E_INVALID;
    }
    if (n == 0) return 0;
    if (E->broken) return CC_E_HIP;
    BGCHK(hipSetDevice(ctx->device));
    RC(bgzf_streams(E));
    BGCHK(hipMemcpyAsync(dst, R->p + off, (size_t)n, hipMemcpyDeviceToHost, E->st[0]));
    BGCHK(hipStreamSynchronize(E->st[0]));
    return 0;
}

int bgzf_patch_hook_fn(void* user, int64_t token, uint64_t off, const uint8_t* bytes, uint64_t n) {
    cc_ctx* ctx = (cc_ctx*)user;
    if (!ctx) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return resident_patch(ctx, E, token, off, bytes, n) ? 1 : 0;
}

}  // namespace

extern "C" {

int64_t cc_bgzf_inflate(cc_ctx* ctx, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen, const uint64_t* uoff,
                        const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int64_t r = bgzf_decode(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok);
    if (r < 0) ctx->err = E->err;
    return r;
}

int cc_bgzf_inflate_hook(cc_ctx* ctx, ccio_inflate_fn* fn, void** user) {
    if (!ctx || !fn || !user) return CC_E_INVALID;
    *fn = bgzf_inflate_hook_fn;
    *user = ctx;
    return 0;
}

int64_t cc_bgzf_inflate_keep(cc_ctx* ctx, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen,
                             const uint64_t* uoff, const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok,
                             uint64_t total, int64_t* resident_id) {
    if (!ctx || !resident_id) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int64_t r = bgzf_decode_keep(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, total, resident_id);
    if (r < 0) ctx->err = E->err;
    return r;
}

int cc_bgzf_inflate_keep_hook(cc_ctx* ctx, ccio_inflate_keep_fn* keep, ccio_resident_patch_fn* patch, void** user) {
    if (!ctx || !keep || !patch || !user) return CC_E_INVALID;
    *keep = bgzf_keep_hook_fn;
    *patch = bgzf_patch_hook_fn;
    *user = ctx;
    return 0;
}

int cc_resident_patch(cc_ctx* ctx, int64_t id, uint64_t off, const uint8_t* bytes, uint64_t n) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int rc = resident_patch(ctx, E, id, off, bytes, n);
    if (rc) ctx->err = E->err;
    return rc;
}

int cc_resident_free(cc_ctx* ctx, int64_t id) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const Resident* R = resident_find(E, id);
    if (!R) { ctx->err = "cc_resident_free: unknown id"; return CC_E_INVALID; }
    (void)hipSetDevice(ctx->device);
    for (int b = 0; b < 2; ++b)   // (every call that touches a stream waits before it returns: idle already)
        if (E->st[b]) (void)hipStreamSynchronize(E->st[b]);
    (void)hipFree(R->p);
    E->dec->res.erase(id);
    return 0;
}

// test hooks: a resident stream's bytes (its total; at most cap of them go to dst), and how many live
int64_t cc_resident_fetch(cc_ctx* ctx, int64_t id, uint8_t* dst, uint64_t cap) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const Resident* R = resident_find(E, id);
    if (!R) { ctx->err = "cc_resident_fetch: unknown id"; return CC_E_INVALID; }
    const size_t nb = (size_t)std::min<uint64_t>(cap, R->total);
    if (dst && nb) {
        RC(bgzf_dec_enter(ctx, E));
        hipError_t e = hipMemcpyAsync(dst, R->p, nb, hipMemcpyDeviceToHost, E->st[0]);
        if (e == hipSuccess) e = hipStreamSynchronize(E->st[0]);
        if (e != hipSuccess) {
            E->broken = true;
            ctx->err = E->err = std::string("HIP error ") + hipGetErrorString(e) + " fetching a resident stream";
            return CC_E_HIP;
        }
    }
    return (int64_t)R->total;
}

int64_t cc_bgzf_deflate_resident(cc_ctx* ctx, int64_t id, uint64_t off, uint64_t n, uint8_t* stage, uint64_t slot,
                                 uint32_t* out_len, int64_t cap) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int64_t r = bgzf_encode_resident(ctx, E, id, off, n, stage, slot, out_len, cap);
    if (r < 0) ctx->err = E->err;
    return r;
}

int cc_resident_put(cc_ctx* ctx, const uint8_t* bytes, uint64_t n, int64_t* id) {
    if (!ctx || !id) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int rc = resident_put(ctx, E, bytes, n, id);
    if (rc) ctx->err = E->err;
    return rc;
}

int64_t cc_resident_count(cc_ctx* ctx) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return E->dec ? (int64_t)E->dec->res.size() : 0;
}

int64_t cc_bgzf_inflate_crc(cc_ctx* ctx, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen,
                            const uint64_t* uoff, const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok,
                            uint32_t* crc) {
    if (!ctx || (members > 0 && !crc)) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int64_t r = bgzf_decode(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, nullptr, crc);
    if (r < 0) ctx->err = E->err;
    return r;
}

int cc_bgzf_inflate_crc_hook(cc_ctx* ctx, ccio_inflate_crc_fn* fn, void** user) {
    if (!ctx || !fn || !user) return CC_E_INVALID;
    *fn = bgzf_inflate_crc_hook_fn;
    *user = ctx;
    return 0;
}

int64_t cc_bgzf_inflate_keep_crc(cc_ctx* ctx, const uint8_t* comp, const uint64_t* coff, const uint32_t* clen,
                                 const uint64_t* uoff, const uint32_t* ulen, int64_t members, uint8_t* out, uint8_t* ok,
                                 uint64_t total, int64_t* resident_id, uint32_t* crc) {
    if (!ctx || !resident_id || (members > 0 && !crc)) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int64_t r = bgzf_decode_keep(ctx, E, comp, coff, clen, uoff, ulen, members, out, ok, total, resident_id, crc);
    if (r < 0) ctx->err = E->err;
    return r;
}

int cc_bgzf_inflate_keep_crc_hook(cc_ctx* ctx, ccio_inflate_keep_crc_fn* keep, ccio_resident_patch_fn* patch, void** user) {
    if (!ctx || !keep || !patch || !user) return CC_E_INVALID;
    *keep = bgzf_keep_crc_hook_fn;
    *patch = bgzf_patch_hook_fn;
    *user = ctx;
    return 0;
}

int cc_crc32(cc_ctx* ctx, const uint8_t* data, uint64_t nbytes, const uint64_t* off, const uint64_t* len, int64_t n,
             uint32_t* crc) {
    if (!ctx) return CC_E_INVALID;
    if (n == 0) return 0;
    if (n < 0 || !off || !len || !crc || (nbytes > 0 && !data)) {
        ctx->err = "cc_crc32: null argument or a negative range count";
        return CC_E_INVALID;
    }
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    auto work = [&]() -> int {
        if (E->broken) return CC_E_HIP;
        BGCHK(hipSetDevice(ctx->device));
        RC(bgzf_streams(E));
        // the upload, padded like a resident stream: every aligned word that overlaps a range is allocated
        uint8_t* d = nullptr;
        if (hipMalloc((void**)&d, bi_align((size_t)nbytes) + 32) != hipSuccess) {
            (void)hipGetLastError();   // (out of memory is no reason for the latch)
            E->err = "cc_crc32: no device memory for the bytes";
            return CC_E_HIP;
        }
        hipError_t e = nbytes ? hipMemcpyAsync(d, data, (size_t)nbytes, hipMemcpyHostToDevice, E->st[0]) : hipSuccess;
        int rc = 0;
        if (e == hipSuccess) rc = crc_ranges(ctx, E, "cc_crc32", d, nbytes, off, len, n, crc);
        (void)hipStreamSynchronize(E->st[0]);
        (void)hipFree(d);
        BGCHK(e);
        return rc;
    };
    const int rc = work();
    if (rc) ctx->err = E->err;
    return rc;
}

int cc_resident_crc32(cc_ctx* ctx, int64_t id, const uint64_t* off, const uint64_t* len, int64_t n, uint32_t* crc) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const Resident* R = resident_find(E, id);
    int rc = 0;
    if (!R) {
        E->err = "cc_resident_crc32: unknown id";
        rc = CC_E_INVALID;
    } else if (n < 0 || (n > 0 && (!off || !len || !crc))) {
        E->err = "cc_resident_crc32: null argument or a negative range count";
        rc = CC_E_INVALID;
    } else if (n > 0) {
        rc = bgzf_dec_enter(ctx, E);
        if (!rc) rc = crc_ranges(ctx, E, "cc_resident_crc32", R->p, R->total, off, len, n, crc);
    }
    if (rc) ctx->err = E->err;
    return rc;
}

}  // extern "C"
