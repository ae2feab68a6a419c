// The device BGZF encoder (cc_bgzf_deflate, cc_bgzf_hook): included by cc_engine.hip after cc_ctx.
//
// k_bgzf_deflate: one workgroup per piece (<= 0xff00 bytes, the writers' cut).  The piece lives in
// LDS for the whole kernel.
//   pass 1, tile by tile (one position per thread): every position looks its 4-byte hash up in an
//     LDS table that holds only positions of EARLIER tiles, and tries distance 1; after a barrier
//     the tile's positions enter the table by atomic max, so what a position sees depends on the
//     bytes alone.  The greedy parse chain next[i] = i + max(1, len[i]) is resolved per wave by
//     pointer jumping (every position's exit from its 64-position segment), the segments' entry
//     points follow from eight LDS reads, and each wave marks the positions its entry reaches.
//     Tokens go to a per-piece array in device memory (indexed by position), their symbols to LDS
//     histograms.
//   codes: rank sort of the symbols in parallel, then deflate_core.h's serial builder (literal /
//     length tree, distance tree and header plan on three different waves).
//   form: the bits of a stored, a fixed and a dynamic block are counted; the smallest wins (stored
//     on a tie), so a member never exceeds 0xff00 + 5 + 26 bytes.
//   pass 2: token bit lengths are prefix-summed per tile and each token ORs its bits into the LDS
//     words the piece occupied (the piece is dead by then); the words are copied out with plain
//     vector stores.
// The CRC32 field is left to the host (it runs while the device encodes) unless cc_bgzf_set_crc is on:
// then k_crc32 (bgzf_crc32.hip.inc) takes the pieces' CRCs from the device input buffer and they come
// back with the lengths.
//
// The kernel is a template over the effort (cc_bgzf_set_effort).  Effort 1 is the encoder above.
// Effort 2 replaces pass 1's match finder and adds a lazy step; everything from the parse on is
// the same text:
//   buckets: a hash slot holds the four largest positions entered so far, sorted, as 16-bit
//     position + 1 in one 64-bit LDS word (a compare-and-swap insert: the content after any set of
//     inserts is the set's four largest, whatever their order).
//   same-tile visibility: the eight 64-position segments of a tile take turns; a wave reads its
//     lanes' buckets, then enters its own positions, then the workgroup meets at a barrier.  A
//     position therefore sees every hashed position before its own segment and none from it on:
//     a function of the bytes alone.  Distance 1 is still tried on its own.
//   lazy step: the finder runs one tile ahead of the parse, so position i knows len[i + 1] (also
//     across a tile's edge) and becomes a literal when len[i + 1] > len[i]; its successor is still
//     a function of i alone and the pointer-jumping parse is unchanged.
// With 64 KiB of buckets beside the resident piece effort 2 runs one workgroup per CU.
#include <mutex>

#include "deflate_core.h"

namespace {

constexpr int BG_T = 512;                 // threads = positions per tile
constexpr int BG_PIECE = 0xff00;
constexpr int BG_WORDS = BG_PIECE / 4 + 2;   // the piece and 8 bytes of zero padding (unaligned word reads)
constexpr int BG_SLOTS = 3072;            // hash slots: piece + table + the rest stay under 80 KiB (two workgroups per CU)
constexpr int BG_OSLOT = 0x10000 + 64;    // a member's slot in the device output
constexpr int BG_CHUNK = 256;             // pieces per launch
constexpr uint32_t BG_NONE = 0xffffffffu; // a position that starts no token
constexpr int BG2_WAYS = 4;               // effort 2: positions per bucket (16 bits each, one 64-bit word)
constexpr int BG2_SLOTS = 8192;           // effort 2: buckets (64 KiB: with the piece under the CU's 160 KiB)

template <int EFFORT> struct BgTab { typedef uint32_t T; static constexpr int N = BG_SLOTS; };
template <> struct BgTab<2> { typedef unsigned long long T; static constexpr int N = BG2_SLOTS; };

struct BgCodes {   // built after pass 1 in the hash table's LDS
    uint32_t lfreq[288], dfreq[32];
    uint32_t lval[288], dval[32];
    uint16_t lsym[288], dsym[32];
    uint8_t llen[288], dlen[32];
    uint16_t lcode[288], dcode[32];
    uint32_t work0[dfl::WORK], work1[dfl::WORK];
    dfl::DynHeader hdr;
};
static_assert(sizeof(BgCodes) <= BG_SLOTS * sizeof(uint32_t), "the code tables reuse the hash table's LDS");
static_assert(BG2_WAYS * 16 == 64 && BG_PIECE < 0xffff, "a bucket is one 64-bit word of position + 1 in 16 bits");

struct BgSink {   // the header writer's bit sink: one thread, plain ORs into zeroed LDS words
    uint32_t* w;
    uint32_t pos;
    __host__ __device__ void put(uint32_t v, int nb) {
        if (nb <= 0) return;
        const uint32_t i = pos >> 5, sh = pos & 31;   // each word guarded on its own: a payload may end in the last word
        if (i < (uint32_t)BG_WORDS) w[i] |= v << sh;
        if (sh + (uint32_t)nb > 32 && i + 1 < (uint32_t)BG_WORDS) w[i + 1] |= v >> (32 - sh);
        pos += (uint32_t)nb;
    }
};

__device__ inline uint32_t bg_load32(const uint32_t* W, int pos) {
    const int w = pos >> 2;
    const uint64_t v = ((uint64_t)W[w + 1] << 32) | W[w];
    return (uint32_t)(v >> ((pos & 3) * 8));
}

// bytes that agree at c and i (c < i), at most maxl (<= n - i: no read passes the padding)
__device__ inline int bg_extend(const uint32_t* W, int c, int i, int maxl) {
    int l = 0;
    while (l < maxl) {
        const uint32_t x = bg_load32(W, i + l) ^ bg_load32(W, c + l);
        if (x) { l += __builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    return l < maxl ? l : maxl;
}

// bucket b (16-bit fields, the largest in the low bits, 0: empty) with p entered: the four largest
__device__ inline unsigned long long bg_bucket_with(unsigned long long b, uint32_t p) {
    int k = 0;   // fields above p
#pragma unroll
    for (int w = 0; w < BG2_WAYS; ++w) k += (uint32_t)((b >> (16 * w)) & 0xffff) > p;
    if (k == BG2_WAYS) return b;
    const unsigned long long lo = (1ull << (16 * k)) - 1;   // k <= 3
    return (b & lo) | ((unsigned long long)p << (16 * k)) | ((b & ~lo) << 16);
}

// A tile's parse, tokens and histogram counts: position i = tb + tid offers (len, dist), len 0: a
// literal.  carry: the first position no earlier token covers (the same in every thread).
__device__ __forceinline__ void bg_parse_tile(const int tb, const int i, const int n, const int len, const int dist,
                                          int& carry, uint16_t* s_exit, uint32_t* s_lhist, uint32_t* s_dhist,
                                          const uint8_t* s_bytes, uint32_t* tokp) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nxt = i + (len ? len : 1);
    const int wb = tb + (tid & ~63), we = wb + 64;
    int E = nxt;   // where the chain from this position leaves the wave's segment
    for (int it = 0; it < 6; ++it) {
        const bool in_seg = E < we;
        const int v = __shfl(E, in_seg ? E - wb : lane);
        if (in_seg) E = v;
    }
    s_exit[tid] = (uint16_t)(E - tb);
    __syncthreads();
    int s = carry, mystart = 0x7fffffff;
    for (int c = 0; c < BG_T / 64; ++c)
        if (s < tb + 64 * c + 64) {
            if (c == wv) mystart = s;
            s = tb + (int)s_exit[s - tb];
        }
    carry = s;
    uint64_t mask = 0;
    int p = __builtin_amdgcn_readfirstlane(mystart);
    while (p < we) {
        mask |= 1ull << (p - wb);
        p = __builtin_amdgcn_readlane(nxt, p - wb);
    }
    if (i < n) {
        uint32_t t = BG_NONE;
        if ((mask >> lane) & 1) {
            if (len) {
                int eb, ev;
                t = dfl::tok_match(len, dist);
                atomicAdd(&s_lhist[dfl::len_sym(len, &eb, &ev)], 1u);
                atomicAdd(&s_dhist[dfl::dist_sym(dist, &eb, &ev)], 1u);
            } else {
                t = dfl::tok_lit(s_bytes[i]);
                atomicAdd(&s_lhist[t], 1u);
            }
        }
        tokp[i] = t;
    }
}

// (flatten: with two instantiations deflate_core.h's builders have two callers each and would no
// longer be inlined as they are into a single kernel)
template <int EFFORT>
__global__ __launch_bounds__(BG_T) __attribute__((flatten)) void k_bgzf_deflate(const uint8_t* __restrict__ in, uint64_t n_total,
                                                       uint32_t* __restrict__ tok, uint8_t* __restrict__ out,
                                                       uint32_t* __restrict__ out_len) {
    __shared__ uint32_t s_data[BG_WORDS];
    __shared__ typename BgTab<EFFORT>::T s_tab[BgTab<EFFORT>::N];
    __shared__ uint32_t s_lhist[288], s_dhist[32];
    __shared__ uint16_t s_exit[BG_T];
    __shared__ uint32_t s_wsum[BG_T / 64];
    __shared__ uint32_t s_misc[4];   // bits of the fixed block, of the dynamic block, the payload's first free bit
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t off = (uint64_t)blockIdx.x * BG_PIECE;
    const int n = (int)(n_total - off < (uint64_t)BG_PIECE ? n_total - off : (uint64_t)BG_PIECE);
    const uint8_t* src = in + off;   // 256-byte aligned: the input buffer is, and so is every piece's offset
    uint32_t* tokp = tok + (uint64_t)blockIdx.x * BG_PIECE;
    const uint8_t* s_bytes = (const uint8_t*)s_data;

    for (int w = tid; w < BG_WORDS; w += BG_T) {
        const int b = 4 * w;
        uint32_t v = 0;
        if (b + 4 <= n) v = *(const uint32_t*)(src + b);
        else
            for (int k = 0; k < 4; ++k)
                if (b + k < n) v |= (uint32_t)src[b + k] << (8 * k);
        s_data[w] = v;
    }
    for (int k = tid; k < BgTab<EFFORT>::N; k += BG_T) s_tab[k] = 0;
    if (tid < 288) s_lhist[tid] = 0;
    if (tid < 32) s_dhist[tid] = 0;
    if (tid < 4) s_misc[tid] = 0;
    __syncthreads();

    // ---- pass 1: matches, parse, tokens, histograms
    int carry = 0;
    if constexpr (EFFORT == 1) {
    for (int tb = 0; tb < n; tb += BG_T) {
        const int i = tb + tid;
        int len = 0, dist = 0;
        uint32_t slot = 0;
        bool hashed = false;
        if (i < n) {
            const int maxl = n - i < dfl::MAX_MATCH ? n - i : dfl::MAX_MATCH;
            if (i + 4 <= n) {
                hashed = true;
                slot = (((bg_load32(s_data, i) * 2654435761u) >> 16) * (uint32_t)BG_SLOTS) >> 16;
                const uint32_t c = s_tab[slot];   // position + 1 of an earlier tile, 0: none
                if (c) {
                    const int d = i - (int)(c - 1);
                    if (d > 0 && d <= dfl::WINDOW) {
                        const int l = bg_extend(s_data, (int)(c - 1), i, maxl);
                        if (l >= dfl::MIN_MATCH) { len = l; dist = d; }
                    }
                }
            }
            if (i >= 1 && len < maxl) {
                const int l1 = bg_extend(s_data, i - 1, i, maxl);
                if (l1 >= dfl::MIN_MATCH && l1 >= len) { len = l1; dist = 1; }
            }
            if (len == dfl::MIN_MATCH && dist > 4096) len = 0;   // three literals are cheaper
        }
        __syncthreads();   // every lookup of this tile precedes its inserts
        if (hashed) atomicMax(&s_tab[slot], (uint32_t)(i + 1));
        bg_parse_tile(tb, i, n, len, dist, carry, s_exit, s_lhist, s_dhist, s_bytes, tokp);
    }
    } else {
    __shared__ uint16_t s_len[BG_T + 2];   // the tile's lengths and the next tile's first
    // the matches of tile tb; its positions enter the buckets segment by segment (uniform barriers)
    auto find_tile = [&](const int tb, int& len, int& dist) {
        const int i = tb + tid;
        len = 0;
        dist = 0;
        const bool hashed = i + 4 <= n;
        uint32_t slot = 0;
        if (hashed) slot = (((bg_load32(s_data, i) * 2654435761u) >> 16) * (uint32_t)BG2_SLOTS) >> 16;   // < BG2_SLOTS
        // a position with four later positions of its own segment in its bucket would be pushed out
        // by them: runs skip the insert (the bucket's content is the same)
        bool enter = hashed;
        {
            bool covered = true;
#pragma unroll
            for (int k = 1; k <= BG2_WAYS; ++k) {
                const uint32_t sk = __shfl_down(hashed ? slot : 0xffffffffu, k);
                covered = covered && lane + k < 64 && sk == slot;
            }
            if (covered) enter = false;
        }
        unsigned long long seen = 0;   // the bucket before this segment's positions
        for (int sg = 0; sg < BG_T / 64; ++sg) {
            if (sg == wv && hashed) {
                seen = s_tab[slot];   // the whole wave reads before any of its lanes enters
                if (enter) {
                    unsigned long long old = seen;
                    for (;;) {
                        const unsigned long long nw = bg_bucket_with(old, (uint32_t)(i + 1));
                        if (nw == old) break;
                        const unsigned long long got = atomicCAS(&s_tab[slot], old, nw);
                        if (got == old) break;
                        old = got;
                    }
                }
            }
            __syncthreads();
        }
        if (i < n) {
            const int maxl = n - i < dfl::MAX_MATCH ? n - i : dfl::MAX_MATCH;
#pragma unroll
            for (int w = 0; w < BG2_WAYS; ++w) {   // nearest first: a farther one must be longer
                const int c = (int)((seen >> (16 * w)) & 0xffff);   // position + 1, 0: none
                const int d = i - (c - 1);
                if (c && d > 0 && d <= dfl::WINDOW && len < maxl && s_bytes[c - 1 + len] == s_bytes[i + len]) {
                    const int l = bg_extend(s_data, c - 1, i, maxl);
                    if (l >= dfl::MIN_MATCH && l > len) { len = l; dist = d; }
                }
            }
            if (i >= 1 && len < maxl) {
                const int l1 = bg_extend(s_data, i - 1, i, maxl);
                if (l1 >= dfl::MIN_MATCH && l1 >= len) { len = l1; dist = 1; }
            }
            if (len == dfl::MIN_MATCH && dist > 4096) len = 0;   // three literals are cheaper
        }
    };
    int len, dist;
    find_tile(0, len, dist);
    for (int tb = 0; tb < n; tb += BG_T) {
        int nlen = 0, ndist = 0;
        if (tb + BG_T < n) find_tile(tb + BG_T, nlen, ndist);
        s_len[tid] = (uint16_t)len;
        if (tid == 0) s_len[BG_T] = (uint16_t)nlen;   // of position tb + BG_T
        __syncthreads();
        if ((int)s_len[tid + 1] > len) len = 0;   // lazy: the next position's match is longer
        // (the parse's barrier separates these reads from the next tile's writes)
        bg_parse_tile(tb, tb + tid, n, len, dist, carry, s_exit, s_lhist, s_dhist, s_bytes, tokp);
        len = nlen;
        dist = ndist;
    }
    }
    __syncthreads();

    // ---- codes (the hash table is dead: its LDS holds the tables)
    BgCodes& C = *reinterpret_cast<BgCodes*>(s_tab);
    if (tid == 0) s_lhist[256] += 1;   // end of block
    __syncthreads();
    {
        const uint32_t lf = tid < dfl::NLIT ? s_lhist[tid] : 0;
        const uint32_t df = tid < dfl::NDIST ? s_dhist[tid] : 0;
        if (tid < 288) C.lfreq[tid] = lf;
        if (tid < 32) C.dfreq[tid] = df;
        const int ul = __syncthreads_count(lf != 0), ud = __syncthreads_count(df != 0);
        if (tid == 0) {
            dfl::ensure_two(C.lfreq, dfl::NLIT, ul);
            dfl::ensure_two(C.dfreq, dfl::NDIST, ud);
        }
        __syncthreads();
    }
    // rank sort by (count, symbol): threads 0..285 the literal/length symbols, 288..317 the distances
    int ml, md;
    {
        const bool isl = tid < dfl::NLIT, isd = tid >= 288 && tid < 288 + dfl::NDIST;
        const uint32_t* F = isd ? C.dfreq : C.lfreq;
        const int me = isd ? tid - 288 : tid, cnt = isd ? dfl::NDIST : dfl::NLIT;
        const uint32_t f = (isl || isd) ? F[me] : 0;
        if (f) {
            int r = 0;
            for (int j = 0; j < cnt; ++j) {
                const uint32_t g = F[j];
                r += g && (g < f || (g == f && j < me));
            }
            if (isd) { C.dval[r] = f; C.dsym[r] = (uint16_t)me; }
            else { C.lval[r] = f; C.lsym[r] = (uint16_t)me; }
        }
        ml = __syncthreads_count(isl && f);
        md = __syncthreads_count(isd && f);
    }
    if (tid == 0) { dfl::huffman_lengths(C.lval, ml); dfl::limit_lengths(C.lval, ml, 15, C.work0); }
    if (tid == 64) { dfl::huffman_lengths(C.dval, md); dfl::limit_lengths(C.dval, md, 15, C.work1); }
    if (tid < 288) C.llen[tid] = 0;
    if (tid < 32) C.dlen[tid] = 0;
    __syncthreads();
    if (tid < ml) C.llen[C.lsym[tid]] = (uint8_t)C.lval[tid];
    if (tid < md) C.dlen[C.dsym[tid]] = (uint8_t)C.dval[tid];
    __syncthreads();
    if (tid == 128) dfl::plan_header(C.llen, C.dlen, &C.hdr);
    {   // the three forms' sizes from the true histograms
        uint32_t fx = 0, dy = 0;
        if (tid < dfl::NLIT) {
            const uint32_t f = s_lhist[tid], e = (uint32_t)dfl::lit_extra_bits(tid);
            fx = f * ((uint32_t)dfl::fixed_lit_len(tid) + e);
            dy = f * (C.llen[tid] + e);
        } else if (tid >= 288 && tid < 288 + dfl::NDIST) {
            const uint32_t f = s_dhist[tid - 288], e = (uint32_t)dfl::dist_extra_bits(tid - 288);
            fx = f * (5 + e);
            dy = f * (C.dlen[tid - 288] + e);
        }
        if (fx) atomicAdd(&s_misc[0], fx);
        if (dy) atomicAdd(&s_misc[1], dy);
    }
    __syncthreads();
    const uint32_t fixed_bits = s_misc[0] + 3, dyn_bits = s_misc[1] + C.hdr.bits, stored_bits = 40 + 8 * (uint32_t)n;
    int form = dyn_bits < fixed_bits ? 2 : 1;
    if (stored_bits <= (form == 2 ? dyn_bits : fixed_bits)) form = 0;
    uint32_t plen;   // payload bytes
    if (form == 0) {
        plen = 5 + (uint32_t)n;
    } else {
        if (form == 1) {
            __syncthreads();   // the dynamic lengths were read above
            if (tid < 288) C.llen[tid] = (uint8_t)dfl::fixed_lit_len(tid);
            if (tid < 32) C.dlen[tid] = 5;
        }
        for (int w = tid; w < BG_WORDS; w += BG_T) s_data[w] = 0;   // the piece is dead: the payload's words
        __syncthreads();
        if (tid == 0) dfl::canonical_codes(C.llen, form == 1 ? 288 : dfl::NLIT, C.lcode, C.work0);
        if (tid == 64) dfl::canonical_codes(C.dlen, form == 1 ? 32 : dfl::NDIST, C.dcode, C.work1);
        if (tid == 128) {
            BgSink sink{s_data, 0};
            if (form == 1) sink.put(1u | (1u << 1), 3);
            else dfl::write_header(&C.hdr, sink);
            s_misc[2] = sink.pos;
        }
        __syncthreads();
        // ---- pass 2: bit offsets by prefix sum, bits ORed into LDS
        uint32_t base = s_misc[2];
        for (int tb = 0; tb < n; tb += BG_T) {
            const int i = tb + tid;
            uint64_t v = 0;
            int nb = 0;
            if (i < n) {
                const uint32_t t = tokp[i];   // written by this very thread in pass 1
                if (t != BG_NONE) nb = dfl::tok_bits(t, C.llen, C.lcode, C.dlen, C.dcode, &v);
            }
            uint32_t x = (uint32_t)nb;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            if (lane == 63) s_wsum[wv] = x;
            __syncthreads();
            uint32_t wbase = 0, tot = 0;
            for (int k = 0; k < BG_T / 64; ++k) {
                const uint32_t q = s_wsum[k];
                if (k < wv) wbase += q;
                tot += q;
            }
            if (nb) {
                const uint32_t o = base + wbase + x - (uint32_t)nb, w = o >> 5, sh = o & 31;
                // a Huffman form is chosen when it is at least one bit under stored, so its payload may
                // reach byte 5 + n - 1 = 65,284 of the 65,288 here: every word is guarded on its own
                // index (the guards only ever fail if the counted size was wrong)
                if (w < (uint32_t)BG_WORDS) atomicOr(&s_data[w], (uint32_t)(v << sh));
                if (sh + (uint32_t)nb > 32 && w + 1 < (uint32_t)BG_WORDS)
                    atomicOr(&s_data[w + 1], (uint32_t)(v >> (32 - sh)));
                if (sh + (uint32_t)nb > 64 && w + 2 < (uint32_t)BG_WORDS)
                    atomicOr(&s_data[w + 2], (uint32_t)(v >> (64 - sh)));
            }
            base += tot;
            __syncthreads();
        }
        if (tid == 0) {
            BgSink sink{s_data, base};
            sink.put(C.lcode[256], C.llen[256]);
        }
        plen = (base + C.llen[256] + 7) >> 3;
        if (plen > 5 + (uint32_t)n) plen = 5 + (uint32_t)n;   // the counted size bounds it (at most 5 + n): keeps every store in the slot
        __syncthreads();
    }

    // ---- the member: header, payload, ISIZE (the CRC32 word before it is the host's)
    uint8_t* m = out + (uint64_t)blockIdx.x * BG_OSLOT;
    const uint32_t bsize = plen + 26;
    if (tid < 18) {
        const uint8_t hd[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0, 0};
        uint8_t b = hd[tid];
        if (tid == 16) b = (uint8_t)((bsize - 1) & 0xff);
        if (tid == 17) b = (uint8_t)((bsize - 1) >> 8);
        m[tid] = b;
    }
    const uint32_t nn = (uint32_t)n;
    auto payload = [&](uint32_t k) -> uint32_t {
        if (form) return s_bytes[k];
        if (k >= 5) return s_bytes[k - 5];
        return k == 0 ? 1u : k == 1 ? (nn & 0xff) : k == 2 ? (nn >> 8) : k == 3 ? (~nn & 0xff) : ((~nn >> 8) & 0xff);
    };
    uint16_t* m16 = (uint16_t*)(m + 18);   // 2-byte aligned: slots are 64-byte multiples
    for (uint32_t k = (uint32_t)tid; 2 * k + 1 < plen; k += BG_T) m16[k] = (uint16_t)(payload(2 * k) | (payload(2 * k + 1) << 8));
    if (tid == 0 && (plen & 1)) m[18 + plen - 1] = (uint8_t)payload(plen - 1);
    if (tid >= 64 && tid < 72) {
        const int k = tid - 64;
        m[18 + plen + k] = k < 4 ? 0 : (uint8_t)(nn >> (8 * (k - 4)));
    }
    if (tid == 0) out_len[blockIdx.x] = bsize;
}

// the members of a launch side by side (each at a 4-byte boundary): the download moves compressed
// bytes only
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t* __restrict__ out, const uint32_t* __restrict__ len,
                                                   uint32_t* __restrict__ packed) {
    __shared__ uint32_t s_off;
    const int tid = (int)threadIdx.x, piece = (int)blockIdx.x;
    if (tid == 0) s_off = 0;
    __syncthreads();
    uint32_t a = 0;
    for (int j = tid; j < piece; j += 256) a += (len[j] + 3) >> 2;
    if (a) atomicAdd(&s_off, a);
    __syncthreads();
    const uint32_t words = (len[piece] + 3) >> 2;
    const uint32_t* srcw = (const uint32_t*)(out + (uint64_t)piece * BG_OSLOT);
    uint32_t* dst = packed + s_off;
    for (uint32_t w = (uint32_t)tid; w < words; w += 256) dst[w] = srcw[w];
}

uint32_t bg_crc_table(uint32_t crc, const uint8_t* p, size_t n) {   // when neither library loads
    static uint32_t T[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            T[i] = c;
        }
    });
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = T[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}

}  // namespace

struct BgzfDec;   // the inflater's buffers (bgzf_inflate.hip.inc): same streams, mutex and latch

struct BgzfEnc {
    std::mutex mu;          // one caller at a time (the writers' and readers' threads call concurrently)
    bool ready = false, broken = false, streams = false;
    int effort = 1;         // cc_bgzf_set_effort: read once per round, under mu
    bool crc_on = false;    // cc_bgzf_set_crc: likewise
    CrcBufs cb;             // the encoder's CRC values (made by the first round with crc_on)
    double crc_ms = 0;      // k_crc32 of every caller on these streams (scope bgzf_crc32)
    int64_t crc_n = 0;
    double idx_ms = 0;      // k_index_fields (scope index_fields)
    int64_t idx_n = 0;
    double put_ms = 0;      // cc_resident_put's uploads (scope resident_put)
    int64_t put_n = 0;
    BgzfDec* dec = nullptr;
    std::string err;
    hipStream_t st[2] = {nullptr, nullptr};
    uint8_t* h_in[2] = {nullptr, nullptr};
    uint8_t* h_out[2] = {nullptr, nullptr};
    uint32_t* h_len[2] = {nullptr, nullptr};
    uint8_t* d_in[2] = {nullptr, nullptr};
    uint8_t* d_out[2] = {nullptr, nullptr};
    uint32_t* d_pack[2] = {nullptr, nullptr};
    uint32_t* d_tok[2] = {nullptr, nullptr};
    uint32_t* d_len[2] = {nullptr, nullptr};
    hipEvent_t ev[2][6] = {};   // per stream: around the kernel, the upload, the download
    bool timed[2] = {false, false};
    bool up_timed[2] = {false, false};   // the launch uploaded its input (not one fed from a resident stream)
    double prof_ms = 0, h2d_ms = 0, d2h_ms = 0;   // the kernel (scope bgzf_deflate), the two copies
    int64_t prof_n = 0, h2d_n = 0;
    uint32_t (*crc_ld)(uint32_t, const void*, size_t) = nullptr;       // libdeflate_crc32
    unsigned long (*crc_z)(unsigned long, const uint8_t*, unsigned) = nullptr;   // zlib's crc32
    uint32_t crc(const uint8_t* p, size_t n) const {
        if (crc_ld) return crc_ld(0, p, n);
        if (crc_z) return (uint32_t)crc_z(0, p, (unsigned)n);
        return bg_crc_table(0, p, n);
    }
};

namespace {

#define BGCHK(x)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            E->err = std::string("HIP error ") + hipGetErrorString(e_) + " at " #x;          \
            E->broken = true;   /* nothing more is started on the device by this encoder */  \
            return CC_E_HIP;                                                                 \
        }                                                                                    \
    } while (0)

// the two streams the encoder and the inflater share (no others are opened)
int bgzf_streams(BgzfEnc* E) {
    if (E->streams) return 0;
    for (int b = 0; b < 2; ++b) BGCHK(hipStreamCreateWithFlags(&E->st[b], hipStreamNonBlocking));
    E->streams = true;
    return 0;
}

void bgzf_dec_free(BgzfDec* D);

int bgzf_init(BgzfEnc* E) {
    constexpr size_t in_bytes = (size_t)BG_CHUNK * BG_PIECE, out_bytes = (size_t)BG_CHUNK * BG_OSLOT;
    RC(bgzf_streams(E));
    for (int b = 0; b < 2; ++b) {
        BGCHK(hipHostMalloc((void**)&E->h_in[b], in_bytes));
        BGCHK(hipHostMalloc((void**)&E->h_out[b], out_bytes));
        BGCHK(hipHostMalloc((void**)&E->h_len[b], BG_CHUNK * sizeof(uint32_t)));
        BGCHK(hipMalloc((void**)&E->d_in[b], in_bytes));
        BGCHK(hipMalloc((void**)&E->d_out[b], out_bytes));
        BGCHK(hipMalloc((void**)&E->d_pack[b], out_bytes));
        BGCHK(hipMalloc((void**)&E->d_tok[b], in_bytes * sizeof(uint32_t)));
        BGCHK(hipMalloc((void**)&E->d_len[b], BG_CHUNK * sizeof(uint32_t)));
        for (int k = 0; k < 6; ++k) BGCHK(hipEventCreate(&E->ev[b][k]));
    }
    if (void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL))
        E->crc_ld = (uint32_t (*)(uint32_t, const void*, size_t))dlsym(h, "libdeflate_crc32");
    if (!E->crc_ld)
        if (void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL))
            E->crc_z = (unsigned long (*)(unsigned long, const uint8_t*, unsigned))dlsym(h, "crc32");
    E->ready = true;
    return 0;
}

void bgzf_free(cc_ctx* ctx) {
    BgzfEnc* E = ctx->bgzf;
    if (!E) return;
    for (int b = 0; b < 2; ++b)
        if (E->st[b]) (void)hipStreamSynchronize(E->st[b]);
    bgzf_dec_free(E->dec);
    crc_bufs_free(&E->cb);
    for (int b = 0; b < 2; ++b) {
        if (E->h_in[b]) (void)hipHostFree(E->h_in[b]);
        if (E->h_out[b]) (void)hipHostFree(E->h_out[b]);
        if (E->h_len[b]) (void)hipHostFree(E->h_len[b]);
        if (E->d_in[b]) (void)hipFree(E->d_in[b]);
        if (E->d_out[b]) (void)hipFree(E->d_out[b]);
        if (E->d_pack[b]) (void)hipFree(E->d_pack[b]);
        if (E->d_tok[b]) (void)hipFree(E->d_tok[b]);
        if (E->d_len[b]) (void)hipFree(E->d_len[b]);
        for (int k = 0; k < 6; ++k)
            if (E->ev[b][k]) (void)hipEventDestroy(E->ev[b][k]);
        if (E->st[b]) (void)hipStreamDestroy(E->st[b]);
    }
    delete E;
    ctx->bgzf = nullptr;
}

BgzfEnc* bgzf_get(cc_ctx* ctx) {
    std::lock_guard<std::mutex> lk(ctx->bgzf_mu);
    if (!ctx->bgzf) ctx->bgzf = new BgzfEnc();
    return ctx->bgzf;
}

// the encoder's kernel time so far (or its reset); the pointer is read under the mutex that guards
// its creation by a writer thread
void bgzf_prof(cc_ctx* ctx, bool reset, double* ms, int64_t* n, double* h2d = nullptr, double* d2h = nullptr,
               int64_t* h2d_n = nullptr) {
    BgzfEnc* E;
    {
        std::lock_guard<std::mutex> lk(ctx->bgzf_mu);
        E = ctx->bgzf;
    }
    if (!E) return;
    std::lock_guard<std::mutex> lk(E->mu);
    if (reset) { E->prof_ms = E->h2d_ms = E->d2h_ms = 0; E->prof_n = E->h2d_n = 0; }
    if (h2d) *h2d = E->h2d_ms;
    if (h2d_n) *h2d_n = E->h2d_n;
    if (d2h) *d2h = E->d2h_ms;
    if (ms) *ms = E->prof_ms;
    if (n) *n = E->prof_n;
}

// k_crc32's time so far on the coders' streams (or its reset)
void bgzf_crc_prof(cc_ctx* ctx, bool reset, double* ms, int64_t* n) {
    BgzfEnc* E;
    {
        std::lock_guard<std::mutex> lk(ctx->bgzf_mu);
        E = ctx->bgzf;
    }
    if (!E) return;
    std::lock_guard<std::mutex> lk(E->mu);
    if (reset) { E->crc_ms = 0; E->crc_n = 0; }
    if (ms) *ms = E->crc_ms;
    if (n) *n = E->crc_n;
}

// k_index_fields' time so far (or its reset)
void bgzf_idx_prof(cc_ctx* ctx, bool reset, double* ms, int64_t* n, double* put_ms = nullptr, int64_t* put_n = nullptr) {
    BgzfEnc* E;
    {
        std::lock_guard<std::mutex> lk(ctx->bgzf_mu);
        E = ctx->bgzf;
    }
    if (!E) return;
    std::lock_guard<std::mutex> lk(E->mu);
    if (reset) { E->idx_ms = E->put_ms = 0; E->idx_n = E->put_n = 0; }
    if (put_ms) *put_ms = E->put_ms;
    if (put_n) *put_n = E->put_n;
    if (ms) *ms = E->idx_ms;
    if (n) *n = E->idx_n;
}

// a finished, timed k_crc32 launch of set B's stream b added to the scope
int crc_prof_add(BgzfEnc* E, CrcBufs* B, int b) {
    if (!B->timed[b]) return 0;
    float ms = 0;
    BGCHK(hipEventElapsedTime(&ms, B->ev[b][0], B->ev[b][1]));
    E->crc_ms += ms;
    E->crc_n += 1;
    B->timed[b] = false;
    return 0;
}

// cc_bgzf_deflate's work.  Launches of BG_CHUNK pieces alternate between two streams, each with
// its own pinned and device buffers: while one launch encodes, the previous one's members are
// downloaded and framed and the next one's input is staged; the CRCs are computed meanwhile, by the
// calling thread or (crc_on) by k_crc32 over the launch's input buffer, behind its encoder kernels.
// With dev (cc_bgzf_deflate_resident: n bytes of a resident stream at a 256-byte multiple of it, data
// null) the kernels read their pieces where they lie: nothing is staged or uploaded, and the CRCs are
// always k_crc32's.
int64_t bgzf_encode(cc_ctx* ctx, BgzfEnc* E, const uint8_t* data, uint64_t n, uint8_t* stage, uint64_t slot,
                    uint32_t* out_len, int64_t cap, const uint8_t* dev = nullptr) {
    const int64_t np = (int64_t)((n + BG_PIECE - 1) / BG_PIECE);
    if (np == 0) return 0;
    if ((!data && !dev) || !stage || !out_len || slot < 0x10000 || np > cap) {
        E->err = "cc_bgzf_deflate: null argument, slot under 65536 or more pieces than cap";
        return CC_E_INVALID;
    }
    if (E->broken) return CC_E_HIP;
    BGCHK(hipSetDevice(ctx->device));   // (not enter(): a writer's thread, the switches are the engine thread's)
    if (!E->ready) RC(bgzf_init(E));
    const bool prof = ctx->profiling;
    const bool dev_crc = E->crc_on || dev;   // the whole round one way
    if (dev_crc) BGCHK(crc_bufs_init(&E->cb, BG_CHUNK));
    const auto kernel = E->effort == 2 ? k_bgzf_deflate<2> : k_bgzf_deflate<1>;   // the whole round at one effort
    const int64_t nchunks = (np + BG_CHUNK - 1) / BG_CHUNK;
    std::vector<uint32_t> crcs(dev_crc ? 0 : (size_t)np);
    auto pieces_of = [&](int64_t k) { return (int)std::min<int64_t>(BG_CHUNK, np - k * BG_CHUNK); };
    auto launch = [&](int64_t k) -> int {
        const int b = (int)(k & 1), pc = pieces_of(k);
        const uint64_t o = (uint64_t)k * BG_CHUNK * BG_PIECE, bytes = std::min<uint64_t>(n - o, (uint64_t)pc * BG_PIECE);
        const uint8_t* in = dev ? dev + o : E->d_in[b];
        if (!dev) {
            memcpy(E->h_in[b], data + o, bytes);
            if (prof) BGCHK(hipEventRecord(E->ev[b][2], E->st[b]));
            BGCHK(hipMemcpyAsync(E->d_in[b], E->h_in[b], bytes, hipMemcpyHostToDevice, E->st[b]));
            if (prof) BGCHK(hipEventRecord(E->ev[b][3], E->st[b]));
        }
        E->timed[b] = prof;
        E->up_timed[b] = prof && !dev;
        if (prof) BGCHK(hipEventRecord(E->ev[b][0], E->st[b]));
        klaunch(E->st[b], kernel, (unsigned)pc, BG_T, in, (uint64_t)bytes, E->d_tok[b], E->d_out[b], E->d_len[b]);
        if (prof) BGCHK(hipEventRecord(E->ev[b][1], E->st[b]));
        klaunch(E->st[b], k_bgzf_pack, (unsigned)pc, 256, E->d_out[b], E->d_len[b], E->d_pack[b]);
        BGCHK(hipGetLastError());
        BGCHK(hipMemcpyAsync(E->h_len[b], E->d_len[b], (size_t)pc * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st[b]));
        if (dev_crc) {
            E->cb.timed[b] = prof;
            BGCHK(crc_launch(E->st[b], prof ? E->cb.ev[b] : nullptr, in, nullptr, CR_PIECE, bytes, E->cb.d[b], pc));
            BGCHK(hipMemcpyAsync(E->cb.h[b], E->cb.d[b], (size_t)pc * sizeof(uint32_t), hipMemcpyDeviceToHost, E->st[b]));
        }
        return 0;
    };
    auto finish = [&](int64_t k) -> int {
        const int b = (int)(k & 1), pc = pieces_of(k);
        BGCHK(hipStreamSynchronize(E->st[b]));
        if (E->timed[b]) {
            float ms = 0;
            BGCHK(hipEventElapsedTime(&ms, E->ev[b][0], E->ev[b][1]));
            E->prof_ms += ms;
            E->prof_n += 1;
        }
        if (E->up_timed[b]) {
            float ms = 0;
            BGCHK(hipEventElapsedTime(&ms, E->ev[b][2], E->ev[b][3]));
            E->h2d_ms += ms;
            E->h2d_n += 1;
        }
        if (dev_crc) RC(crc_prof_add(E, &E->cb, b));
        uint64_t words = 0;
        for (int j = 0; j < pc; ++j) {
            const uint32_t ln = E->h_len[b][j];
            if (ln < 28 || ln > 0x10000) {
                E->err = "cc_bgzf_deflate: a member's size is out of range";
                E->broken = true;   // the kernel miscounted: this encoder is not used again
                return CC_E_INVALID;
            }
            words += (ln + 3) >> 2;
        }
        if (E->timed[b]) BGCHK(hipEventRecord(E->ev[b][4], E->st[b]));
        BGCHK(hipMemcpyAsync(E->h_out[b], E->d_pack[b], words * 4, hipMemcpyDeviceToHost, E->st[b]));
        if (E->timed[b]) BGCHK(hipEventRecord(E->ev[b][5], E->st[b]));
        BGCHK(hipStreamSynchronize(E->st[b]));
        if (E->timed[b]) {
            float ms = 0;
            BGCHK(hipEventElapsedTime(&ms, E->ev[b][4], E->ev[b][5]));
            E->d2h_ms += ms;
        }
        uint64_t w = 0;
        for (int j = 0; j < pc; ++j) {
            const int64_t p = k * BG_CHUNK + j;
            const uint32_t ln = E->h_len[b][j], crc = dev_crc ? E->cb.h[b][j] : crcs[(size_t)p];
            uint8_t* m = stage + (uint64_t)p * slot;
            memcpy(m, E->h_out[b] + 4 * w, ln);
            for (int q = 0; q < 4; ++q) m[ln - 8 + q] = (uint8_t)(crc >> (8 * q));
            out_len[p] = ln;
            w += (ln + 3) >> 2;
        }
        return 0;
    };
    // on any failure both streams are drained before the buffers can be touched again
    auto drained = [&](int rc) {
        if (rc)
            for (int b = 0; b < 2; ++b) (void)hipStreamSynchronize(E->st[b]);
        return rc;
    };
#define BGRC(x) do { int rc_ = drained(x); if (rc_) return rc_; } while (0)
    for (int64_t k = 0; k < nchunks; ++k) {
        BGRC(launch(k));
        const int64_t p0 = k * BG_CHUNK;
        for (int j = 0; !dev_crc && j < pieces_of(k); ++j) {
            const uint64_t o = (uint64_t)(p0 + j) * BG_PIECE;
            crcs[(size_t)(p0 + j)] = E->crc(data + o, (size_t)std::min<uint64_t>(BG_PIECE, n - o));
        }
        if (k >= 1) BGRC(finish(k - 1));
    }
    BGRC(finish(nchunks - 1));
#undef BGRC
    return np;
}

// ccio_deflate_fn over a context: any failure is a nonzero return (the writers then use the host encoder)
int bgzf_hook_fn(void* user, const uint8_t* data, uint64_t n, uint8_t* stage, uint64_t slot, uint32_t* out_len,
                 int64_t pieces) {
    cc_ctx* ctx = (cc_ctx*)user;
    if (!ctx) return 1;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    return bgzf_encode(ctx, E, data, n, stage, slot, out_len, pieces) == pieces ? 0 : 1;
}

}  // namespace

extern "C" {

int64_t cc_bgzf_deflate(cc_ctx* ctx, const uint8_t* data, uint64_t n, uint8_t* stage, uint64_t slot, uint32_t* out_len,
                        int64_t cap) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);
    const int64_t r = bgzf_encode(ctx, E, data, n, stage, slot, out_len, cap);
    if (r < 0) ctx->err = E->err;
    return r;
}

int cc_bgzf_set_effort(cc_ctx* ctx, int effort) {
    if (!ctx) return CC_E_INVALID;
    if (effort != 1 && effort != 2) {
        ctx->err = "cc_bgzf_set_effort: the effort is 1 or 2";
        return CC_E_INVALID;
    }
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);   // a running round holds it: it finishes at its own effort
    E->effort = effort;
    return 0;
}

int cc_bgzf_set_crc(cc_ctx* ctx, int on) {
    if (!ctx) return CC_E_INVALID;
    BgzfEnc* E = bgzf_get(ctx);
    std::lock_guard<std::mutex> lk(E->mu);   // a running round holds it: it finishes the way it began
    E->crc_on = on != 0;
    return 0;
}

int cc_bgzf_hook(cc_ctx* ctx, ccio_deflate_fn* fn, void** user) {
    if (!ctx || !fn || !user) return CC_E_INVALID;
    *fn = bgzf_hook_fn;
    *user = ctx;
    return 0;
}

}  // extern "C"
