// The per-record parts of the output BAM assembler: ccio_write_bam_ex's three record kinds restated
// over cc_out_spec.  Plain C++ that compiles in the HIP kernels (bam_assemble.hip.inc: k_asm_sizes,
// k_asm_copy) and with a host compiler alone (assemble_host below; tests/asan/assemble_core_driver.cpp
// runs it under sanitizers against ccio_write_bam_ex), so both execute the same text.
//
// The contract (a bad spec must never fault a device other people share):
//   * layout() reads a spec's template record, name and RG offsets only after the indices that lead
//     to them were checked against their tables, and refuses (error bits, nothing of the layout is
//     meaningful) whatever does not fit: it is the only function that may run on unchecked specs;
//   * out16() reads only bytes layout() accepted, through F::fetch(base, a, valid) with
//     [a, a + valid) inside the accepted range, and gives the 16 bytes at any offset of the output
//     record, bytes from `valid` on zero.
#ifndef CC_ASSEMBLE_CORE_H
#define CC_ASSEMBLE_CORE_H

#include "unpack_core.h"

#if defined(__HIPCC__)
#define ASM_HD __host__ __device__ inline
#else
#define ASM_HD inline
#include <algorithm>
#include <utility>
#include <vector>
#endif

namespace asmb {

using upk::W16;

// cc_out_spec (include/consensuscruncher_amd.h), field for field
struct Spec {
    int32_t kind, src_file;
    int64_t src_rec, name_id;
    int32_t flag, mapq, tlen, rg_id;
    int64_t cons_off;
    int32_t cons_len, pad;
};
static_assert(sizeof(Spec) == 56, "cc_out_spec layout");
enum : int32_t { OUT_RAW = 0, OUT_RENAME = 1, OUT_NEW = 2 };

// refusals (the first bad spec's bits are reported)
enum : uint32_t {
    AE_KIND = 1u,       // a kind other than 0, 1, 2
    AE_SRC = 2u,        // src_file or src_rec out of range, or the record's offset outside its stream
    AE_TMPL = 4u,       // a template whose block_size, l_read_name, n_cigar and l_seq do not fit
    AE_NAME = 8u,       // name_id out of range, or its offsets outside the blob or out of order
    AE_LONGNAME = 16u,  // a new name longer than 254 bytes (l_read_name is one byte)
    AE_CONS = 32u,      // cons_off / cons_len, or the nibble range, outside the consensus arrays
    AE_RG = 64u,        // rg_id outside the RG table, or its offsets outside the blob
};

// one source: the records are base[shift + rec_off[i] ...), all inside base[shift, shift + bytes)
struct Src {
    const uint8_t* base;
    uint64_t shift, bytes;
    const uint64_t* rec_off;
    int64_t nrec;
};
struct Tables {
    const Src* src;
    int32_t nsrc, n_rg;
    const uint8_t* names;       // n_names names side by side: name i is names[name_off[i], name_off[i + 1])
    const int64_t* name_off;
    int64_t n_names;
    uint64_t names_bytes;
    const uint8_t* cons_seq;    // CC_OUT_NEW: nibbles at cons_seq + cons_off / 2, qualities at cons_qual + cons_off
    const uint8_t* cons_qual;
    uint64_t cons_seq_bytes, cons_qual_bytes;
    const uint8_t* rg;          // RG value i is rg[rg_off[i], rg_off[i + 1])
    const int64_t* rg_off;
    uint64_t rg_bytes;
};

// an accepted spec's output record
struct Lay {
    uint32_t size;       // block_size word included
    int32_t kind;
    const uint8_t* sbase;
    uint64_t rec;        // the template's block_size word is sbase[rec]
    uint32_t bs, lqn, ncig, nl, L, rgl;
    uint64_t name_at, seq_at, qual_at, rg_at;
    bool has_rg;
    uint32_t h[9];       // kinds 1, 2: the new block_size word and the 32 core bytes
};

ASM_HD int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// The spec checked and laid out; *key is its samtools-sort key, tid << 32 | (pos + 1) << 1 | reverse
// (tid unsigned: -1 sorts last; the reverse bit is the spec's flag for CC_OUT_NEW, else the
// template's).  Returns the refusal bits, 0 when y and *key are valid.
ASM_HD uint32_t layout(const Spec& sp, const Tables& T, Lay& y, uint64_t* key) {
    if (sp.kind != OUT_RAW && sp.kind != OUT_RENAME && sp.kind != OUT_NEW) return AE_KIND;
    if (sp.src_file < 0 || sp.src_file >= T.nsrc) return AE_SRC;
    const Src& s = T.src[sp.src_file];
    if (sp.src_rec < 0 || sp.src_rec >= s.nrec) return AE_SRC;
    const uint64_t rel = s.rec_off[sp.src_rec];
    if (rel >= s.bytes) return AE_SRC;
    upk::Rec f;
    const uint8_t* rec = s.base + s.shift + rel;
    if (!upk::parse(rec, s.bytes - rel, f)) return AE_TMPL;
    y.kind = sp.kind;
    y.sbase = s.base;
    y.rec = s.shift + rel;
    y.bs = (uint32_t)f.bs;
    y.lqn = (uint32_t)f.l_read_name;
    y.ncig = (uint32_t)f.n_cigar;
    y.nl = y.L = y.rgl = 0;
    y.name_at = y.seq_at = y.qual_at = y.rg_at = 0;
    y.has_rg = false;
    const uint32_t fl = sp.kind == OUT_NEW ? (uint32_t)(uint16_t)sp.flag : (uint32_t)f.flag;
    *key = ((uint64_t)(uint32_t)f.tid << 32) | ((uint64_t)(uint32_t)(f.pos + 1) << 1) | ((fl >> 4) & 1u);
    if (sp.kind == OUT_RAW) {
        y.size = 4u + y.bs;
        return 0;
    }
    if (sp.name_id >= 0) {
        if (sp.name_id >= T.n_names) return AE_NAME;
        const int64_t a = T.name_off[sp.name_id], b = T.name_off[sp.name_id + 1];
        if (a < 0 || b < a || (uint64_t)b > T.names_bytes) return AE_NAME;
        if (b - a > 254) return AE_LONGNAME;
        y.nl = (uint32_t)(b - a);
        y.name_at = (uint64_t)a;
    }
    y.h[3] = (y.nl + 1u);
    if (sp.kind == OUT_RENAME) {
        y.size = 4u + 32u + y.nl + 1u + (y.bs - 32u - y.lqn);
        y.h[0] = y.size - 4u;
        y.h[1] = (uint32_t)f.tid;
        y.h[2] = (uint32_t)f.pos;
        y.h[3] |= upk::ld32(rec + 12) & 0xffffff00u;   // mapq and bin stay the template's
        y.h[4] = upk::ld32(rec + 16);
        y.h[5] = (uint32_t)f.lseq;
        y.h[6] = (uint32_t)f.mtid;
        y.h[7] = (uint32_t)f.mpos;
        y.h[8] = (uint32_t)f.tlen;
        return 0;
    }
    // CC_OUT_NEW: create_aligned_segment
    if (sp.cons_len < 0 || sp.cons_off < 0) return AE_CONS;
    y.L = (uint32_t)sp.cons_len;
    y.qual_at = (uint64_t)sp.cons_off;
    y.seq_at = (uint64_t)sp.cons_off / 2;
    if (y.qual_at + y.L > T.cons_qual_bytes || y.seq_at + (y.L + 1u) / 2u > T.cons_seq_bytes) return AE_CONS;
    if (sp.rg_id >= 0) {
        if (sp.rg_id >= T.n_rg) return AE_RG;
        const int64_t a = T.rg_off[sp.rg_id], b = T.rg_off[sp.rg_id + 1];
        if (a < 0 || b < a || (uint64_t)b > T.rg_bytes || b - a > 0xffffff) return AE_RG;
        y.has_rg = true;
        y.rgl = (uint32_t)(b - a);
        y.rg_at = (uint64_t)a;
    }
    int64_t rlen = 0;
    for (uint32_t c = 0; c < y.ncig; ++c) {
        const uint32_t v = upk::ld32(rec + f.cig_off + 4u * c), op = v & 0xf;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += v >> 4;
    }
    const int64_t pos = f.pos;
    const int bin = reg2bin(pos < 0 ? 0 : pos, pos < 0 ? 1 : pos + (rlen ? rlen : 1));
    const uint64_t size = 4ull + 32 + y.nl + 1 + 4ull * y.ncig + (y.L + 1u) / 2u + (uint64_t)y.L + (y.has_rg ? 3ull + y.rgl + 1 : 0);
    if (size > 0xffffffffull) return AE_CONS;
    y.size = (uint32_t)size;
    y.h[0] = y.size - 4u;
    y.h[1] = (uint32_t)f.tid;
    y.h[2] = (uint32_t)f.pos;
    y.h[3] |= ((uint32_t)(uint8_t)sp.mapq << 8) | ((uint32_t)(uint16_t)bin << 16);
    y.h[4] = y.ncig | ((uint32_t)(uint16_t)sp.flag << 16);
    y.h[5] = y.L;
    y.h[6] = (uint32_t)f.mtid;
    y.h[7] = (uint32_t)f.mpos;
    y.h[8] = (uint32_t)sp.tlen;
    return 0;
}

// w's bytes moved k (0..15) places up: byte i becomes byte i + k, the low k bytes zero
ASM_HD W16 shl_bytes(const W16& w, uint32_t k) {
    uint64_t lo = (uint64_t)w.w[0] | ((uint64_t)w.w[1] << 32), hi = (uint64_t)w.w[2] | ((uint64_t)w.w[3] << 32);
    if (k & 8u) { hi = lo; lo = 0; }
    const uint32_t b = (k & 7u) * 8u;
    if (b) {
        hi = (hi << b) | (lo >> (64u - b));
        lo <<= b;
    }
    return W16{{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)}};
}
ASM_HD W16 keep_bytes(W16 w, uint32_t valid) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        const int32_t nb = (int32_t)valid - 4 * i;
        w.w[i] = nb >= 4 ? w.w[i] : (nb <= 0 ? 0u : (w.w[i] & ((1u << (8 * nb)) - 1u)));
    }
    return w;
}
// word k (0..8) of the head, without indexing it by a variable (the array stays in registers)
ASM_HD uint32_t head_word(const Lay& y, uint32_t k) {
    uint32_t r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 9; ++i) r = k == i ? y.h[i] : r;
    return r;
}
// `valid` (1..16) bytes of the 36-byte head from byte a on
ASM_HD W16 head16(const Lay& y, uint32_t a, uint32_t valid) {
    const uint32_t q = a >> 2, sh = (a & 3u) * 8u;
    W16 o;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t x0 = head_word(y, q + i), x1 = head_word(y, q + i + 1);   // (past word 8: zero)
        o.w[i] = sh ? ((x0 >> sh) | (x1 << (32u - sh))) : x0;
    }
    return keep_bytes(o, valid);
}

// The 16 bytes at offset j of the output record y, bytes from `valid` (1..16, j + valid <= y.size)
// on zero.  F::fetch(base, a, valid): the bytes base[a, a + valid), zero from `valid` on.
template <class F>
ASM_HD W16 out16(const Lay& y, const Tables& T, uint32_t j, uint32_t valid) {
    if (y.kind == OUT_RAW) return F::fetch(y.sbase, y.rec + j, valid);
    W16 o{{0u, 0u, 0u, 0u}};
    const uint64_t e = (uint64_t)j + valid;
    auto put = [&](const W16& w, uint32_t at) {
        const W16 s = shl_bytes(w, at);
        o.w[0] |= s.w[0]; o.w[1] |= s.w[1]; o.w[2] |= s.w[2]; o.w[3] |= s.w[3];
    };
    // the part of [j, e) inside the piece [beg, beg + len), taken from base[a ...)
    auto mem = [&](uint64_t beg, uint64_t len, const uint8_t* base, uint64_t a) {
        const uint64_t lo = j > beg ? j : beg, hi = e < beg + len ? e : beg + len;
        if (lo < hi) put(F::fetch(base, a + (lo - beg), (uint32_t)(hi - lo)), (uint32_t)(lo - j));
    };
    if (j < 36u) {
        const uint32_t hi = e < 36u ? (uint32_t)e : 36u;
        put(head16(y, j, hi - j), 0u);
    }
    mem(36u, y.nl, T.names, y.name_at);
    uint64_t p = 37ull + y.nl;   // (the name's NUL is a zero byte: nothing to add)
    if (y.kind == OUT_RENAME) {
        mem(p, (uint64_t)y.bs - 32u - y.lqn, y.sbase, y.rec + 36u + y.lqn);
        return o;
    }
    mem(p, 4ull * y.ncig, y.sbase, y.rec + 36u + y.lqn);
    p += 4ull * y.ncig;
    mem(p, (y.L + 1u) / 2u, T.cons_seq, y.seq_at);
    p += (y.L + 1u) / 2u;
    mem(p, y.L, T.cons_qual, y.qual_at);
    p += y.L;
    if (y.has_rg) {
        const uint64_t lo = j > p ? j : p, hi = e < p + 3 ? e : p + 3;
        if (lo < hi) {
            const uint32_t rgz = 0x5a4752u >> (8u * (uint32_t)(lo - p));   // "RGZ"
            put(keep_bytes(W16{{rgz, 0u, 0u, 0u}}, (uint32_t)(hi - lo)), (uint32_t)(lo - j));
        }
        mem(p + 3, y.rgl, T.rg, y.rg_at);
    }
    return o;
}

// the plain byte-at-a-time fetch (host code, and what the device's aligned loads must agree with)
struct ByteFetch {
    static ASM_HD W16 fetch(const uint8_t* base, uint64_t a, uint32_t valid) {
        W16 o{{0u, 0u, 0u, 0u}};
        for (uint32_t k = 0; k < valid; ++k) o.w[k >> 2] |= (uint32_t)base[a + k] << (8 * (k & 3));
        return o;
    }
};

// the number of whole digits [begin, end) of an 8-bit LSD sort that orders keys whose OR is `bits`
ASM_HD void key_digits(uint64_t bits, unsigned* begin, unsigned* end) {
    unsigned lo = 0, hi = 64;
    if (!bits) { *begin = *end = 0; return; }
    while (!((bits >> lo) & 1ull)) ++lo;
    while (!((bits >> (hi - 1)) & 1ull)) --hi;
    lo &= ~7u;
    *begin = lo;
    *end = hi;
}

// records per offset slice: a slice's sizes sum to at most `bound` (the scans' totals are 32-bit)
ASM_HD int64_t slice_records(uint64_t bound, uint32_t largest) {
    const uint64_t k = bound / (largest ? largest : 1u);
    return (int64_t)(k ? k : 1);
}

#if !defined(__HIPCC__)
// The whole assembly on the host, as the device runs it: the sizes pass, the stable sort, the
// offsets, then every record chunk by chunk.  header_bytes + records into out (resized) and
// at[n + 1].  Returns -1 when every spec was accepted, else the first refused spec (*err its bits).
inline int64_t assemble_host(const uint8_t* header, uint64_t header_bytes, const Spec* spec, int64_t n, const Tables& T,
                             bool sorted, std::vector<uint8_t>& out, std::vector<uint64_t>& at, uint32_t* err) {
    std::vector<Lay> lay((size_t)n);
    std::vector<std::pair<uint64_t, int64_t>> k((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        uint64_t key = 0;
        const uint32_t e = layout(spec[i], T, lay[(size_t)i], &key);
        if (e) { *err = e; return i; }
        k[(size_t)i] = {key, i};
    }
    if (sorted)
        std::stable_sort(k.begin(), k.end(), [](const std::pair<uint64_t, int64_t>& a, const std::pair<uint64_t, int64_t>& b) {
            return a.first < b.first;
        });
    at.assign((size_t)n + 1, 0);
    at[0] = header_bytes;
    for (int64_t o = 0; o < n; ++o) at[(size_t)o + 1] = at[(size_t)o] + lay[(size_t)k[(size_t)o].second].size;
    out.assign((size_t)at[(size_t)n], 0xee);
    for (uint64_t b = 0; b < header_bytes; ++b) out[(size_t)b] = header[b];
    for (int64_t o = 0; o < n; ++o) {
        const Lay& y = lay[(size_t)k[(size_t)o].second];
        uint8_t* d = out.data() + at[(size_t)o];
        // as the copy kernel cuts it: a head up to the output's next 16-byte line, then whole lines
        uint32_t v = (16u - (uint32_t)(at[(size_t)o] & 15u)) & 15u;
        for (uint32_t j = 0; j < y.size; j += v, v = 16u) {
            v = v ? v : 16u;
            v = y.size - j < v ? y.size - j : v;
            const W16 w = out16<ByteFetch>(y, T, j, v);
            for (uint32_t b = 0; b < v; ++b) d[j + b] = (uint8_t)(w.w[b >> 2] >> (8 * (b & 3)));
        }
    }
    *err = 0;
    return -1;
}
#endif

}  // namespace asmb

#endif
