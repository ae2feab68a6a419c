// The per-name parts of the consensus read-name formatter: ccio_format_csn_names' rule (sscs_qname +
// ':' + suffix, from packed fields and the interned barcode / cigar strings) and
// ccio_format_dcs_names' rule (dcs_consensus_tag on two SSCS qnames of the record table) restated so
// that a name's length and the 16 bytes at any offset of it can be computed on their own.  Plain C++
// that compiles in the HIP kernels (name_format.hip.inc: k_name_sizes_*, k_name_write_*) and with a
// host compiler alone (csn_host / dcs_host below; tests/asan/name_core_driver.cpp runs them under
// sanitizers against the two libccio functions), so both execute the same text.
//
// The contract (a bad field must never fault a device other people share):
//   * csn_layout() reads a string's offsets only after its id was checked against its table, and
//     refuses whatever does not fit; dcs_layout() reads a name only through F::word(base, a, valid)
//     with a 8-byte aligned and [a, a + valid) inside the name: they are the only functions that may
//     run on unchecked input (the record indices of a dcs pair are the caller's to check);
//   * csn_out16() / dcs_out16() read only bytes the layout accepted, through F::fetch(base, a, valid)
//     with [a, a + valid) inside the accepted range, and give the 16 bytes at any offset of the name,
//     bytes from `valid` on zero.
#ifndef CC_NAME_CORE_H
#define CC_NAME_CORE_H

#include "assemble_core.h"

#if defined(__HIPCC__)
#define NMC_HD __host__ __device__ __forceinline__
#define NMC_UNROLL _Pragma("unroll")
#else
#define NMC_HD inline
#define NMC_UNROLL
#include <vector>
#endif

// a lambda that must be part of its caller (a layout captured by reference then stays in registers)
#define NMC_INL __attribute__((always_inline))

namespace nmc {

using upk::W16;

// refusals (the first refused name's bits are reported)
enum : uint32_t {
    NE_BC = 1u,          // csn: f0 outside the barcode table
    NE_CG5 = 2u,         // csn: f5 outside the cigar table
    NE_CG6 = 4u,         // csn: f6 outside the cigar table
    NE_STR = 8u,         // csn: a string's offsets outside its blob, out of order, or 2^30 bytes or more
    NE_T_NOUS = 16u,     // dcs: no '_' in the tag name
    NE_T_NOCOLON = 32u,  // dcs: no ':' in the tag name
    NE_D_NOCOLON = 64u,  // dcs: no ':' in the partner name
    NE_REC = 128u,       // dcs: a record index outside the table, or its qname slot outside the blob
};

// ---- decimals ---------------------------------------------------------------------------------
NMC_HD uint32_t digits32(uint32_t u) {
    uint32_t d = 1;
    while (u >= 10u) { u /= 10u; ++d; }
    return d;
}
NMC_HD uint32_t digits64(uint64_t u) {
    uint32_t d = 0;
    while (u > 0xffffffffull) { u /= 10u; ++d; }
    return d + digits32((uint32_t)u);
}
// a number as its text is produced: magnitude, sign, and the text's length (sign included)
struct Dec {
    uint64_t u;
    uint32_t neg, len;
};
NMC_HD Dec dec_i32(int32_t v) {
    const uint32_t neg = v < 0;
    const uint32_t u = neg ? 0u - (uint32_t)v : (uint32_t)v;   // (INT32_MIN: 2^31)
    return Dec{u, neg, neg + digits32(u)};
}
NMC_HD Dec dec_u32(uint32_t v) { return Dec{v, 0u, digits32(v)}; }
NMC_HD Dec dec_i64(int64_t v) {
    const uint32_t neg = v < 0;
    const uint64_t u = neg ? 0ull - (uint64_t)v : (uint64_t)v;   // (INT64_MIN: 2^63)
    return Dec{u, neg, neg + digits64(u)};
}
// character k (< d.len) of the text
NMC_HD uint32_t dec_char(const Dec& d, uint32_t k) {
    if (d.neg && k == 0) return '-';
    uint32_t r = d.len - 1u - k;   // the digits to its right
    uint64_t u = d.u;
    while (u > 0xffffffffull && r) { u /= 10u; --r; }
    if (u > 0xffffffffull) return '0' + (uint32_t)(u % 10u);
    uint32_t w = (uint32_t)u;
    for (; r; --r) w /= 10u;
    return '0' + w % 10u;
}

// ---- assembling 16 output bytes ------------------------------------------------------------------
// byte q (0..15) of o set to c, without indexing the words by a variable (they stay in registers)
NMC_HD void put_byte(W16& o, uint32_t q, uint32_t c) {
    const uint32_t v = c << (8u * (q & 3u));
    NMC_UNROLL
    for (uint32_t i = 0; i < 4; ++i) o.w[i] |= (q >> 2) == i ? v : 0u;
}
NMC_HD void put_w16(W16& o, const W16& w, uint32_t at) {
    const W16 s = asmb::shl_bytes(w, at);
    o.w[0] |= s.w[0]; o.w[1] |= s.w[1]; o.w[2] |= s.w[2]; o.w[3] |= s.w[3];
}
// the window [j, e) of a name being produced into o
struct Win {
    W16 o;
    uint32_t j, e;
    // the part of the window inside the piece [beg, beg + len), copied from base[a ...)
    template <class F>
    NMC_HD void mem(uint32_t beg, uint32_t len, const uint8_t* base, uint64_t a) {
        const uint32_t lo = j > beg ? j : beg, hi = e < beg + len ? e : beg + len;
        if (lo < hi) put_w16(o, F::fetch(base, a + (lo - beg), hi - lo), lo - j);
    }
    // ... and inside a piece whose byte k is fn(k)
    template <class Fn>
    NMC_HD void gen(uint32_t beg, uint32_t len, Fn fn) {
        const uint32_t lo = j > beg ? j : beg, hi = e < beg + len ? e : beg + len;
        for (uint32_t p = lo; p < hi; ++p) put_byte(o, p - j, fn(p - beg));
    }
};

// ---- csn: sscs_qname + ':' + suffix -----------------------------------------------------------------
// a table's strings side by side: string i is blob[off[i], off[i + 1]), all inside blob[0, bytes)
struct Strs {
    const uint8_t* blob;
    const int64_t* off;
    int64_t n;
    uint64_t bytes;
};

// bc[f0] _f1_f2_f3_f4_ cg[f5] _ cg[f6] _strand_u32(f8):suffix
struct CsnLay {
    uint64_t bc_at, c5_at, c6_at;
    uint32_t bc_len, c5_len, c6_len;
    int32_t f1, f2, f3, f4;
    uint32_t l1, l2, l3, l4;   // their texts' lengths (scalars, not arrays: the kernels keep them in registers)
    uint32_t f8, f8l, strand, sl, sufl;
    int64_t suf;
    uint32_t p_g1, p_c5, p_c6, p_g2, len;   // where the pieces begin (the '_' between the cigars is at p_c6 - 1)
};

NMC_HD uint32_t str_at(const Strs& t, int32_t id, uint64_t* at, uint32_t* len) {
    const int64_t a = t.off[id], b = t.off[id + 1];
    if (a < 0 || b < a || (uint64_t)b > t.bytes || b - a >= (1ll << 30)) return NE_STR;
    *at = (uint64_t)a;
    *len = (uint32_t)(b - a);
    return 0;
}

// Name i's fields (f: its nine packed fields) checked and laid out.  Returns the refusal bits, 0 when
// y is valid.
NMC_HD uint32_t csn_layout(const int32_t* f, int64_t suffix, const Strs& bc, const Strs& cg, CsnLay& y) {
    const int32_t f0 = f[0], f5 = f[5], f6 = f[6];
    if (f0 < 0 || f0 >= bc.n) return NE_BC;
    if (f5 < 0 || f5 >= cg.n) return NE_CG5;
    if (f6 < 0 || f6 >= cg.n) return NE_CG6;
    if (str_at(bc, f0, &y.bc_at, &y.bc_len) || str_at(cg, f5, &y.c5_at, &y.c5_len) || str_at(cg, f6, &y.c6_at, &y.c6_len))
        return NE_STR;
    y.f1 = f[1]; y.f2 = f[2]; y.f3 = f[3]; y.f4 = f[4];
    y.l1 = dec_i32(y.f1).len; y.l2 = dec_i32(y.f2).len; y.l3 = dec_i32(y.f3).len; y.l4 = dec_i32(y.f4).len;
    const uint32_t g1 = 5u + y.l1 + y.l2 + y.l3 + y.l4;   // "_f1_f2_f3_f4_"
    const int32_t s = f[7] & 3;
    y.strand = (uint32_t)(s < 2 ? s : 2);
    y.sl = y.strand == 2u ? 4u : 3u;
    y.f8 = (uint32_t)f[8];
    y.f8l = digits32(y.f8);
    y.suf = suffix;
    y.sufl = dec_i64(suffix).len;
    y.p_g1 = y.bc_len;
    y.p_c5 = y.p_g1 + g1;
    y.p_c6 = y.p_c5 + y.c5_len + 1u;
    y.p_g2 = y.p_c6 + y.c6_len;
    y.len = y.p_g2 + 1u + y.sl + 1u + y.f8l + 1u + y.sufl;
    return 0;
}

// byte k of "_f1_f2_f3_f4_"
NMC_HD uint32_t csn_g1(const CsnLay& y, uint32_t k) {
    const uint32_t e1 = 1u + y.l1, e2 = e1 + 1u + y.l2, e3 = e2 + 1u + y.l3, e4 = e3 + 1u + y.l4;   // the fields' ends
    if (k >= e4) return '_';
    const uint32_t beg = k < e1 ? 0u : (k < e2 ? e1 : (k < e3 ? e2 : e3));
    const int32_t v = k < e1 ? y.f1 : (k < e2 ? y.f2 : (k < e3 ? y.f3 : y.f4));
    const uint32_t l = k < e1 ? y.l1 : (k < e2 ? y.l2 : (k < e3 ? y.l3 : y.l4));
    if (k == beg) return '_';
    const uint32_t neg = v < 0;
    return dec_char(Dec{neg ? 0u - (uint32_t)v : (uint32_t)v, neg, l}, k - beg - 1u);
}
// byte k of "_strand_u32(f8):suffix"
NMC_HD uint32_t csn_g2(const CsnLay& y, uint32_t k) {
    if (k == 0) return '_';
    k -= 1u;
    if (k < y.sl) {
        const uint32_t w = y.strand == 0u ? 0x00736f70u : (y.strand == 1u ? 0x0067656eu : 0x656e6f4eu);   // pos neg None
        return (w >> (8u * k)) & 0xffu;
    }
    k -= y.sl;
    if (k == 0) return '_';
    k -= 1u;
    if (k < y.f8l) return dec_char(Dec{y.f8, 0u, y.f8l}, k);
    k -= y.f8l;
    if (k == 0) return ':';
    const uint32_t neg = y.suf < 0;
    return dec_char(Dec{neg ? 0ull - (uint64_t)y.suf : (uint64_t)y.suf, neg, y.sufl}, k - 1u);
}

// The 16 bytes at offset j of the name y, bytes from `valid` (1..16, j + valid <= y.len) on zero.
// F::fetch(base, a, valid): the bytes base[a, a + valid), zero from `valid` on.
template <class F>
NMC_HD W16 csn_out16(const CsnLay& y, const Strs& bc, const Strs& cg, uint32_t j, uint32_t valid) {
    Win w{W16{{0u, 0u, 0u, 0u}}, j, j + valid};
    w.template mem<F>(0u, y.bc_len, bc.blob, y.bc_at);
    w.gen(y.p_g1, y.p_c5 - y.p_g1, [&](uint32_t k) NMC_INL { return csn_g1(y, k); });
    w.template mem<F>(y.p_c5, y.c5_len, cg.blob, y.c5_at);
    w.gen(y.p_c6 - 1u, 1u, [](uint32_t) NMC_INL { return (uint32_t)'_'; });
    w.template mem<F>(y.p_c6, y.c6_len, cg.blob, y.c6_at);
    w.gen(y.p_g2, y.len - y.p_g2, [&](uint32_t k) NMC_INL { return csn_g2(y, k); });
    return w.o;
}

// ---- dcs: dcs_consensus_tag(t, d) -------------------------------------------------------------------
// 0x80 in every byte of x that equals c, 0 elsewhere (exact: no carry crosses a byte)
NMC_HD uint64_t eq_bytes(uint64_t x, uint32_t c) {
    const uint64_t k7 = 0x7f7f7f7f7f7f7f7full;
    const uint64_t y = x ^ (0x0101010101010101ull * c);
    return ~(((y & k7) + k7) | y | k7);
}
NMC_HD uint32_t first_byte(uint64_t m) { return (uint32_t)__builtin_ctzll(m) >> 3; }
NMC_HD uint32_t last_byte(uint64_t m) { return (63u - (uint32_t)__builtin_clzll(m)) >> 3; }

// what the rule needs to know of a name of len bytes: `len` stands for "not there"
struct Scan {
    uint32_t us1, usl, c1, c2;   // its first and last '_', its first and second ':'
    uint32_t pos;                // "pos" somewhere in it
};
// F::word(base, a, valid): the 8 bytes at base + a (a a multiple of 8), bytes from `valid` (1..8) on zero
template <class F>
NMC_HD Scan scan_name(const uint8_t* base, uint64_t at, uint32_t len) {
    Scan s{len, len, len, len, 0u};
    uint64_t pp = 0, po = 0;   // the previous word's 'p' and 'o' bytes
    for (uint32_t w = 0; w < len; w += 8u) {
        const uint32_t valid = len - w < 8u ? len - w : 8u;
        const uint64_t x = F::word(base, at + w, valid);
        const uint64_t U = eq_bytes(x, '_');
        uint64_t C = eq_bytes(x, ':');
        if (U) {
            if (s.us1 == len) s.us1 = w + first_byte(U);
            s.usl = w + last_byte(U);
        }
        if (C && s.c1 == len) {
            s.c1 = w + first_byte(C);
            C &= C - 1ull;
        }
        if (C && s.c2 == len) s.c2 = w + first_byte(C);
        const uint64_t P = eq_bytes(x, 'p'), O = eq_bytes(x, 'o'), S = eq_bytes(x, 's');
        // inside the word; 'p' the last byte before it; "po" the last two bytes before it
        const uint64_t hit = (P & (O >> 8) & (S >> 16)) | ((pp >> 56) & O & (S >> 8) & 0x80ull) |
                             ((pp >> 48) & (po >> 56) & S & 0x80ull);
        s.pos |= hit != 0;
        pp = P;
        po = O;
    }
    return s;
}

// t[0, tb) and d[0, db) the barcodes, t[tb + 1, tb + 1 + cl) the coordinates, t[t1 + 1, t1 + 1 + tfl)
// and d[d1 + 1, d1 + 1 + dfl) the fields; pos: t's halves first.  Every value is at most 255.
struct DcsLay {
    uint32_t tb, db, cl, t1, tfl, d1, dfl, pos, len;
};
NMC_HD uint64_t dcs_pack(const DcsLay& y) {
    return (uint64_t)y.tb | ((uint64_t)y.db << 8) | ((uint64_t)y.cl << 16) | ((uint64_t)y.t1 << 24) | ((uint64_t)y.tfl << 32) |
           ((uint64_t)y.d1 << 40) | ((uint64_t)y.dfl << 48) | ((uint64_t)y.pos << 56);
}
NMC_HD DcsLay dcs_unpack(uint64_t v) {
    DcsLay y;
    y.tb = (uint32_t)v & 0xffu; y.db = (uint32_t)(v >> 8) & 0xffu; y.cl = (uint32_t)(v >> 16) & 0xffu;
    y.t1 = (uint32_t)(v >> 24) & 0xffu; y.tfl = (uint32_t)(v >> 32) & 0xffu; y.d1 = (uint32_t)(v >> 40) & 0xffu;
    y.dfl = (uint32_t)(v >> 48) & 0xffu; y.pos = (uint32_t)(v >> 56) & 1u;
    y.len = y.tb + 1u + y.db + 1u + y.cl + 1u + y.tfl + 1u + y.dfl;
    return y;
}

// The pair laid out: the tag name is base[ta, ta + tl), the partner base[da, da + dl), both at most
// 255 bytes at 8-byte aligned offsets.  Returns the refusal bits, 0 when y is valid.
template <class F>
NMC_HD uint32_t dcs_layout(const uint8_t* base, uint64_t ta, uint32_t tl, uint64_t da, uint32_t dl, DcsLay& y) {
    const Scan t = scan_name<F>(base, ta, tl);
    if (t.us1 == tl) return NE_T_NOUS;
    if (t.c1 == tl) return NE_T_NOCOLON;
    const Scan d = scan_name<F>(base, da, dl);
    if (d.c1 == dl) return NE_D_NOCOLON;
    y.tb = t.us1;
    y.db = d.us1;   // (no '_': all of d)
    y.cl = (t.usl > t.us1 ? t.usl : tl) - t.us1 - 1u;   // the rest up to its last '_', or all of it
    y.t1 = t.c1;
    y.tfl = t.c2 - t.c1 - 1u;
    y.d1 = d.c1;
    y.dfl = d.c2 - d.c1 - 1u;
    y.pos = t.pos;
    y.len = y.tb + 1u + y.db + 1u + y.cl + 1u + y.tfl + 1u + y.dfl;
    return 0;
}

// The 16 bytes at offset j of the name y, bytes from `valid` (1..16, j + valid <= y.len) on zero.
template <class F>
NMC_HD W16 dcs_out16(const DcsLay& y, const uint8_t* base, uint64_t ta, uint64_t da, uint32_t j, uint32_t valid) {
    Win w{W16{{0u, 0u, 0u, 0u}}, j, j + valid};
    const bool p = y.pos != 0u;
    // barcode _ barcode _ coordinates : field _ field
    const uint64_t b0 = p ? ta : da, b1 = p ? da : ta;
    const uint32_t l0 = p ? y.tb : y.db, l1 = p ? y.db : y.tb;
    const uint64_t f0 = p ? ta + y.t1 + 1u : da + y.d1 + 1u, f1 = p ? da + y.d1 + 1u : ta + y.t1 + 1u;
    const uint32_t m0 = p ? y.tfl : y.dfl, m1 = p ? y.dfl : y.tfl;
    uint32_t at = 0;
    auto sep = [&](uint32_t c) NMC_INL {
        w.gen(at, 1u, [c](uint32_t) NMC_INL { return c; });
        at += 1u;
    };
    w.template mem<F>(at, l0, base, b0); at += l0;
    sep('_');
    w.template mem<F>(at, l1, base, b1); at += l1;
    sep('_');
    w.template mem<F>(at, y.cl, base, ta + y.tb + 1u); at += y.cl;
    sep(':');
    w.template mem<F>(at, m0, base, f0); at += m0;
    sep('_');
    w.template mem<F>(at, m1, base, f1);
    return w.o;
}

// the plain byte-at-a-time source (host code, and what the device's aligned loads must agree with):
// never reads a byte at or past a + valid
struct ByteSrc {
    static NMC_HD W16 fetch(const uint8_t* base, uint64_t a, uint32_t valid) { return asmb::ByteFetch::fetch(base, a, valid); }
    static NMC_HD uint64_t word(const uint8_t* base, uint64_t a, uint32_t valid) {
        uint64_t w = 0;
        for (uint32_t k = 0; k < valid; ++k) w |= (uint64_t)base[a + k] << (8u * k);
        return w;
    }
};

#if !defined(__HIPCC__)
// A name's bytes as the write kernels cut them: a head up to the blob's next 16-byte line, then whole
// lines, the rest; out16(j, v) gives the v bytes at offset j of the name.
template <class Out>
inline void write_cut(uint8_t* blob, uint64_t off, uint32_t len, Out out16) {
    uint32_t v = (16u - (uint32_t)(off & 15u)) & 15u;
    for (uint32_t j = 0; j < len; j += v, v = 16u) {
        v = v ? v : 16u;
        v = len - j < v ? len - j : v;
        const W16 w = out16(j, v);
        for (uint32_t b = 0; b < v; ++b) blob[off + j + b] = (uint8_t)(w.w[b >> 2] >> (8 * (b & 3)));
    }
}

// The whole formatting on the host, as the device runs it: the sizes pass, the offsets, then every name
// in 16-byte cuts into a blob of exactly the total.  Returns -1 when every name was accepted, else the
// first refused name (*err its bits).
inline int64_t csn_host(int64_t n, const int32_t* f9, const int64_t* suffix, const Strs& bc, const Strs& cg,
                        std::vector<uint8_t>& blob, std::vector<int64_t>& off, uint32_t* err) {
    off.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        CsnLay y;
        const uint32_t e = csn_layout(f9 + 9 * i, suffix[i], bc, cg, y);
        if (e) { *err = e; return i; }
        off[(size_t)i + 1] = off[(size_t)i] + y.len;
    }
    blob.assign((size_t)off[(size_t)n], 0xee);
    for (int64_t i = 0; i < n; ++i) {
        CsnLay y;
        csn_layout(f9 + 9 * i, suffix[i], bc, cg, y);
        write_cut(blob.data(), (uint64_t)off[(size_t)i], y.len,
                  [&](uint32_t j, uint32_t v) { return csn_out16<ByteSrc>(y, bc, cg, j, v); });
    }
    *err = 0;
    return -1;
}

// base: the table's qname blob; qn_off / qn_len: its slots, nrec of them
inline int64_t dcs_host(int64_t n, const int64_t* rec_tag, const int64_t* rec_ds, const uint8_t* base, const uint64_t* qn_off,
                        const uint16_t* qn_len, int64_t nrec, std::vector<uint8_t>& blob, std::vector<int64_t>& off,
                        uint32_t* err) {
    off.assign((size_t)n + 1, 0);
    std::vector<uint64_t> lay((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t rt = rec_tag[i], rd = rec_ds[i];
        if (rt < 0 || rt >= nrec || rd < 0 || rd >= nrec) { *err = NE_REC; return i; }
        DcsLay y;
        const uint32_t e = dcs_layout<ByteSrc>(base, qn_off[rt], qn_len[rt], qn_off[rd], qn_len[rd], y);
        if (e) { *err = e; return i; }
        lay[(size_t)i] = dcs_pack(y);
        off[(size_t)i + 1] = off[(size_t)i] + y.len;
    }
    blob.assign((size_t)off[(size_t)n], 0xee);
    for (int64_t i = 0; i < n; ++i) {
        const DcsLay y = dcs_unpack(lay[(size_t)i]);
        const uint64_t ta = qn_off[rec_tag[i]], da = qn_off[rec_ds[i]];
        write_cut(blob.data(), (uint64_t)off[(size_t)i], y.len,
                  [&](uint32_t j, uint32_t v) { return dcs_out16<ByteSrc>(y, base, ta, da, j, v); });
    }
    *err = 0;
    return -1;
}
#endif

}  // namespace nmc

#endif
