// CRC-32 as zlib computes it (reflected polynomial 0xEDB88320, initial register and final XOR all
// ones) for the device BGZF coders: the generated tables, the GF(2) arithmetic that moves a register
// over zero bytes and joins CRCs, and the per-lane rule of k_crc32.  Plain C++ that compiles in the
// HIP kernel (bgzf_crc32.hip.inc), in the engine's host code (cc_crc32 joins the segments of a long
// range with combine) and with a host compiler alone (tests/asan/crc_core_driver.cpp runs it under
// sanitizers), so all of them execute the same text.  No table is written out: every entry comes
// from the polynomial.
//
// The register is the reflected one: bit 31 is x^0, bit 0 is x^31.  Pushing a zero byte through it
// multiplies it by x^8 modulo P, so `nbytes` zero bytes are one product with x^(8 * nbytes).
//
// Two identities keep the kernel simple:
//   (1) with a zero initial register, leading zero bytes leave the register at zero;
//   (2) crc(M) = raw0(M) ^ advance(0xffffffff, len(M)) ^ 0xffffffff, where raw0 is the register after
//       M from a zero start, without the final XOR (the register is linear in its start value).
// Together they let a segment that starts at any byte address be read as aligned 16-byte words with
// the leading pad bytes masked to zero.  Trailing bytes are not harmless: the last, partial word is
// processed over its valid bytes only.
//
// The per-lane rule (lane): a segment of len bytes starts pad (0..15) bytes into its first aligned
// word; its words are 0 .. nwords(pad, len) - 1.  Lane t of LANES takes words t, t + LANES, ...; between
// two of its words lie STRIDE_BYTES bytes of other lanes, which its register crosses as zeros (the
// stride operator, four 256-entry tables); after its last word it advances over the true count of
// bytes left in the segment.  The XOR of all lanes' registers is raw0 of the segment (linearity),
// and finish() adds identity (2).  Words are read only through Src::word16(w) with w < nwords.
#ifndef CC_CRC_CORE_H
#define CC_CRC_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

namespace crc {

constexpr uint32_t POLY = 0xedb88320u;
constexpr uint32_t ONE = 0x80000000u;        // x^0
constexpr uint32_t LANES = 256;              // k_crc32's workgroup
constexpr uint32_t STRIDE_BYTES = 16 * LANES - 16;   // 4,080: between the end of a lane's word and its next
constexpr uint32_t SEGMENT = 0x10000;        // a segment's longest
constexpr int SLICES = 4;                    // slice-by-4: 4 x 256 entries, as many again for the stride

struct W16 { uint32_t v[4]; };               // an aligned 16-byte word, little-endian

// the register after 8 * bytes zero bits, bit by bit (the definition the tables are made from)
CRC_HD uint32_t shift_bytes(uint32_t r, int bytes) {
    for (int k = 0; k < 8 * bytes; ++k) r = (r & 1) ? POLY ^ (r >> 1) : r >> 1;
    return r;
}

// a * b modulo P
CRC_HD uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = ONE; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? POLY ^ (b >> 1) : b >> 1;
    }
    return p;
}

// x^(8n) modulo P, by square and multiply
CRC_HD uint32_t xpow8n(uint64_t n) {
    uint32_t r = ONE, sq = ONE >> 8;   // x^8
    for (; n; n >>= 1) {
        if (n & 1) r = mulmod(r, sq);
        if (n > 1) sq = mulmod(sq, sq);
    }
    return r;
}

// the register v pushed through nbytes zero bytes
CRC_HD uint32_t advance(uint32_t v, uint64_t nbytes) { return mulmod(v, xpow8n(nbytes)); }

// zlib's crc32_combine: the CRC of A || B from the finalised CRCs of A and B and B's length
CRC_HD uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return advance(crc_a, len_b) ^ crc_b; }

// identity (2): the CRC of a message of len bytes from its zero-start register
CRC_HD uint32_t finish(uint32_t raw0, uint64_t len) { return raw0 ^ advance(0xffffffffu, len) ^ 0xffffffffu; }

// Table entries.  slice k, byte b: the register b after 1 + k bytes (slice 0 is the bytewise
// table); stride k, byte b: the register b << 8k after STRIDE_BYTES zero bytes.
CRC_HD uint32_t slice_entry(int k, uint32_t b) { return shift_bytes(b, 1 + k); }
CRC_HD uint32_t stride_entry(int k, uint32_t b, uint32_t xstride) { return mulmod(b << (8 * k), xstride); }

struct Tables {
    const uint32_t* slice;    // [SLICES][256]
    const uint32_t* stride;   // [4][256]
};

// both tables on the host (the kernel's threads fill theirs in LDS from the same entries)
inline void make_tables(uint32_t* slice, uint32_t* stride) {
    const uint32_t xs = xpow8n(STRIDE_BYTES);
    for (int k = 0; k < SLICES; ++k)
        for (uint32_t b = 0; b < 256; ++b) {
            slice[256 * k + b] = slice_entry(k, b);
            stride[256 * k + b] = stride_entry(k, b, xs);
        }
}

CRC_HD uint32_t byte_step(const Tables& T, uint32_t r, uint32_t byte) { return T.slice[(r ^ byte) & 0xff] ^ (r >> 8); }
CRC_HD uint32_t word_step(const Tables& T, uint32_t r, uint32_t w) {   // four bytes at once
    r ^= w;
    return T.slice[768 + (r & 0xff)] ^ T.slice[512 + ((r >> 8) & 0xff)] ^ T.slice[256 + ((r >> 16) & 0xff)] ^
           T.slice[r >> 24];
}
CRC_HD uint32_t stride_step(const Tables& T, uint32_t r) {   // r through STRIDE_BYTES zero bytes
    return T.stride[r & 0xff] ^ T.stride[256 + ((r >> 8) & 0xff)] ^ T.stride[512 + ((r >> 16) & 0xff)] ^
           T.stride[768 + (r >> 24)];
}

// the aligned words that overlap a segment (none for an empty one)
CRC_HD uint32_t nwords(uint32_t pad, uint32_t len) { return len ? (pad + len + 15) >> 4 : 0; }

// Lane t's share of raw0 of the segment, already advanced to the segment's end.
template <class Src>
CRC_HD uint32_t lane(const Tables& T, const Src& src, uint32_t pad, uint32_t len, uint32_t t) {
    const uint32_t nw = nwords(pad, len), end = pad + len;   // end: the segment's end from word 0's first byte
    if (t >= nw) return 0;
    uint32_t r = 0, done = 0;
    for (uint32_t w = t; w < nw; w += LANES) {
        if (w != t) r = stride_step(T, r);
        W16 x = src.word16(w);
        if (w == 0)   // identity (1): the pad bytes before the segment count as zeros
            for (uint32_t k = 0; k < 4; ++k)
                x.v[k] = pad >= 4 * k + 4 ? 0 : pad > 4 * k ? x.v[k] & (0xffffffffu << (8 * (pad - 4 * k))) : x.v[k];
        const uint32_t hi = end - 16 * w < 16 ? end - 16 * w : 16;   // valid bytes of this word
        for (uint32_t k = 0; k < 4; ++k) {
            if (hi >= 4 * k + 4) r = word_step(T, r, x.v[k]);
            else
                for (uint32_t q = 4 * k; q < hi; ++q) r = byte_step(T, r, (x.v[k] >> (8 * (q & 3))) & 0xff);
        }
        done = 16 * w + hi;
    }
    return advance(r, end - done);
}

}  // namespace crc

#endif
