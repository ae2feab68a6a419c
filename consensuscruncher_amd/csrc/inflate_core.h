// The serial parts of the DEFLATE (RFC 1951) decoder behind the device BGZF reader: the bit reader,
// the stored / fixed / dynamic block headers, the code-length code, the decode tables built from
// code lengths, the length and distance bases, and the symbol loop.  Plain C++ that compiles in the
// HIP kernel (bgzf_inflate.hip.inc) and with a host compiler (tests/asan/inflate_core_driver.cpp
// runs it under sanitizers), so both execute the same text.
//
// The contract (a corrupt member must never fault a device other people share):
//   * input is read only through Src::word(i, valid) with i + valid <= clen;
//   * output is produced only through Sink::lit / Sink::match, after the core has checked that the
//     bytes fit in ulen and that a match's distance is <= min(bytes produced so far, 32768);
//   * over-subscribed code-length sets are refused, incomplete ones too, except a distance code
//     that is empty or a single one-bit code, which zlib accepts as well.  (This is stricter than
//     zlib in one place: zlib also accepts a literal/length code that is a single one-bit code, an
//     end-of-block-only block; the core refuses it, and such a member goes to the host codec.)
//     Symbols 286, 287, 30 and 31, a stored LEN that is not ~NLEN and a block type 3 are refused;
//   * a member is good (R_DONE) only if a final block ended and exactly ulen bytes were produced;
//   * every loop iteration consumes at least one input bit or fails, so work is bounded by 8 * clen.
// run() can pause (R_PAUSE) when the sink is full or the staged input runs low, and resumes where
// it stopped: the kernel decodes a member in batches; on the host it runs through in one call.
#ifndef CC_INFLATE_CORE_H
#define CC_INFLATE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define IFL_HD __host__ __device__ inline
#else
#define IFL_HD inline
#endif

namespace ifl {

constexpr int MAXBITS = 15;
constexpr int FAST_BITS = 9, FAST = 1 << FAST_BITS;   // codes up to 9 bits decode by one table read
constexpr int NLIT = 288, NDIST = 32, NCL = 19;       // table capacities (286 / 30 symbols are valid)
constexpr int WINDOW = 32768;
constexpr int LENS = NLIT + NDIST + NCL + 1;          // the code lengths of a header, then the 19 of the code-length code
constexpr int CL_AT = NLIT + NDIST;
constexpr uint32_t HEADER_BYTES = 640;   // a block header never spans more (17 + 57 + 316 * 14 bits)
constexpr uint32_t SYMBOL_BYTES = 8;     // nor a length/distance pair (48 bits)

enum { R_PAUSE = 0, R_DONE = 1, R_FAIL = 2 };
enum { P_HEAD = 0, P_STORED = 1, P_CODES = 2, P_DONE = 3, P_FAIL = 4 };

// A canonical Huffman decoder: fast[] answers codes of up to FAST_BITS bits (sym | len << 9, 0 for
// none), count[] / sym[] answer the longer ones by length counts.
template <int N>
struct Huff {
    uint16_t fast[FAST];
    uint16_t count[MAXBITS + 1];
    uint16_t sym[N];
};

struct Tables {   // the caller's storage (LDS in the kernel)
    Huff<NLIT>* L;
    Huff<NDIST>* D;       // also holds the code-length code while a dynamic header is read
    uint8_t* lens;        // LENS bytes
    uint16_t* offs;       // MAXBITS + 1 words of scratch
};

// where a member stands between two calls of run()
struct State {
    uint32_t phase, last, stored_left, produced, ulen;
};

// LSB-first bit reader over bytes [0, end); only [0, avail) is staged so far (avail == end on the host).
template <class Src>
struct Bits {
    Src src;
    uint32_t pos, end, avail;   // pos: the next byte not yet in buf
    uint32_t cnt;               // valid bits in buf (the rest are zero)
    uint64_t buf;

    IFL_HD void refill() {
        while (cnt <= 32 && pos < avail) {
            const uint32_t left = avail - pos, valid = left < 4 ? left : 4;
            buf |= (uint64_t)src.word(pos, valid) << cnt;
            cnt += 8 * valid;
            pos += valid;
        }
    }
    // n <= 16 bits; false when the member has fewer left
    IFL_HD bool take(uint32_t n, uint32_t* v) {
        if (cnt < n) refill();
        if (cnt < n) return false;
        *v = (uint32_t)buf & ((1u << n) - 1);
        buf >>= n;
        cnt -= n;
        return true;
    }
    IFL_HD void drop(uint32_t n) { buf >>= n; cnt -= n; }
    IFL_HD void align() { drop(cnt & 7); }
    // fewer than need bytes are staged although the member has more: pause for the next stage
    IFL_HD bool low(uint32_t need) const { return avail < end && (avail - pos) + (cnt >> 3) < need; }
};

IFL_HD uint32_t bit_reverse(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

// the order the code-length code's own lengths are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
IFL_HD int cl_order(int i) {
    constexpr uint64_t A = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                           6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t B = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? A >> (5 * i) : B >> (5 * (i - 12))) & 31);
}

// length symbol 257..285 -> base and extra-bit count; distance symbol 0..29 likewise
IFL_HD void len_base(int sym, uint32_t* base, uint32_t* ebits) {
    if (sym < 265) { *base = (uint32_t)(sym - 254); *ebits = 0; return; }
    if (sym == 285) { *base = 258; *ebits = 0; return; }
    const uint32_t e = (uint32_t)(sym - 261) >> 2;
    *ebits = e;
    *base = 3 + ((4 + ((uint32_t)(sym - 261) & 3)) << e);
}
IFL_HD void dist_base(int sym, uint32_t* base, uint32_t* ebits) {
    if (sym < 4) { *base = (uint32_t)sym + 1; *ebits = 0; return; }
    const uint32_t e = ((uint32_t)sym >> 1) - 1;
    *ebits = e;
    *base = 1 + ((2 + ((uint32_t)sym & 1)) << e);
}

enum { H_COMPLETE = 0, H_INCOMPLETE = 1, H_EMPTY = 2, H_OVER = -1 };

// The decoder of the code with lengths lens[0..n) (0: unused), n <= the capacity of sym[].
// H_OVER leaves the tables unusable; the caller decides about H_INCOMPLETE and H_EMPTY.
IFL_HD int build(uint16_t* fast, uint16_t* count, uint16_t* sym, const uint8_t* lens, int n, uint16_t* offs) {
    for (int l = 0; l <= MAXBITS; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) count[lens[s] & 15] += 1;
    for (int i = 0; i < FAST; ++i) fast[i] = 0;
    if (count[0] == n) return H_EMPTY;
    int left = 1;
    for (int l = 1; l <= MAXBITS; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return H_OVER;
    }
    offs[1] = 0;
    for (int l = 1; l < MAXBITS; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        if (l) sym[offs[l]++] = (uint16_t)s;
    }
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= FAST_BITS; ++l) {
        for (int j = 0; j < (int)count[l]; ++j) {
            const uint16_t e = (uint16_t)(sym[idx++] | (l << 9));
            for (uint32_t k = bit_reverse(code, l); k < (uint32_t)FAST; k += 1u << l) fast[k] = e;
            ++code;
        }
        code <<= 1;
    }
    return left > 0 ? H_INCOMPLETE : H_COMPLETE;
}

// the next symbol, -1 for a code the tables do not hold or one that runs past the member's end
template <class Src>
IFL_HD int decode(const uint16_t* fast, const uint16_t* count, const uint16_t* sym, Bits<Src>& b) {
    if (b.cnt < (uint32_t)MAXBITS) b.refill();
    const uint32_t e = fast[(uint32_t)b.buf & (FAST - 1)];
    if (e) {
        const uint32_t l = e >> 9;
        if (l > b.cnt) return -1;
        b.drop(l);
        return (int)(e & 511);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= MAXBITS; ++l) {
        if ((uint32_t)l > b.cnt) return -1;
        code |= (int)(b.buf >> (l - 1)) & 1;
        const int c = (int)count[l];
        if (code - c < first) {
            b.drop((uint32_t)l);
            return (int)sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// the two tables of a fixed block
IFL_HD bool fixed_tables(const Tables& t) {
    for (int s = 0; s < NLIT; ++s) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < NDIST; ++s) t.lens[NLIT + s] = 5;
    return build(t.L->fast, t.L->count, t.L->sym, t.lens, NLIT, t.offs) == H_COMPLETE &&
           build(t.D->fast, t.D->count, t.D->sym, t.lens + NLIT, NDIST, t.offs) == H_COMPLETE;
}

// a dynamic block's header: HLIT / HDIST / HCLEN, the code-length code, the run-length coded
// lengths, then the two tables
template <class Src>
IFL_HD bool dynamic_tables(const Tables& t, Bits<Src>& b) {
    uint32_t v;
    if (!b.take(14, &v)) return false;
    const int hlit = (int)(v & 31) + 257, hdist = (int)((v >> 5) & 31) + 1, hclen = (int)(v >> 10) + 4;
    if (hlit > 286 || hdist > 30) return false;
    uint8_t* cl = t.lens + CL_AT;
    for (int i = 0; i < NCL; ++i) cl[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        if (!b.take(3, &v)) return false;
        cl[cl_order(i)] = (uint8_t)v;
    }
    if (build(t.D->fast, t.D->count, t.D->sym, cl, NCL, t.offs) != H_COMPLETE) return false;
    const int total = hlit + hdist;
    int idx = 0;
    while (idx < total) {
        const int s = decode(t.D->fast, t.D->count, t.D->sym, b);
        if (s < 0 || s > 18) return false;
        if (s < 16) { t.lens[idx++] = (uint8_t)s; continue; }
        uint8_t prev = 0;
        int rep;
        if (s == 16) {
            if (idx == 0 || !b.take(2, &v)) return false;
            prev = t.lens[idx - 1];
            rep = 3 + (int)v;
        } else if (s == 17) {
            if (!b.take(3, &v)) return false;
            rep = 3 + (int)v;
        } else {
            if (!b.take(7, &v)) return false;
            rep = 11 + (int)v;
        }
        if (idx + rep > total) return false;
        while (rep--) t.lens[idx++] = prev;
    }
    if (t.lens[256] == 0) return false;   // no end-of-block code
    if (build(t.L->fast, t.L->count, t.L->sym, t.lens, hlit, t.offs) != H_COMPLETE) return false;
    const int rd = build(t.D->fast, t.D->count, t.D->sym, t.lens + hlit, hdist, t.offs);
    if (rd == H_OVER) return false;
    // zlib accepts an incomplete distance code only when it is a single one-bit code
    if (rd == H_INCOMPLETE && !(t.D->count[1] == 1 && t.D->count[0] == hdist - 1)) return false;
    return true;
}

// Decodes until the member ends (R_DONE), is refused (R_FAIL), or the sink is full or the staged
// input low (R_PAUSE: call again after draining / staging).  Sink: full(produced), lit(byte,
// produced), match(len, dist, produced); produced is the output offset the bytes go to.
template <class Src, class Sink>
IFL_HD int run(State& s, Bits<Src>& b, const Tables& t, Sink& k) {
    for (;;) {
        if (s.phase == P_HEAD) {
            if (s.last) {
                s.phase = s.produced == s.ulen ? P_DONE : P_FAIL;
                continue;
            }
            if (b.low(HEADER_BYTES)) return R_PAUSE;
            uint32_t v;
            if (!b.take(3, &v)) { s.phase = P_FAIL; continue; }
            s.last = v & 1;
            const uint32_t type = v >> 1;
            if (type == 0) {
                uint32_t len, nlen;
                b.align();
                if (!b.take(16, &len) || !b.take(16, &nlen) || (len ^ 0xffffu) != nlen || len > s.ulen - s.produced) {
                    s.phase = P_FAIL;
                    continue;
                }
                s.stored_left = len;
                s.phase = P_STORED;
            } else if (type == 1) {
                s.phase = fixed_tables(t) ? P_CODES : P_FAIL;
            } else if (type == 2) {
                s.phase = dynamic_tables(t, b) ? P_CODES : P_FAIL;
            } else {
                s.phase = P_FAIL;
            }
        } else if (s.phase == P_STORED) {
            while (s.stored_left) {
                if (k.full(s.produced) || b.low(SYMBOL_BYTES)) return R_PAUSE;
                uint32_t v;
                if (!b.take(8, &v)) { s.phase = P_FAIL; break; }
                k.lit((uint8_t)v, s.produced);
                s.produced += 1;
                s.stored_left -= 1;
            }
            if (s.phase == P_STORED) s.phase = P_HEAD;
        } else if (s.phase == P_CODES) {
            for (;;) {
                if (k.full(s.produced) || b.low(SYMBOL_BYTES)) return R_PAUSE;
                const int sym = decode(t.L->fast, t.L->count, t.L->sym, b);
                if (sym < 0) { s.phase = P_FAIL; break; }
                if (sym < 256) {
                    if (s.produced >= s.ulen) { s.phase = P_FAIL; break; }
                    k.lit((uint8_t)sym, s.produced);
                    s.produced += 1;
                    continue;
                }
                if (sym == 256) { s.phase = P_HEAD; break; }
                if (sym >= 286) { s.phase = P_FAIL; break; }
                uint32_t len, eb, ev, dist;
                len_base(sym, &len, &eb);
                if (!b.take(eb, &ev)) { s.phase = P_FAIL; break; }
                len += ev;
                const int ds = decode(t.D->fast, t.D->count, t.D->sym, b);
                if (ds < 0 || ds >= 30) { s.phase = P_FAIL; break; }
                dist_base(ds, &dist, &eb);
                if (!b.take(eb, &ev)) { s.phase = P_FAIL; break; }
                dist += ev;
                if (dist > s.produced || dist > (uint32_t)WINDOW || len > s.ulen - s.produced) { s.phase = P_FAIL; break; }
                k.match(len, dist, s.produced);
                s.produced += len;
            }
        } else {
            return s.phase == P_DONE ? R_DONE : R_FAIL;
        }
    }
}

// ---- the host's whole-member form (the test driver; the kernel has its own Src and Sink)
struct FlatSrc {
    const uint8_t* p;
    IFL_HD uint32_t word(uint32_t i, uint32_t valid) const {
        uint32_t w = 0;
        for (uint32_t k = 0; k < valid; ++k) w |= (uint32_t)p[i + k] << (8 * k);
        return w;
    }
};
struct FlatSink {
    uint8_t* out;
    IFL_HD bool full(uint32_t) const { return false; }
    IFL_HD void lit(uint8_t c, uint32_t at) { out[at] = c; }
    IFL_HD void match(uint32_t len, uint32_t dist, uint32_t at) {
        for (uint32_t i = 0; i < len; ++i) out[at + i] = out[at + i - dist];
    }
};

// in[0..clen) -> out[0..ulen); true when the member is good
IFL_HD bool inflate_flat(const uint8_t* in, uint32_t clen, uint8_t* out, uint32_t ulen, const Tables& t) {
    State s = {P_HEAD, 0, 0, 0, ulen};
    Bits<FlatSrc> b = {{in}, 0, clen, clen, 0, 0};
    FlatSink k = {out};
    return run(s, b, t, k) == R_DONE;
}

}  // namespace ifl

#endif
