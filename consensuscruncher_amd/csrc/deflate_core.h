// The serial parts of the DEFLATE (RFC 1951) encoder behind the device BGZF writer: symbol tables,
// the length-limited Huffman code builder, canonical code assignment and the dynamic-block header.
// Plain C++ that compiles in the HIP kernel (bgzf_deflate.hip.inc) and with a host compiler
// (tests/asan/deflate_core_driver.cpp runs it under sanitizers), so both execute the same text.
// No tables in memory: every symbol mapping is arithmetic.
#ifndef CC_DEFLATE_CORE_H
#define CC_DEFLATE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DFL_HD __host__ __device__ inline
#else
#define DFL_HD inline
#endif

namespace dfl {

constexpr int NLIT = 286;    // literal/length symbols 0..285 (256 = end of block)
constexpr int NDIST = 30;    // distance symbols
constexpr int NCL = 19;      // code-length alphabet
constexpr int MIN_MATCH = 3, MAX_MATCH = 258, WINDOW = 32768;
constexpr int MAX_ITEMS = NLIT + NDIST;   // the header's run-length items never outnumber the lengths

DFL_HD int ilog2(uint32_t x) { return 31 - __builtin_clz(x); }

// match length 3..258 -> symbol 257..285, its extra-bit count and value
DFL_HD int len_sym(int len, int* ebits, int* eval) {
    if (len == MAX_MATCH) { *ebits = 0; *eval = 0; return 285; }
    const int l = len - MIN_MATCH;
    if (l < 8) { *ebits = 0; *eval = 0; return 257 + l; }
    const int e = ilog2((uint32_t)l) - 2;
    *ebits = e;
    *eval = l & ((1 << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}

// distance 1..32768 -> symbol 0..29, its extra-bit count and value
DFL_HD int dist_sym(int dist, int* ebits, int* eval) {
    const int d = dist - 1;
    if (d < 4) { *ebits = 0; *eval = 0; return d; }
    const int hb = ilog2((uint32_t)d);
    *ebits = hb - 1;
    *eval = d & ((1 << (hb - 1)) - 1);
    return 2 * hb + ((d >> (hb - 1)) & 1);
}

DFL_HD int lit_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
DFL_HD int dist_extra_bits(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
DFL_HD int fixed_lit_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

DFL_HD uint32_t bit_reverse(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

// A decoder wants every tree to hold at least two codes (zlib's rule): the smallest unused symbols
// get a count of 1 until two are in use.  Returns the number of symbols in use.
DFL_HD int ensure_two(uint32_t* freq, int n, int used) {
    for (int s = 0; s < n && used < 2; ++s)
        if (!freq[s]) { freq[s] = 1; ++used; }
    return used;
}

// Symbols in use, sorted by (count, symbol) ascending: val[k] their counts, sym[k] their numbers.
// A rank sort; the kernel computes the same ranks with one symbol per thread.
DFL_HD int sort_used(const uint32_t* freq, int n, uint32_t* val, uint16_t* sym) {
    int m = 0;
    for (int s = 0; s < n; ++s) {
        if (!freq[s]) continue;
        int r = 0;
        for (int j = 0; j < n; ++j)
            if (freq[j] && (freq[j] < freq[s] || (freq[j] == freq[s] && j < s))) ++r;
        val[r] = freq[s];
        sym[r] = (uint16_t)s;
        ++m;
    }
    return m;
}

// Moffat and Katajainen's in-place minimum-redundancy code lengths: A holds m >= 2 counts in
// ascending order and ends up holding the code lengths (non-increasing).
DFL_HD void huffman_lengths(uint32_t* A, int m) {
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < m - 1; ++next) {
        if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
        else A[next] = A[leaf++];
        if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
        else A[next] += A[leaf++];
    }
    A[m - 2] = 0;
    for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = m - 2;
    next = m - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
}

// Lengths A[0..m) (non-increasing, any size) limited to maxbits with the Kraft sum kept at one:
// codes longer than the limit move to it, then for each unit of overflow one code leaves the limit
// and pairs with the deepest shorter code one level down.  The frequency order is kept.
// Scratch arrays are the caller's (work, WORK words): the kernel keeps them in LDS, not in private
// memory.
constexpr int WORK = 36;
DFL_HD void limit_lengths(uint32_t* A, int m, int maxbits, uint32_t* bl /* WORK words */) {
    for (int l = 0; l <= 32; ++l) bl[l] = 0;
    for (int k = 0; k < m; ++k) bl[A[k] > (uint32_t)maxbits ? (uint32_t)maxbits : A[k]]++;
    uint64_t total = 0;
    for (int l = 1; l <= maxbits; ++l) total += (uint64_t)bl[l] << (maxbits - l);
    while (total > (1ull << maxbits)) {
        bl[maxbits]--;
        for (int l = maxbits - 1; l >= 1; --l)
            if (bl[l]) { bl[l]--; bl[l + 1] += 2; break; }
        --total;
    }
    int k = 0;
    for (int l = maxbits; l >= 1; --l)
        for (uint32_t c = 0; c < bl[l]; ++c) A[k++] = (uint32_t)l;
}

// Code lengths (<= maxbits) of n symbols from their counts; a symbol not in use gets 0.  freq may
// gain the dummy counts of ensure_two.  val (n words), sym (n halfwords) and work are scratch.
DFL_HD void build_lengths(uint32_t* freq, int n, int maxbits, uint8_t* len, uint32_t* val, uint16_t* sym,
                          uint32_t* work) {
    int used = 0;
    for (int s = 0; s < n; ++s) used += freq[s] != 0;
    ensure_two(freq, n, used);
    const int m = sort_used(freq, n, val, sym);
    huffman_lengths(val, m);
    limit_lengths(val, m, maxbits, work);
    for (int s = 0; s < n; ++s) len[s] = 0;
    for (int k = 0; k < m; ++k) len[sym[k]] = (uint8_t)val[k];
}

// Canonical codes (RFC 1951 3.2.2) from lengths, bit-reversed: DEFLATE packs Huffman codes from
// their most significant bit while the stream fills bytes from the least.
DFL_HD void canonical_codes(const uint8_t* len, int n, uint16_t* code, uint32_t* work) {
    uint32_t* cnt = work;
    uint32_t* nextc = work + 16;
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) cnt[len[s]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    nextc[0] = 0;
    for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; nextc[l] = c; }
    for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)bit_reverse(nextc[len[s]]++, len[s]) : 0;
}

DFL_HD int cl_order(int k) {   // the order in which the header stores the code-length code lengths:
    if (k < 3) return 16 + k;  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const int j = k - 3;
    return j == 0 ? 0 : (j & 1) ? 8 + (j >> 1) : 8 - (j >> 1);
}

// What the dynamic header needs, worked out before any bit is written.
struct DynHeader {
    int hlit, hdist, hclen, nitems;
    uint32_t bits;                 // the header's size, the 3 block-type bits included
    uint8_t cl_len[NCL];
    uint16_t cl_code[NCL];
    uint8_t item_sym[MAX_ITEMS];   // code-length symbols 0..18 in stream order
    uint8_t item_ext[MAX_ITEMS];   // the repeat count's extra-bit value for 16, 17, 18
    uint32_t cl_freq[NCL], val[NCL], work[WORK];   // scratch
    uint16_t sym[NCL];
};

DFL_HD int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// The HLIT/HDIST/HCLEN header of a dynamic block for the given code lengths: the two length lists
// as one sequence, run-length coded with 16 (repeat previous 3-6), 17 (zeros 3-10) and 18 (zeros
// 11-138), and the 7-bit-limited code for those symbols.
DFL_HD void plan_header(const uint8_t* llen, const uint8_t* dlen, DynHeader* h) {
    int hlit = NLIT, hdist = NDIST;
    while (hlit > 257 && !llen[hlit - 1]) --hlit;
    while (hdist > 1 && !dlen[hdist - 1]) --hdist;
    h->hlit = hlit;
    h->hdist = hdist;
    const int total = hlit + hdist;
    uint32_t* clfreq = h->cl_freq;
    for (int s = 0; s < NCL; ++s) clfreq[s] = 0;
    int ni = 0;
    for (int i = 0; i < total;) {
        const int v = i < hlit ? llen[i] : dlen[i - hlit];
        int run = 1;
        while (i + run < total && (i + run < hlit ? llen[i + run] : dlen[i + run - hlit]) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                h->item_sym[ni] = 18; h->item_ext[ni++] = (uint8_t)(r - 11); clfreq[18]++;
                run -= r;
            }
            if (run >= 3) {
                h->item_sym[ni] = 17; h->item_ext[ni++] = (uint8_t)(run - 3); clfreq[17]++;
                run = 0;
            }
        } else {
            h->item_sym[ni] = (uint8_t)v; h->item_ext[ni++] = 0; clfreq[v]++;
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                h->item_sym[ni] = 16; h->item_ext[ni++] = (uint8_t)(r - 3); clfreq[16]++;
                run -= r;
            }
        }
        for (; run > 0; --run) { h->item_sym[ni] = (uint8_t)v; h->item_ext[ni++] = 0; clfreq[v]++; }
    }
    h->nitems = ni;
    build_lengths(clfreq, NCL, 7, h->cl_len, h->val, h->sym, h->work);
    canonical_codes(h->cl_len, NCL, h->cl_code, h->work);
    int hclen = NCL;
    while (hclen > 4 && !h->cl_len[cl_order(hclen - 1)]) --hclen;
    h->hclen = hclen;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int k = 0; k < ni; ++k) bits += h->cl_len[h->item_sym[k]] + (uint32_t)cl_extra_bits(h->item_sym[k]);
    h->bits = bits;
}

// Writes the block-type bits (final block, BTYPE 10) and the planned header through sink.put(value,
// nbits), least significant bit first.
template <class Sink>
DFL_HD void write_header(const DynHeader* h, Sink& sink) {
    sink.put(1u | (2u << 1), 3);
    sink.put((uint32_t)(h->hlit - 257), 5);
    sink.put((uint32_t)(h->hdist - 1), 5);
    sink.put((uint32_t)(h->hclen - 4), 4);
    for (int k = 0; k < h->hclen; ++k) sink.put(h->cl_len[cl_order(k)], 3);
    for (int k = 0; k < h->nitems; ++k) {
        const int s = h->item_sym[k];
        sink.put(h->cl_code[s], h->cl_len[s]);
        const int e = cl_extra_bits(s);
        if (e) sink.put(h->item_ext[k], e);
    }
}

// A token as the kernel and the driver exchange it: a literal byte, or a match.
// bits 16..24 length (0: literal), bits 0..15 distance - 1 (or the literal byte).
DFL_HD uint32_t tok_lit(uint8_t b) { return b; }
DFL_HD uint32_t tok_match(int len, int dist) { return ((uint32_t)len << 16) | (uint32_t)(dist - 1); }

// The token's bits (<= 48) and their count under the given codes.
DFL_HD int tok_bits(uint32_t tok, const uint8_t* llen, const uint16_t* lcode, const uint8_t* dlen,
                    const uint16_t* dcode, uint64_t* out) {
    const int len = (int)(tok >> 16);
    if (!len) {
        const int b = (int)(tok & 0xff);
        *out = lcode[b];
        return llen[b];
    }
    int eb, ev, n;
    const int ls = len_sym(len, &eb, &ev);
    uint64_t v = lcode[ls];
    n = llen[ls];
    v |= (uint64_t)ev << n;
    n += eb;
    const int ds = dist_sym((int)(tok & 0xffff) + 1, &eb, &ev);
    v |= (uint64_t)dcode[ds] << n;
    n += dlen[ds];
    v |= (uint64_t)ev << n;
    n += eb;
    *out = v;
    return n;
}

}  // namespace dfl

#endif
