// Stand-alone check of consensuscruncher_amd/csrc/deflate_core.h (the serial core the device BGZF
// encoder shares with the host): a trivial serial greedy matcher makes tokens, the shared code
// builder, symbol tables and header writer turn them into a raw DEFLATE stream in each block form,
// zlib inflates it, and the result must equal the input.  Built with -fsanitize=address,undefined
// by tests/test_deflate_core_host.py; exit 0 and a silent stderr are the pass.
// Arguments: files whose bytes are encoded as further inputs, in 0xff00-byte pieces.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../consensuscruncher_amd/csrc/deflate_core.h"

namespace {

typedef std::vector<uint8_t> Bytes;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 1) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
};

Bytes random_bytes(size_t n, uint64_t seed) {
    Rng r(seed);
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)r.next();
    return b;
}

Bytes text_like(size_t n, uint64_t seed) {
    static const char* words[] = {"ACGT", "chr1", "\t", "NNNN", "IIIIHHGG", "read", ":", "0", "147", "\n", "GATTACA", "="};
    Rng r(seed);
    Bytes b;
    while (b.size() < n) {
        const char* w = words[r.next() % 12];
        b.insert(b.end(), w, w + strlen(w));
        if (r.next() % 5 == 0) b.push_back((uint8_t)('!' + r.next() % 60));
    }
    b.resize(n);
    return b;
}

struct BitSink {
    Bytes out;
    uint64_t acc = 0;
    int fill = 0;
    uint64_t bits = 0;
    void put(uint64_t v, int n) {
        bits += (uint64_t)n;
        while (n > 0) {   // at most 32 bits at a time keeps acc within 64
            const int k = n < 32 ? n : 32;
            acc |= (v & ((1ull << k) - 1)) << fill;
            fill += k;
            v >>= k;
            n -= k;
            while (fill >= 8) { out.push_back((uint8_t)acc); acc >>= 8; fill -= 8; }
        }
    }
    void flush() { if (fill) { out.push_back((uint8_t)acc); acc = 0; fill = 0; } }
};

// greedy tokens: one hash candidate (the last position with the same 4-byte hash) and distance 1
std::vector<uint32_t> tokens_of(const Bytes& d) {
    const size_t n = d.size();
    std::vector<int32_t> head(1 << 13, -1);
    std::vector<uint32_t> t;
    auto extend = [&](size_t c, size_t i) {
        size_t l = 0;
        const size_t cap = std::min<size_t>(dfl::MAX_MATCH, n - i);
        while (l < cap && d[c + l] == d[i + l]) ++l;
        return l;
    };
    auto hash = [&](size_t i) {
        uint32_t w;
        memcpy(&w, &d[i], 4);
        return (w * 2654435761u) >> 19;
    };
    size_t i = 0;
    while (i < n) {
        size_t len = 0, dist = 0;
        if (i + 4 <= n) {
            const int32_t c = head[hash(i)];
            if (c >= 0 && i - (size_t)c <= (size_t)dfl::WINDOW) { len = extend((size_t)c, i); dist = i - (size_t)c; }
        }
        if (i >= 1) {
            const size_t l1 = extend(i - 1, i);
            if (l1 >= len) { len = l1; dist = 1; }
        }
        if (len < (size_t)dfl::MIN_MATCH) len = 0;
        const size_t adv = len ? len : 1;
        for (size_t k = i; k < i + adv && k + 4 <= n; ++k) head[hash(k)] = (int32_t)k;
        t.push_back(len ? dfl::tok_match((int)len, (int)dist) : dfl::tok_lit(d[i]));
        i += adv;
    }
    return t;
}

int fail(const std::string& what) {
    fprintf(stderr, "deflate_core_driver: %s\n", what.c_str());
    return 1;
}

bool inflate_equals(const Bytes& comp, const Bytes& want, const std::string& name) {
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) return false;
    Bytes got(want.size() + 16);
    z.next_in = const_cast<uint8_t*>(comp.data());
    z.avail_in = (uInt)comp.size();
    z.next_out = got.data();
    z.avail_out = (uInt)got.size();
    const int rc = inflate(&z, Z_FINISH);
    const size_t n = got.size() - z.avail_out;
    const bool ok = rc == Z_STREAM_END && z.avail_in == 0 && n == want.size() &&
                    (n == 0 || memcmp(got.data(), want.data(), n) == 0);
    inflateEnd(&z);
    if (!ok) fprintf(stderr, "deflate_core_driver: %s: inflate rc=%d, %zu of %zu bytes, %u unused\n", name.c_str(), rc, n,
                     want.size(), z.avail_in);
    return ok;
}

struct Codes {
    uint8_t llen[dfl::NLIT], dlen[dfl::NDIST];
    uint16_t lcode[dfl::NLIT], dcode[dfl::NDIST];
};

// the block for tokens under codes c; dyn: with the dynamic header, else the fixed block type
Bytes emit(const std::vector<uint32_t>& toks, const Codes& c, const dfl::DynHeader* dyn, uint64_t* bits) {
    BitSink s;
    if (dyn) dfl::write_header(dyn, s);
    else s.put(1u | (1u << 1), 3);
    for (uint32_t t : toks) {
        uint64_t v;
        const int n = dfl::tok_bits(t, c.llen, c.lcode, c.dlen, c.dcode, &v);
        if (n <= 0 || n > 48) { fprintf(stderr, "deflate_core_driver: token of %d bits\n", n); exit(1); }
        s.put(v, n);
    }
    s.put(c.lcode[256], c.llen[256]);
    *bits = s.bits;
    s.flush();
    return s.out;
}

// lengths are a complete prefix code within the limit, and every counted symbol has a code
bool check_lengths(const uint8_t* len, const uint32_t* freq, int n, int maxbits, const std::string& name) {
    uint64_t kraft = 0;
    int used = 0;
    for (int s = 0; s < n; ++s) {
        if (freq[s] && !len[s]) { fprintf(stderr, "deflate_core_driver: %s: symbol %d has no code\n", name.c_str(), s); return false; }
        if (len[s] > maxbits) { fprintf(stderr, "deflate_core_driver: %s: length %d over %d\n", name.c_str(), len[s], maxbits); return false; }
        if (len[s]) { kraft += 1ull << (maxbits - len[s]); ++used; }
    }
    if (used < 2 || kraft != (1ull << maxbits)) {
        fprintf(stderr, "deflate_core_driver: %s: %d codes, Kraft sum %llu of %llu\n", name.c_str(), used,
                (unsigned long long)kraft, 1ull << maxbits);
        return false;
    }
    return true;
}

// unlimited Huffman cost by repeated merging of the two smallest (the yardstick for huffman_lengths)
uint64_t huffman_cost(std::vector<uint64_t> f) {
    uint64_t cost = 0;
    while (f.size() > 1) {
        std::sort(f.begin(), f.end(), std::greater<uint64_t>());
        const uint64_t a = f.back(); f.pop_back();
        const uint64_t b = f.back(); f.pop_back();
        cost += a + b;
        f.push_back(a + b);
    }
    return cost;
}

bool build_codes(std::vector<uint32_t>& lf, std::vector<uint32_t>& df, Codes* c, const std::string& name) {
    uint32_t val[dfl::NLIT], work[dfl::WORK];
    uint16_t sym[dfl::NLIT];
    dfl::build_lengths(lf.data(), dfl::NLIT, 15, c->llen, val, sym, work);
    dfl::build_lengths(df.data(), dfl::NDIST, 15, c->dlen, val, sym, work);
    if (!check_lengths(c->llen, lf.data(), dfl::NLIT, 15, name + " lit") ||
        !check_lengths(c->dlen, df.data(), dfl::NDIST, 15, name + " dist"))
        return false;
    dfl::canonical_codes(c->llen, dfl::NLIT, c->lcode, work);
    dfl::canonical_codes(c->dlen, dfl::NDIST, c->dcode, work);
    return true;
}

bool one_piece(const Bytes& d, const std::string& name) {
    const std::vector<uint32_t> toks = tokens_of(d);
    std::vector<uint32_t> lf(dfl::NLIT, 0), df(dfl::NDIST, 0);
    size_t covered = 0;
    for (uint32_t t : toks) {
        const int len = (int)(t >> 16);
        if (!len) { lf[t & 0xff]++; covered += 1; continue; }
        int eb, ev;
        const int dist = (int)(t & 0xffff) + 1;
        if (len < dfl::MIN_MATCH || len > dfl::MAX_MATCH || dist > dfl::WINDOW) return !fail(name + ": bad token");
        const int ls = dfl::len_sym(len, &eb, &ev);
        if (ls < 257 || ls > 285 || eb != dfl::lit_extra_bits(ls)) return !fail(name + ": length symbol");
        lf[ls]++;
        const int ds = dfl::dist_sym(dist, &eb, &ev);
        if (ds < 0 || ds > 29 || eb != dfl::dist_extra_bits(ds)) return !fail(name + ": distance symbol");
        df[ds]++;
        covered += (size_t)len;
    }
    if (covered != d.size()) return !fail(name + ": tokens do not cover the input");
    lf[256]++;
    // dynamic
    Codes c;
    std::vector<uint32_t> lf2 = lf, df2 = df;
    if (!build_codes(lf2, df2, &c, name)) return false;
    dfl::DynHeader h;
    dfl::plan_header(c.llen, c.dlen, &h);
    uint64_t bits = 0, want = h.bits;
    for (int s = 0; s < dfl::NLIT; ++s) want += (uint64_t)lf[s] * (c.llen[s] + (uint64_t)dfl::lit_extra_bits(s));
    for (int s = 0; s < dfl::NDIST; ++s) want += (uint64_t)df[s] * (c.dlen[s] + (uint64_t)dfl::dist_extra_bits(s));
    const Bytes dyn = emit(toks, c, &h, &bits);
    if (bits != want) return !fail(name + ": dynamic block size differs from the counted size");
    if (!inflate_equals(dyn, d, name + " (dynamic)")) return false;
    // fixed
    Codes f;
    uint32_t work[dfl::WORK];
    for (int s = 0; s < dfl::NLIT; ++s) f.llen[s] = (uint8_t)dfl::fixed_lit_len(s);
    for (int s = 0; s < dfl::NDIST; ++s) f.dlen[s] = 5;
    // the fixed code spans 288 and 32 symbols: assign over the full alphabets, keep the used part
    uint8_t l288[288], d32[32];
    uint16_t c288[288], c32[32];
    for (int s = 0; s < 288; ++s) l288[s] = (uint8_t)dfl::fixed_lit_len(s);
    for (int s = 0; s < 32; ++s) d32[s] = 5;
    dfl::canonical_codes(l288, 288, c288, work);
    dfl::canonical_codes(d32, 32, c32, work);
    memcpy(f.lcode, c288, sizeof f.lcode);
    memcpy(f.dcode, c32, sizeof f.dcode);
    const Bytes fix = emit(toks, f, nullptr, &bits);
    return inflate_equals(fix, d, name + " (fixed)");
}

bool all_pieces(const Bytes& d, const std::string& name) {
    for (size_t o = 0, k = 0; o < d.size(); o += 0xff00, ++k)
        if (!one_piece(Bytes(d.begin() + (long)o, d.begin() + (long)std::min(d.size(), o + 0xff00)), name + "[" + std::to_string(k) + "]"))
            return false;
    return true;
}

// code lengths straight from histograms
bool histogram(std::vector<uint32_t> f, int maxbits, const std::string& name, bool expect_limit) {
    const int n = (int)f.size();
    std::vector<uint8_t> len((size_t)n);
    std::vector<uint32_t> val((size_t)n), orig = f;
    std::vector<uint16_t> sym((size_t)n);
    uint32_t work[dfl::WORK];
    // the unlimited lengths are optimal
    std::vector<uint32_t> g = f;
    int used = 0;
    for (uint32_t x : g) used += x != 0;
    dfl::ensure_two(g.data(), n, used);
    const int m = dfl::sort_used(g.data(), n, val.data(), sym.data());
    std::vector<uint64_t> counts;
    for (int k = 0; k < m; ++k) {
        if (k && val[(size_t)k] < val[(size_t)k - 1]) return !fail(name + ": sort_used out of order");
        counts.push_back(val[(size_t)k]);
    }
    dfl::huffman_lengths(val.data(), m);
    uint64_t cost = 0, deepest = 0;
    for (int k = 0; k < m; ++k) { cost += counts[(size_t)k] * val[(size_t)k]; deepest = std::max<uint64_t>(deepest, val[(size_t)k]); }
    if (cost != huffman_cost(counts)) return !fail(name + ": huffman_lengths is not minimum-redundancy");
    if (expect_limit && deepest <= (uint64_t)maxbits) return !fail(name + ": histogram does not reach past the limit");
    dfl::build_lengths(f.data(), n, maxbits, len.data(), val.data(), sym.data(), work);
    if (!check_lengths(len.data(), orig.data(), n, maxbits, name)) return false;
    std::vector<uint16_t> code((size_t)n);
    dfl::canonical_codes(len.data(), n, code.data(), work);
    // prefix-free: no two codes of the canonical assignment collide on their low bits
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            if (!len[(size_t)a] || !len[(size_t)b]) continue;
            const int l = std::min(len[(size_t)a], len[(size_t)b]);
            if (((code[(size_t)a] ^ code[(size_t)b]) & ((1u << l) - 1)) == 0) return !fail(name + ": codes share a prefix");
        }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    bool ok = true;
    // symbol tables against RFC 1951 3.2.5
    {
        static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        static const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        for (int len = 3; len <= 258; ++len) {
            int eb, ev, want = 28;
            while (lbase[want] > len) --want;
            if (len == 258) want = 28; else if (want == 28) want = 27;
            const int s = dfl::len_sym(len, &eb, &ev);
            if (s != 257 + want || eb != lext[want] || ev != len - lbase[want]) ok = ok && !fail("len_sym(" + std::to_string(len) + ")");
        }
        for (int d = 1; d <= 32768; ++d) {
            int eb, ev, want = 29;
            while (dbase[want] > d) --want;
            const int s = dfl::dist_sym(d, &eb, &ev);
            if (s != want || eb != (want < 4 ? 0 : want / 2 - 1) || ev != d - dbase[want]) ok = ok && !fail("dist_sym(" + std::to_string(d) + ")");
        }
        static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int k = 0; k < 19; ++k)
            if (dfl::cl_order(k) != order[k]) ok = ok && !fail("cl_order");
    }
    // the crafted buffers of tests/test_gpu_bgzf.py
    const size_t sizes[] = {1, 2, 3, 4, 255, 256, 257, 0xfeff, 0xff00, 0xff01, 2 * 0xff00 + 3};
    for (size_t n : sizes) ok = ok && all_pieces(text_like(n, n), "text" + std::to_string(n));
    ok = ok && all_pieces(Bytes(0xff00, 0), "zeros");
    ok = ok && all_pieces(random_bytes(0xff00, 7), "random");
    {
        const Bytes seed = random_bytes(300, 11);
        Bytes b(seed);
        for (size_t L = 3; L <= 258; ++L) {
            b.insert(b.end(), seed.begin(), seed.begin() + (long)L);
            b.push_back((uint8_t)(seed[L] ^ 0x55));
        }
        ok = ok && all_pieces(b, "ladder");
    }
    for (size_t gap : {(size_t)32768, (size_t)32769}) {
        Bytes b = random_bytes(gap, 13);
        b.insert(b.end(), b.begin(), b.begin() + 20000);
        ok = ok && all_pieces(b, "window" + std::to_string(gap));
    }
    for (size_t tail = 0; tail <= 3; ++tail) {   // a match that ends on the last byte, then 0..3 loose bytes
        Bytes b = text_like(500, 17);
        b.insert(b.end(), b.begin() + 100, b.begin() + 160);
        for (size_t k = 0; k < tail; ++k) b.push_back((uint8_t)(0xf0 + k));
        ok = ok && all_pieces(b, "tail" + std::to_string(tail));
    }
    // histograms that force the length limit, and the degenerate trees
    {
        std::vector<uint32_t> fib(dfl::NLIT, 0);
        uint32_t a = 1, b = 1;
        for (int s = 0; s < 40; ++s) { fib[(size_t)s * 7] = a; const uint32_t c = a + b; a = b; b = c; }
        ok = ok && histogram(fib, 15, "fibonacci lit", true);
        std::vector<uint32_t> fd(dfl::NDIST, 0);
        a = b = 1;
        for (int s = 0; s < 30; ++s) { fd[(size_t)s] = a; const uint32_t c = a + b; a = b; b = c; }
        ok = ok && histogram(fd, 15, "fibonacci dist", true);
        std::vector<uint32_t> fc(dfl::NCL, 0);
        a = b = 1;
        for (int s = 0; s < 19; ++s) { fc[(size_t)s] = a; const uint32_t c = a + b; a = b; b = c; }
        ok = ok && histogram(fc, 7, "fibonacci code-length", true);
        std::vector<uint32_t> one(dfl::NLIT, 0);
        one[256] = 1;
        ok = ok && histogram(one, 15, "single symbol", false);
        ok = ok && histogram(std::vector<uint32_t>(dfl::NDIST, 0), 15, "no distance symbol", false);
        ok = ok && histogram(std::vector<uint32_t>(dfl::NLIT, 1), 15, "flat", false);
        Rng r(23);
        for (int t = 0; t < 50 && ok; ++t) {
            std::vector<uint32_t> f(dfl::NLIT, 0);
            for (auto& x : f) x = r.next() % 3 ? r.next() % (1u << (r.next() % 16)) : 0;
            ok = ok && histogram(f, 15, "random histogram " + std::to_string(t), false);
        }
    }
    // a block of one repeated literal (a single distinct symbol besides end-of-block) and one with no match
    ok = ok && all_pieces(Bytes(2, 'A'), "two equal bytes");
    ok = ok && all_pieces(Bytes{'a', 'b', 'c', 'd', 'e', 'f', 'g'}, "no match");
    for (int i = 1; i < argc && ok; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) return fail(std::string("cannot open ") + argv[i]);
        Bytes b;
        uint8_t buf[1 << 16];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + k);
        fclose(f);
        ok = ok && all_pieces(b, argv[i]);
    }
    if (!ok) return 1;
    printf("ok\n");
    return 0;
}
