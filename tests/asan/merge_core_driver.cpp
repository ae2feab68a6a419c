// csrc/merge_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: the key against a
// straight restatement, every refusal code on heap blocks of exactly the source's size (a byte read
// past an accepted range is reported), lower / upper on the edge arrays, and the place rule
// (mrg::merge_host, as the device runs it) on 2, 3 and 8 small sources against std::stable_sort of
// the concatenation.  Prints "ok <checks>" and exits 0 when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../consensuscruncher_amd/csrc/merge_core.h"

namespace {

int g_checks = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        ++g_checks;                                                    \
        if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

void put32(std::vector<uint8_t>& v, uint32_t x) {
    for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i)));
}
// one raw record: block_size, then a core with the given fields, a name of `nl` bytes (NUL included)
std::vector<uint8_t> record(int32_t tid, int32_t pos, uint16_t flag, uint32_t nl, uint8_t fill) {
    std::vector<uint8_t> r;
    put32(r, 32u + nl);
    put32(r, (uint32_t)tid);
    put32(r, (uint32_t)pos);
    put32(r, nl);                     // l_read_name | mapq << 8 | bin << 16
    put32(r, (uint32_t)flag << 16);   // n_cigar_op | flag << 16
    put32(r, 0);
    put32(r, (uint32_t)-1);
    put32(r, (uint32_t)-1);
    put32(r, 0);
    for (uint32_t i = 0; i < nl; ++i) r.push_back(i + 1 < nl ? fill : 0);
    return r;
}
// the restatement: ccio.cpp's coord_key, field by field
uint64_t key_of(int32_t tid, int32_t pos, uint16_t flag) {
    const uint64_t t = (uint32_t)tid, p = (uint32_t)(pos + 1);
    return (t << 32) | (p << 1) | ((flag >> 4) & 1u);
}
// the bytes in a heap block of exactly their size
std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size());
    return p;
}

int keys() {
    const int32_t tids[] = {-1, 0, 7}, poss[] = {-1, 0, 2147483646};
    const uint16_t flags[] = {0, 16, 0xffef, 0xffff};
    for (int32_t tid : tids)
        for (int32_t pos : poss)
            for (uint16_t fl : flags) {
                const std::vector<uint8_t> r = record(tid, pos, fl, 3, 'a');
                const auto blk = exact(r);
                uint32_t size = 0;
                uint64_t k = 0;
                CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, r.size(), 0, &size, &k) == 0);
                CHECK(size == r.size());
                CHECK(k == key_of(tid, pos, fl));
                CHECK(k == mrg::key(asmb::ByteFetch::fetch(blk.get(), 4, 16)));
            }
    CHECK(key_of(-1, 0, 0) > key_of(7, 2147483646, 16));   // tid -1 sorts last
    CHECK(key_of(3, -1, 16) < key_of(3, 0, 0));            // pos -1 sorts first
    return 0;
}

int refusals() {
    const std::vector<uint8_t> r = record(1, 5, 0, 4, 'b');
    uint32_t size = 0;
    uint64_t k = 0;
    {
        const auto blk = exact(r);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, r.size(), r.size(), &size, &k) == mrg::ME_OFF);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, r.size(), r.size() + 100, &size, &k) == mrg::ME_OFF);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, r.size(), r.size() - 3, &size, &k) == mrg::ME_SHORT);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, r.size(), 0, &size, &k) == 0);
    }
    {   // block_size 31, and 0xffffffff
        std::vector<uint8_t> b = r;
        b[0] = 31;
        const auto blk = exact(b);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, b.size(), 0, &size, &k) == mrg::ME_BS);
        b[0] = b[1] = b[2] = b[3] = 0xff;
        const auto blk2 = exact(b);
        CHECK(mrg::record<asmb::ByteFetch>(blk2.get(), 0, b.size(), 0, &size, &k) == mrg::ME_PAST);
    }
    {   // one byte short of the record; and a block that ends inside the core
        std::vector<uint8_t> b(r.begin(), r.end() - 1);
        const auto blk = exact(b);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 0, b.size(), 0, &size, &k) == mrg::ME_PAST);
        std::vector<uint8_t> c(r.begin(), r.begin() + 10);
        const auto blk2 = exact(c);
        CHECK(mrg::record<asmb::ByteFetch>(blk2.get(), 0, c.size(), 0, &size, &k) == mrg::ME_PAST);
    }
    {   // a shifted source: the record at shift + rel, the block ends with it
        std::vector<uint8_t> b(7, 0xee);
        b.insert(b.end(), r.begin(), r.end());
        const auto blk = exact(b);
        CHECK(mrg::record<asmb::ByteFetch>(blk.get(), 7, r.size(), 0, &size, &k) == 0);
        CHECK(size == r.size() && k == key_of(1, 5, 0));
    }
    return 0;
}

int searches() {
    const uint64_t none = 0;
    CHECK(mrg::lower(&none, 0, 0, 5) == 0 && mrg::upper(&none, 0, 0, 5) == 0);
    const auto one = std::unique_ptr<uint64_t[]>(new uint64_t[1]{10});
    CHECK(mrg::lower(one.get(), 0, 1, 9) == 0 && mrg::upper(one.get(), 0, 1, 9) == 0);
    CHECK(mrg::lower(one.get(), 0, 1, 10) == 0 && mrg::upper(one.get(), 0, 1, 10) == 1);
    CHECK(mrg::lower(one.get(), 0, 1, 11) == 1 && mrg::upper(one.get(), 0, 1, 11) == 1);
    const auto eq = std::unique_ptr<uint64_t[]>(new uint64_t[5]{4, 4, 4, 4, 4});
    CHECK(mrg::lower(eq.get(), 0, 5, 4) == 0 && mrg::upper(eq.get(), 0, 5, 4) == 5);
    CHECK(mrg::lower(eq.get(), 0, 5, 3) == 0 && mrg::upper(eq.get(), 0, 5, 5) == 5);
    CHECK(mrg::lower(eq.get(), 2, 4, 4) == 2 && mrg::upper(eq.get(), 2, 4, 4) == 4);
    const auto inc = std::unique_ptr<uint64_t[]>(new uint64_t[7]{1, 3, 5, 7, 9, 11, ~0ull});
    for (int64_t i = 0; i < 7; ++i) {
        CHECK(mrg::lower(inc.get(), 0, 7, inc[i]) == i && mrg::upper(inc.get(), 0, 7, inc[i]) == i + 1);
        if (i < 6) CHECK(mrg::lower(inc.get(), 0, 7, inc[i] + 1) == i + 1 && mrg::upper(inc.get(), 0, 7, inc[i] + 1) == i + 1);
    }
    CHECK(mrg::lower(inc.get(), 0, 7, 0) == 0 && mrg::upper(inc.get(), 0, 7, 0) == 0);
    return 0;
}

// nsrc sorted sources with many ties across them, merged by the core and by std::stable_sort
int places(int nsrc, uint32_t seed) {
    std::vector<std::vector<uint8_t>> streams((size_t)nsrc);
    std::vector<std::vector<uint64_t>> offs((size_t)nsrc);
    struct Item { uint64_t key; int s; int64_t i; const uint8_t* p; uint32_t size; };
    std::vector<std::vector<Item>> items((size_t)nsrc);
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int s = 0; s < nsrc; ++s) {
        const int cnt = s == 1 ? 0 : (int)(rnd() % 9) + (s == 0 ? 1 : 0);   // (source 1 is empty)
        std::vector<std::pair<uint64_t, std::vector<uint8_t>>> recs;
        for (int i = 0; i < cnt; ++i) {
            const int32_t tid = (rnd() % 5 == 0) ? -1 : (int32_t)(rnd() % 2), pos = (int32_t)(rnd() % 4) - 1;
            const uint16_t fl = (rnd() & 1) ? 16 : 0;
            recs.push_back({key_of(tid, pos, fl), record(tid, pos, fl, 1 + rnd() % 7, (uint8_t)('a' + s))});
        }
        std::stable_sort(recs.begin(), recs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (auto& r : recs) {
            offs[(size_t)s].push_back(streams[(size_t)s].size());
            streams[(size_t)s].insert(streams[(size_t)s].end(), r.second.begin(), r.second.end());
        }
    }
    std::vector<std::unique_ptr<uint8_t[]>> blocks;
    std::vector<asmb::Src> src((size_t)nsrc);
    std::vector<Item> all;
    for (int s = 0; s < nsrc; ++s) {
        blocks.push_back(exact(streams[(size_t)s]));
        src[(size_t)s] = asmb::Src{blocks.back().get(), 0, streams[(size_t)s].size(), offs[(size_t)s].data(),
                                   (int64_t)offs[(size_t)s].size()};
        for (size_t i = 0; i < offs[(size_t)s].size(); ++i) {
            const uint8_t* p = blocks.back().get() + offs[(size_t)s][i];
            uint32_t bs;
            memcpy(&bs, p, 4);
            uint32_t size = 0;
            uint64_t k = 0;
            CHECK(mrg::record<asmb::ByteFetch>(src[(size_t)s].base, 0, src[(size_t)s].bytes, offs[(size_t)s][i], &size, &k) == 0);
            all.push_back(Item{k, s, (int64_t)i, p, bs + 4});
        }
    }
    const uint8_t header[5] = {'B', 'A', 'M', 1, 9};
    std::vector<uint8_t> out;
    std::vector<uint64_t> at;
    std::vector<uint32_t> org;
    int bad_src = -1;
    int64_t bad_rec = -1;
    CHECK(mrg::merge_host(header, 5, src.data(), nsrc, out, at, org, &bad_src, &bad_rec) == 0);
    std::vector<size_t> order(all.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return all[a].key < all[b].key; });
    CHECK(org.size() == all.size() && at.size() == all.size() + 1 && at[0] == 5);
    CHECK(memcmp(out.data(), header, 5) == 0);
    for (size_t o = 0; o < order.size(); ++o) {
        const Item& it = all[order[o]];
        CHECK(org[o] == order[o]);
        CHECK(at[o + 1] - at[o] == it.size);
        CHECK(memcmp(out.data() + at[o], it.p, it.size) == 0);
    }
    CHECK(at.back() == out.size());
    return 0;
}

int order_refused() {
    std::vector<uint8_t> st;
    std::vector<uint64_t> off;
    for (int32_t pos : {5, 9, 8}) {
        const std::vector<uint8_t> r = record(0, pos, 0, 2, 'x');
        off.push_back(st.size());
        st.insert(st.end(), r.begin(), r.end());
    }
    const auto blk = exact(st);
    const asmb::Src src{blk.get(), 0, st.size(), off.data(), 3};
    std::vector<uint8_t> out;
    std::vector<uint64_t> at;
    std::vector<uint32_t> org;
    int bad_src = -1;
    int64_t bad_rec = -1;
    CHECK(mrg::merge_host(nullptr, 0, &src, 1, out, at, org, &bad_src, &bad_rec) == mrg::ME_ORDER);
    CHECK(bad_src == 0 && bad_rec == 2);
    return 0;
}

}  // namespace

int main() {
    if (keys() || refusals() || searches() || order_refused()) return 1;
    for (uint32_t seed = 1; seed <= 20; ++seed)
        if (places(2, seed) || places(3, seed * 7) || places(8, seed * 13)) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
