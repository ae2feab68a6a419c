// Stand-alone driver for csrc/intern_core.h under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_intern_core_host.py builds and runs it; nothing here is loaded into Python).
// Input file: cases, each
//   u32 len, len record bytes, i32 mode, u32 dlen, dlen delimiter bytes, u8 want
//   want 1: then 3 x {u32 off, u32 len, u8 none}, u8 flags (the expectation); want 0: must be refused.
// Every record is copied into a heap block of exactly its size, so a read past it is an ASan report.
// The key bytes of an accepted record are read through hash_bytes as the kernel reads them.
// Prints "ok <cases> <accepted>"; any mismatch prints to stderr and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../consensuscruncher_amd/csrc/intern_core.h"

static const uint8_t* g_p;
static const uint8_t* g_end;
template <class T>
static T take() {
    T v;
    if (g_p + sizeof(T) > g_end) { fprintf(stderr, "input cut short\n"); exit(1); }
    memcpy(&v, g_p, sizeof(T));
    g_p += sizeof(T);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
    fclose(f);
    g_p = in.data();
    g_end = in.data() + in.size();
    long cases = 0, accepted = 0;
    uint64_t sink = 0;
    while (g_p < g_end) {
        const uint32_t len = take<uint32_t>();
        if (g_p + len > g_end) { fprintf(stderr, "input cut short\n"); return 1; }
        uint8_t* rec = (uint8_t*)malloc(len ? len : 1);
        memcpy(rec, g_p, len);
        g_p += len;
        const int32_t mode = take<int32_t>();
        const uint32_t dlen = take<uint32_t>();
        itn::Delim d{};
        if (dlen > (uint32_t)itn::DELIM_MAX) { fprintf(stderr, "case %ld: delimiter too long\n", cases); return 1; }
        memcpy(d.b, g_p, dlen);
        g_p += dlen;
        d.len = (int32_t)dlen;
        const uint8_t want = take<uint8_t>();
        upk::Rec r;
        itn::Key key[3] = {};
        bool ok = upk::parse(rec, len, r);
        if (ok) {
            key[0] = itn::barcode_key(rec, r, mode, d);
            key[1] = itn::cigar_key(rec, r);
            key[2] = itn::rg_key(rec, r);
            ok = !key[2].refuse;
        }
        if (ok) {
            ++accepted;
            for (int k = 0; k < 3; ++k) {
                if (key[k].none) continue;
                if ((uint64_t)key[k].off + key[k].len > 4ull + (uint64_t)(uint32_t)r.bs) {
                    fprintf(stderr, "case %ld: table %d key outside the record\n", cases, k);
                    return 1;
                }
                sink ^= itn::hash_bytes(rec + key[k].off, key[k].len, 0x1234 + k);
            }
        }
        if (want) {
            uint8_t flags = 0;
            struct { uint32_t off, len; uint8_t none; } e[3];
            for (int k = 0; k < 3; ++k) { e[k].off = take<uint32_t>(); e[k].len = take<uint32_t>(); e[k].none = take<uint8_t>(); }
            flags = take<uint8_t>();
            if (!ok) { fprintf(stderr, "case %ld: refused, expected keys\n", cases); return 1; }
            for (int k = 0; k < 3; ++k) {
                const bool same = e[k].none ? key[k].none : (!key[k].none && key[k].off == e[k].off && key[k].len == e[k].len);
                if (!same) {
                    fprintf(stderr, "case %ld: table %d: got {%u, %u, %d}, expected {%u, %u, %d}\n", cases, k, key[k].off,
                            key[k].len, (int)key[k].none, e[k].off, e[k].len, (int)e[k].none);
                    return 1;
                }
            }
            if ((uint8_t)(key[0].flags | key[2].flags) != flags) {
                fprintf(stderr, "case %ld: flags %d, expected %d\n", cases, key[0].flags | key[2].flags, (int)flags);
                return 1;
            }
        } else if (ok) {
            fprintf(stderr, "case %ld: accepted, expected a refusal\n", cases);
            return 1;
        }
        free(rec);
        ++cases;
    }
    printf("ok %ld %ld %llu\n", cases, accepted, (unsigned long long)(sink & 1));
    return 0;
}
