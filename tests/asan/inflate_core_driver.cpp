// csrc/inflate_core.h on the host, under AddressSanitizer + UndefinedBehaviorSanitizer.  A stand-alone
// program: tests/test_inflate_core_host.py builds it, writes a file of cases and runs it.
//
// The case file is a run of records:
//   u32 clen, u32 ulen, u8 want, clen bytes of raw DEFLATE, then ulen expected bytes when want >= 1.
//   want 2: the member must inflate to exactly the expected bytes;
//   want 1: it may be refused; if it is accepted, the bytes must be the expected ones;
//   want 0: it must be refused.
// Every buffer is a heap block of exactly the size the kernel contract names (clen bytes in, ulen
// bytes out, the tables' own sizes), so the sanitizer judges every bounds claim of the core.
// Prints "ok <cases> <accepted>" and exits 0 when every case holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../consensuscruncher_amd/csrc/inflate_core.h"

namespace {

struct Heap {   // the decoder's tables, each in a block of its own
    ifl::Huff<ifl::NLIT>* L = (ifl::Huff<ifl::NLIT>*)malloc(sizeof(ifl::Huff<ifl::NLIT>));
    ifl::Huff<ifl::NDIST>* D = (ifl::Huff<ifl::NDIST>*)malloc(sizeof(ifl::Huff<ifl::NDIST>));
    uint8_t* lens = (uint8_t*)malloc(ifl::LENS);
    uint16_t* offs = (uint16_t*)malloc((ifl::MAXBITS + 1) * sizeof(uint16_t));
    ~Heap() { free(L); free(D); free(lens); free(offs); }
    ifl::Tables tables() const { return ifl::Tables{L, D, lens, offs}; }
};

bool read_all(const char* path, std::vector<uint8_t>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    std::vector<uint8_t> file;
    if (!read_all(argv[1], file)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Heap heap;
    size_t off = 0;
    long cases = 0, accepted = 0;
    while (off < file.size()) {
        if (off + 9 > file.size()) { fprintf(stderr, "case %ld: truncated record\n", cases); return 2; }
        const uint32_t clen = rd32(&file[off]), ulen = rd32(&file[off + 4]);
        const int want = file[off + 8];
        off += 9;
        const size_t need = (size_t)clen + (want >= 1 ? ulen : 0);
        if (off + need > file.size()) { fprintf(stderr, "case %ld: truncated record\n", cases); return 2; }
        uint8_t* in = (uint8_t*)malloc(clen ? clen : 1);
        uint8_t* out = (uint8_t*)malloc(ulen ? ulen : 1);
        if (clen) memcpy(in, &file[off], clen);
        memset(out, 0xa5, ulen ? ulen : 1);
        const uint8_t* expect = want >= 1 ? &file[off + clen] : nullptr;
        // the tables start each case dirty: nothing may depend on what an earlier member left
        memset(heap.L, 0xff, sizeof *heap.L);
        memset(heap.D, 0xff, sizeof *heap.D);
        memset(heap.lens, 0xff, ifl::LENS);
        const bool ok = ifl::inflate_flat(in, clen, out, ulen, heap.tables());
        int bad = 0;
        if (ok) {
            ++accepted;
            if (want == 0) { fprintf(stderr, "case %ld: accepted, must be refused\n", cases); bad = 1; }
            else if (ulen && memcmp(out, expect, ulen) != 0) { fprintf(stderr, "case %ld: wrong bytes\n", cases); bad = 1; }
        } else if (want == 2) {
            fprintf(stderr, "case %ld: refused, must inflate (clen %u ulen %u)\n", cases, clen, ulen);
            bad = 1;
        }
        free(in);
        free(out);
        if (bad) return 1;
        off += need;
        ++cases;
    }
    printf("ok %ld %ld\n", cases, accepted);
    return 0;
}
