// csrc/crc_core.h on the host, under AddressSanitizer + UndefinedBehaviorSanitizer.  A stand-alone
// program: tests/test_crc_core_host.py builds it, writes a file of cases and runs it.
//
// The case file is a run of records, each led by a kind byte:
//   kind 0: u32 pad (0..15), u32 len, len bytes, u32 crc (zlib's CRC32 of the bytes).  Checked: the
//           bytewise register, identity (1) with pads 0..15 of zeros in front (for len <= 4096),
//           identity (2), and the kernel's per-lane rule run lane by lane: 256 lanes over a heap block
//           of exactly the aligned span (nwords * 16 bytes, the segment at byte `pad`, every other
//           byte 0xa5), so the sanitizer judges the rule's reads and the junk judges its masks;
//   kind 1: u32 len, len bytes, u32 crc, then for every split s = 0..len: u32 crc of [0, s), u32 crc of
//           [s, len) (zlib's).  Checked: combine at every split.
// Before the cases the generated tables are checked against the bit-by-bit definition.
// Prints "ok <cases>" and exits 0 when everything holds; zlib's values are the only judge.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../consensuscruncher_amd/csrc/crc_core.h"

namespace {

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

// the definition, written here once more: one bit at a time
uint32_t bit_byte(uint32_t r, uint8_t c) {
    r ^= c;
    for (int k = 0; k < 8; ++k) r = (r & 1) ? 0xedb88320u ^ (r >> 1) : r >> 1;
    return r;
}

struct HeapSrc {   // the aligned span in a block of exactly its size
    const uint8_t* p;
    crc::W16 word16(uint32_t w) const {
        crc::W16 x;
        for (int k = 0; k < 4; ++k) x.v[k] = rd32(p + 16 * (size_t)w + 4 * k);
        return x;
    }
};

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

int check_tables(const crc::Tables& T) {
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t r = bit_byte(0, (uint8_t)b);
        for (int k = 0; k < crc::SLICES; ++k) {
            if (T.slice[256 * k + b] != r) FAIL("slice %d entry %u", k, b);
            r = bit_byte(r, 0);
        }
        for (int k = 0; k < 4; ++k) {
            uint32_t s = b << (8 * k);
            for (uint32_t i = 0; i < crc::STRIDE_BYTES; ++i) s = bit_byte(s, 0);
            if (T.stride[256 * k + b] != s) FAIL("stride %d entry %u", k, b);
        }
    }
    uint32_t r = 0x12345678u;
    for (int i = 0; i < 1000; ++i) {   // the steps against the bit-by-bit register
        const uint32_t w = r * 2654435761u + (uint32_t)i;
        uint32_t want = r;
        for (int k = 0; k < 4; ++k) want = bit_byte(want, (uint8_t)(w >> (8 * k)));
        if (crc::word_step(T, r, w) != want) FAIL("word_step %d", i);
        if (crc::byte_step(T, r, w & 0xff) != bit_byte(r, (uint8_t)w)) FAIL("byte_step %d", i);
        uint32_t z = r;
        for (uint32_t k = 0; k < crc::STRIDE_BYTES; ++k) z = bit_byte(z, 0);
        if (crc::stride_step(T, r) != z) FAIL("stride_step %d", i);
        const uint32_t nz = (uint32_t)i * 7;
        z = r;
        for (uint32_t k = 0; k < nz; ++k) z = bit_byte(z, 0);
        if (crc::advance(r, nz) != z) FAIL("advance by %u", nz);
        if (crc::mulmod(r, crc::ONE) != r || crc::mulmod(crc::ONE, r) != r) FAIL("mulmod by one");
        if (crc::mulmod(r, w) != crc::mulmod(w, r)) FAIL("mulmod commutes");
        r = want;
    }
    if (crc::xpow8n(0) != crc::ONE || crc::xpow8n(1) != 0x00800000u) FAIL("xpow8n");
    return 0;
}

uint32_t raw0(const crc::Tables& T, const uint8_t* p, size_t n, uint32_t r = 0) {
    for (size_t i = 0; i < n; ++i) r = crc::byte_step(T, r, p[i]);
    return r;
}

int check_case(const crc::Tables& T, long id, uint32_t pad, const uint8_t* bytes, uint32_t len, uint32_t want) {
    if (pad > 15) FAIL("case %ld: pad %u", id, pad);
    const uint32_t r0 = raw0(T, bytes, len);
    if ((raw0(T, bytes, len, 0xffffffffu) ^ 0xffffffffu) != want) FAIL("case %ld: the bytewise register", id);
    if (crc::finish(r0, len) != want) FAIL("case %ld: identity (2)", id);
    if (len <= 4096)
        for (uint32_t z = 0; z < 16; ++z) {   // identity (1)
            uint8_t* m = (uint8_t*)malloc(z + len ? z + len : 1);
            memset(m, 0, z);
            if (len) memcpy(m + z, bytes, len);
            const uint32_t rz = raw0(T, m, z + len);
            free(m);
            if (rz != r0) FAIL("case %ld: identity (1) with %u zero bytes", id, z);
        }
    // the per-lane rule, lane by lane, over a block of exactly the aligned span
    const uint32_t nw = crc::nwords(pad, len);
    if (nw != (len ? (pad + len + 15) / 16 : 0)) FAIL("case %ld: nwords", id);
    uint8_t* span = (uint8_t*)malloc(nw ? (size_t)nw * 16 : 1);
    memset(span, 0xa5, nw ? (size_t)nw * 16 : 1);
    if (len) memcpy(span + pad, bytes, len);
    uint32_t x = 0;
    for (uint32_t t = 0; t < crc::LANES; ++t) x ^= crc::lane(T, HeapSrc{span}, pad, len, t);
    free(span);
    if (crc::finish(x, len) != want) FAIL("case %ld: the lane rule (pad %u, len %u)", id, pad, len);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    std::vector<uint8_t> file;
    if (!read_all(argv[1], file)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t* slice = (uint32_t*)malloc(crc::SLICES * 256 * sizeof(uint32_t));
    uint32_t* stride = (uint32_t*)malloc(4 * 256 * sizeof(uint32_t));
    crc::make_tables(slice, stride);
    const crc::Tables T = {slice, stride};
    int rc = check_tables(T);
    size_t off = 0;
    long cases = 0;
    while (!rc && off < file.size()) {
        const int kind = file[off++];
        if (kind == 0) {
            if (off + 8 > file.size()) { fprintf(stderr, "case %ld: truncated record\n", cases); rc = 2; break; }
            const uint32_t pad = rd32(&file[off]), len = rd32(&file[off + 4]);
            off += 8;
            if (off + (size_t)len + 4 > file.size()) { fprintf(stderr, "case %ld: truncated record\n", cases); rc = 2; break; }
            uint8_t* bytes = (uint8_t*)malloc(len ? len : 1);
            if (len) memcpy(bytes, &file[off], len);
            rc = check_case(T, cases, pad, bytes, len, rd32(&file[off + len]));
            free(bytes);
            off += (size_t)len + 4;
        } else if (kind == 1) {
            if (off + 4 > file.size()) { fprintf(stderr, "case %ld: truncated record\n", cases); rc = 2; break; }
            const uint32_t len = rd32(&file[off]);
            off += 4;
            if (off + (size_t)len + 4 + 8 * ((size_t)len + 1) > file.size()) {
                fprintf(stderr, "case %ld: truncated record\n", cases);
                rc = 2;
                break;
            }
            const uint32_t whole = rd32(&file[off + len]);
            const uint8_t* sp = &file[off + len + 4];
            for (uint32_t s = 0; s <= len && !rc; ++s)
                if (crc::combine(rd32(sp + 8 * (size_t)s), rd32(sp + 8 * (size_t)s + 4), len - s) != whole) {
                    fprintf(stderr, "case %ld: combine at split %u of %u\n", cases, s, len);
                    rc = 1;
                }
            off += (size_t)len + 4 + 8 * ((size_t)len + 1);
        } else {
            fprintf(stderr, "case %ld: unknown kind %d\n", cases, kind);
            rc = 2;
        }
        ++cases;
    }
    free(slice);
    free(stride);
    if (rc) return rc;
    printf("ok %ld\n", cases);
    return 0;
}
