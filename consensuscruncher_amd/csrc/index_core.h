// What the BAI needs of one BAM record, read from the uncompressed stream where it lies: tid, pos,
// block_size, the reference length and the unmapped bit.  Plain C++ that compiles in the HIP kernel
// (bam_index.hip.inc: k_index_fields), in libccio (the index's accumulator takes its bins from here)
// and with a host compiler alone (tests/asan/index_core_driver.cpp runs it under sanitizers), so
// the host walk, the fields-driven index and the kernel execute the same text.
//
// The contract (a bad offset must never fault a device other people share):
//   * field() reads nothing before [a, next) was checked against the stream's size, reads the
//     block_size word only when the span holds one, the 32 core bytes only when block_size says
//     they are there and equals the span, and the cigar only after 32 + l_read_name + 4 * n_cigar_op
//     fits block_size; it is the only function that may run on unchecked offsets;
//   * every byte comes through s.fetch(a, valid) with [a, a + valid) inside [at[i], at[i + 1]):
//     16 bytes at any stream offset, bytes from `valid` (1..16) on zero.
#ifndef CC_INDEX_CORE_H
#define CC_INDEX_CORE_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define IDX_HD __host__ __device__ inline
#else
#define IDX_HD inline
#endif

namespace idx {

struct W16 { uint32_t w[4]; };

// cc_index_field (include/consensuscruncher_amd.h), field for field
struct Field {
    int32_t tid, pos;
    uint32_t block_size;
    uint32_t rl;   // bits 0..30 the reference length, bit 31 the record's flag & 4
};
static_assert(sizeof(Field) == 16, "cc_index_field layout");

constexpr uint32_t RL_MAX = 0x7fffffffu;   // the reference length saturates here
constexpr uint32_t UNMAPPED = 0x80000000u;

// refusals (the first bad record's bits are reported)
enum : uint32_t {
    IE_SPAN = 1u,    // at[i] + 4 + block_size != at[i + 1], or the offsets out of order or past the stream
    IE_SHORT = 2u,   // block_size < 32
    IE_CIGAR = 4u,   // 32 + l_read_name + 4 * n_cigar_op > block_size
};

IDX_HD const char* refusal(uint32_t bits) {
    if (bits & IE_SHORT) return "block_size under 32";
    if (bits & IE_SPAN) return "at[i] + 4 + block_size is not at[i + 1] (or the offsets leave the stream)";
    return "32 + l_read_name + 4 * n_cigar_op is more than block_size";
}

// M, D, N, = and X consume the reference
IDX_HD bool ref_op(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

IDX_HD int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// the interval a record occupies in the index: beg = max(pos, 0), end = beg + (rl ? rl : 1)
IDX_HD void interval(int32_t pos, uint32_t rl, int64_t* beg, int64_t* end) {
    *beg = pos < 0 ? 0 : pos;
    *end = *beg + (rl ? (int64_t)rl : 1);
}

// The record whose block_size word is the stream's byte a and whose successor starts at byte next,
// in a stream of `total` bytes.  0 and o filled in, or the refusal's bits (o is then meaningless).
template <class Src>
IDX_HD uint32_t field(const Src& s, uint64_t a, uint64_t next, uint64_t total, Field& o) {
    if (next > total || a > next || next - a < 4) return IE_SPAN;
    const uint32_t bs = s.fetch(a, 4u).w[0];
    if ((int32_t)bs < 32) return IE_SHORT;
    if (next - a != 4ull + bs) return IE_SPAN;
    const W16 c = s.fetch(a + 4, 16u);   // tid, pos, l_read_name | mapq | bin, n_cigar_op | flag
    const uint32_t lrn = c.w[2] & 0xffu, ncig = c.w[3] & 0xffffu, flag = c.w[3] >> 16;
    if (32ull + lrn + 4ull * ncig > bs) return IE_CIGAR;
    o.tid = (int32_t)c.w[0];
    o.pos = (int32_t)c.w[1];
    o.block_size = bs;
    uint64_t rl = 0;   // at most 65535 ops of under 2^28 each
    if (!(flag & 4u)) {
        const uint64_t cg = a + 36 + lrn;
        for (uint32_t k = 0; k < ncig; k += 4) {
            const uint32_t ops = ncig - k < 4u ? ncig - k : 4u;
            const W16 v = s.fetch(cg + 4ull * k, 4u * ops);
            for (uint32_t j = 0; j < 4; ++j)
                if (j < ops && ref_op(v.w[j] & 0xfu)) rl += v.w[j] >> 4;
        }
    }
    o.rl = (rl > RL_MAX ? RL_MAX : (uint32_t)rl) | ((flag & 4u) ? UNMAPPED : 0u);
    return 0;
}

// the plain byte-at-a-time source (host code, and the reference the device's aligned loads are
// tested against): p[0 .. n) is the stream
struct HostSrc {
    const uint8_t* p;
    W16 fetch(uint64_t a, uint32_t valid) const {   // (host only, little-endian like the rest of libccio)
        W16 o{{0u, 0u, 0u, 0u}};
        memcpy(o.w, p + a, valid);
        return o;
    }
};

}  // namespace idx

#endif
