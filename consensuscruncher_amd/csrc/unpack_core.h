// The per-record parts of the BAM record unpacker: the field parser with its refusals, the payload
// and qname slot sizes, the record digest and the slot layout.  Plain C++ that compiles in the HIP
// kernels (cc_engine.hip: k_unpack_sizes, k_unpack_copy), in libccio (ccio.cpp: ccio_bam_decode,
// ccio_bam_decode_ids) and with a host compiler alone (tests/asan/unpack_core_driver.cpp runs it
// under sanitizers), so all of them execute the same text.
//
// The contract (a corrupt record must never fault a device other people share):
//   * parse() reads only bytes of [rec, rec + min(avail, 4 + bs)), one byte at a time (records start
//     at any alignment), and refuses a record whose lengths do not fit its block_size or the stream;
//   * a parsed record's cigar, sequence, quality and aux offsets all lie inside 4 + bs;
//   * rec_digest reads the record only through Src::word(i, valid) with i + valid <= bs;
//   * write_slots reads the record only through Src::bytes16(i, valid) / bytes8(i, valid) with
//     i + valid inside the parsed fields, and writes whole slots (every padding byte) through
//     Sink::pay16(chunk, words) / Sink::qn8(chunk, words).
#ifndef CC_UNPACK_CORE_H
#define CC_UNPACK_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define UPK_HD __host__ __device__ inline
#else
#define UPK_HD inline
#endif

namespace upk {

constexpr uint8_t RF_QUAL_MISSING = 2;   // CC_RF_QUAL_MISSING (include/consensuscruncher_amd.h)

// payload slot of one record: [qual | pad16][seq nibbles | pad16], the whole slot padded to
// 128 B (one HBM/L2 line) so a read of L = 150 touches two lines, not three or four
UPK_HD uint64_t align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }
UPK_HD uint64_t pay_slot(int32_t lseq) {
    return (align16((uint64_t)lseq) + align16(((uint64_t)lseq + 1) / 2) + 127) & ~(uint64_t)127;
}
// qname slot: l_read_name (the NUL included) in 8-byte words
UPK_HD uint32_t qn_slot(uint32_t l_read_name) { return (l_read_name + 7u) & ~7u; }

struct Rec {
    int32_t bs, tid, pos, l_read_name, mapq, n_cigar, flag, lseq, mtid, mpos, tlen;
    int32_t qn_len;    // strnlen of the read name within l_read_name
    int32_t qlen;      // infer_query_length: ops M, I, S, =, X summed; -1 without a cigar
    uint32_t cig_off, seq_off, qual_off, aux_off;   // from rec (the block_size word is bytes 0..3)
    uint8_t rflags;    // RF_QUAL_MISSING or 0
};

UPK_HD uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
UPK_HD uint32_t ld32(const uint8_t* p) { return ld16(p) | (ld16(p + 2) << 16); }

// One record at rec (block_size first) with avail bytes from rec to the end of the stream.
// False: refused, nothing of o is meaningful.
UPK_HD bool parse(const uint8_t* rec, uint64_t avail, Rec& o) {
    if (avail < 4) return false;
    const int32_t bs = (int32_t)ld32(rec);
    if (bs < 32 || 4 + (uint64_t)(uint32_t)bs > avail) return false;
    const uint8_t* r = rec + 4;
    o.bs = bs;
    o.tid = (int32_t)ld32(r + 0);
    o.pos = (int32_t)ld32(r + 4);
    o.l_read_name = r[8];
    o.mapq = r[9];
    o.n_cigar = (int32_t)ld16(r + 12);
    o.flag = (int32_t)ld16(r + 14);
    o.lseq = (int32_t)ld32(r + 16);
    o.mtid = (int32_t)ld32(r + 20);
    o.mpos = (int32_t)ld32(r + 24);
    o.tlen = (int32_t)ld32(r + 28);
    if (o.lseq < 0) return false;
    const uint64_t need = 32ull + (uint64_t)o.l_read_name + 4ull * (uint64_t)o.n_cigar +
                          ((uint64_t)o.lseq + 1) / 2 + (uint64_t)o.lseq;
    if (need > (uint64_t)bs) return false;
    o.cig_off = 36u + (uint32_t)o.l_read_name;
    o.seq_off = o.cig_off + 4u * (uint32_t)o.n_cigar;
    o.qual_off = o.seq_off + (uint32_t)((o.lseq + 1) / 2);
    o.aux_off = o.qual_off + (uint32_t)o.lseq;
    int32_t k = 0;
    while (k < o.l_read_name && rec[36 + k]) ++k;
    o.qn_len = k;
    int32_t ql = -1;
    if (o.n_cigar > 0) {
        uint32_t s = 0;
        for (int32_t c = 0; c < o.n_cigar; ++c) {
            const uint32_t v = ld32(rec + o.cig_off + 4 * c);
            const uint32_t op = v & 0xf;
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) s += v >> 4;
        }
        ql = (int32_t)s;
    }
    o.qlen = ql;
    o.rflags = (o.lseq == 0 || rec[o.qual_off] == 0xff) ? RF_QUAL_MISSING : 0;
    return true;
}

UPK_HD uint64_t mix64(uint64_t x) {
    x ^= x >> 31; x *= 0x7fb5d329728ea185ULL; x ^= x >> 27; x *= 0x81dadef4bc2dd44dULL; x ^= x >> 33;
    return x;
}

// 64-bit digest of a record's bytes (block_size excluded, bin zeroed, the tail word tagged with its
// length): record equality for the "line read twice" rule (pysam compares every field of two
// AlignedSegments).  s.word(i, valid): the 8 bytes at record core offset i as a little-endian word,
// bytes from `valid` on zero (valid 0..8).
template <class Src>
UPK_HD uint64_t rec_digest(const Src& s, int32_t bs) {
    uint64_t h = 0x9E3779B97F4A7C15ULL ^ (uint64_t)(uint32_t)bs;
    int32_t i = 0;
    for (; i + 8 <= bs; i += 8) {
        uint64_t w = s.word((uint32_t)i, 8);
        if (i == 8) w &= ~(0xffffULL << 16);   // bin
        h = mix64(h ^ w) + 0x632BE59BD9B4E019ULL;
    }
    uint64_t w = s.word((uint32_t)i, (uint32_t)(bs - i));
    if (i == 8) w &= ~(0xffffULL << 16);
    return mix64(h ^ w ^ ((uint64_t)(bs - i) << 56));
}

struct W16 { uint32_t w[4]; };
struct W8 { uint32_t w[2]; };

// Chunk c (16 B) of the payload slot of a parsed record: qualities zero padded to 16, then the
// sequence nibbles zero padded to the slot's end.  s.bytes16(i, valid): the 16 bytes at rec + i,
// bytes from `valid` on zero (valid 1..16).
template <class Src>
UPK_HD W16 pay_chunk(const Src& s, uint32_t qual_off, uint32_t seq_off, int32_t lseq, uint32_t c) {
    const uint32_t qa = (uint32_t)align16((uint64_t)lseq), nb = (uint32_t)((lseq + 1) / 2);
    const uint32_t at = 16u * c;
    if (at < (uint32_t)lseq) {
        const uint32_t v = (uint32_t)lseq - at;
        return s.bytes16(qual_off + at, v < 16u ? v : 16u);
    }
    if (at >= qa && at - qa < nb) {
        const uint32_t v = nb - (at - qa);
        return s.bytes16(seq_off + (at - qa), v < 16u ? v : 16u);
    }
    return W16{{0u, 0u, 0u, 0u}};
}
// Chunk c (8 B) of the qname slot: the name's qn_len bytes, zero filled.
template <class Src>
UPK_HD W8 qn_chunk(const Src& s, int32_t qn_len, uint32_t c) {
    const uint32_t at = 8u * c;
    if (at < (uint32_t)qn_len) {
        const uint32_t v = (uint32_t)qn_len - at;
        return s.bytes8(36u + at, v < 8u ? v : 8u);
    }
    return W8{{0u, 0u}};
}

// both slots of one record, chunk by chunk (the kernel spreads the same chunks over a lane group)
template <class Src, class Sink>
UPK_HD void write_slots(const Src& s, const Rec& r, Sink& out) {
    const uint32_t np = (uint32_t)(pay_slot(r.lseq) / 16), nq = qn_slot((uint32_t)r.l_read_name) / 8;
    for (uint32_t c = 0; c < np; ++c) out.pay16(c, pay_chunk(s, r.qual_off, r.seq_off, r.lseq, c));
    for (uint32_t c = 0; c < nq; ++c) out.qn8(c, qn_chunk(s, r.qn_len, c));
}

// the plain byte-at-a-time source (host code, and the reference the device's funnel-shifted source
// must agree with): never reads a byte at or past i + valid
struct ByteSrc {
    const uint8_t* rec;   // the block_size word
    UPK_HD uint64_t word(uint32_t i, uint32_t valid) const {
        uint64_t w = 0;
        for (uint32_t k = 0; k < valid; ++k) w |= (uint64_t)rec[4 + i + k] << (8 * k);
        return w;
    }
    UPK_HD W16 bytes16(uint32_t i, uint32_t valid) const {
        W16 o{{0u, 0u, 0u, 0u}};
        for (uint32_t k = 0; k < valid; ++k) o.w[k >> 2] |= (uint32_t)rec[i + k] << (8 * (k & 3));
        return o;
    }
    UPK_HD W8 bytes8(uint32_t i, uint32_t valid) const {
        W8 o{{0u, 0u}};
        for (uint32_t k = 0; k < valid; ++k) o.w[k >> 2] |= (uint32_t)rec[i + k] << (8 * (k & 3));
        return o;
    }
};

}  // namespace upk

#endif
