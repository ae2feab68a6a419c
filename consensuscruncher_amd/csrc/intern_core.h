// The per-record parts of the device interner: where a parsed record's three interned keys lie (the
// raw cigar, the barcode inside the read name, the RG value inside the aux fields), the two
// string-derived record flags, and the seeded 64-bit hash of a key's bytes.  Plain C++ that compiles
// in the HIP kernels (table_ids.hip.inc: k_ids_keys), in libccio (ccio.cpp: ccio_intern_keys) and with a
// host compiler alone (tests/asan/intern_core_driver.cpp runs it under sanitizers), so all of them
// execute the same text.
//
// The rules are StringPass::one's and find_rg's (ccio.cpp), with one difference: find_rg trusts the
// aux fields and can read past the record on malformed ones.  The contract here (a corrupt record
// must never fault a device other people share):
//   * every finder reads only bytes of [rec, rec + 4 + bs) of a record upk::parse accepted;
//   * a returned key lies inside the record: off + len <= 4 + bs;
//   * an aux value that does not lie whole inside the record -- a fixed-width value, a B header or a
//     B array cut by the record's end, a negative B count -- refuses the record (refuse = true):
//     nothing else of the result is meaningful then.  A Z or H value without a NUL ends at the
//     record's end, as find_rg ends it.
#ifndef CC_INTERN_CORE_H
#define CC_INTERN_CORE_H

#include "unpack_core.h"

namespace itn {

constexpr uint8_t RF_BAD_SPACER = 1;       // CC_RF_BAD_SPACER (include/consensuscruncher_amd.h)
constexpr uint8_t RF_RG_UNSUPPORTED = 4;   // CC_RF_RG_UNSUPPORTED
constexpr int DELIM_MAX = 16;

// the barcode delimiter, passed to the kernel by value
struct Delim {
    uint8_t b[DELIM_MAX];
    int32_t len;
};

struct Key {
    uint32_t off, len;   // the key's bytes, from rec (the block_size word is bytes 0..3)
    bool none;           // the record has no key in this table (id -1)
    uint8_t flags;       // RF_BAD_SPACER / RF_RG_UNSUPPORTED
    bool refuse;
};

// the raw cigar: 4 * n_cigar bytes (no bytes without a cigar: that key prints as "None")
UPK_HD Key cigar_key(const uint8_t*, const upk::Rec& f) {
    return Key{f.cig_off, 4u * (uint32_t)f.n_cigar, false, 0, false};
}

// first occurrence of d in name[from, qn) (the name starts at rec + 36), or -1
UPK_HD int32_t find_delim(const uint8_t* rec, int32_t qn, int32_t from, const Delim& d) {
    if (d.len <= 0 || from > qn) return -1;
    for (int32_t x = from; x + d.len <= qn; ++x) {
        int32_t k = 0;
        while (k < d.len && rec[36 + x + k] == d.b[k]) ++k;
        if (k == d.len) return x;
    }
    return -1;
}

// mode 0: the bytes between the first delimiter and the next one (or the name's end); no delimiter
// is RF_BAD_SPACER without a key.  mode 1: the bytes before the first '_', or the whole name.
UPK_HD Key barcode_key(const uint8_t* rec, const upk::Rec& f, int mode, const Delim& d) {
    const int32_t qn = f.qn_len;
    if (mode == 0) {
        const int32_t d0 = find_delim(rec, qn, 0, d);
        if (d0 < 0) return Key{0, 0, true, RF_BAD_SPACER, false};
        const int32_t st = d0 + d.len;
        const int32_t d1 = find_delim(rec, qn, st, d);
        return Key{36u + (uint32_t)st, (uint32_t)((d1 < 0 ? qn : d1) - st), false, 0, false};
    }
    int32_t u = 0;
    while (u < qn && rec[36 + u] != '_') ++u;
    return Key{36u, (uint32_t)u, false, 0, false};
}

// the RG value: Z up to its NUL or the record's end, A one byte; H and the fixed-width types on RG,
// RG:B anywhere before it, and an unknown type set RF_RG_UNSUPPORTED without a key
UPK_HD Key rg_key(const uint8_t* rec, const upk::Rec& f) {
    const uint64_t end = 4ull + (uint64_t)(uint32_t)f.bs;
    uint64_t p = f.aux_off;
    bool bad = false;
    const Key refused{0, 0, true, 0, true};
    while (p + 3 <= end) {
        const uint8_t t0 = rec[p], t1 = rec[p + 1], ty = rec[p + 2];
        p += 3;
        const bool is_rg = t0 == 'R' && t1 == 'G';
        uint64_t sz = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': {
                uint64_t q = p;
                while (q < end && rec[q]) ++q;
                if (is_rg) {
                    if (ty != 'Z') bad = true;
                    return Key{(uint32_t)p, (uint32_t)(q - p), bad, (uint8_t)(bad ? RF_RG_UNSUPPORTED : 0), false};
                }
                p = q + 1;
                continue;
            }
            case 'B': {
                if (p + 5 > end) return refused;
                const uint8_t sub = rec[p];
                const int32_t cnt = (int32_t)upk::ld32(rec + p + 1);
                const uint64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                if (cnt < 0 || p + 5 + es * (uint64_t)cnt > end) return refused;
                if (is_rg) bad = true;
                p += 5 + es * (uint64_t)cnt;
                continue;
            }
            default: return Key{0, 0, true, RF_RG_UNSUPPORTED, false};
        }
        if (p + sz > end) return refused;
        if (is_rg) {
            if (ty != 'A') bad = true;
            return Key{(uint32_t)p, 1, bad, (uint8_t)(bad ? RF_RG_UNSUPPORTED : 0), false};
        }
        p += sz;
    }
    return Key{0, 0, true, (uint8_t)(bad ? RF_RG_UNSUPPORTED : 0), false};
}

// seeded 64-bit hash of len bytes (the engine's mix64 chain over little-endian 8-byte words, the
// tail word tagged with the length), read one byte at a time: keys start at any alignment
UPK_HD uint64_t hash_bytes(const uint8_t* p, uint32_t len, uint64_t seed) {
    uint64_t h = upk::mix64(seed ^ (0x9E3779B97F4A7C15ULL + (uint64_t)len));
    uint32_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t w = 0;
        for (uint32_t k = 0; k < 8; ++k) w |= (uint64_t)p[i + k] << (8 * k);
        h = upk::mix64(h ^ w) + 0x632BE59BD9B4E019ULL;
    }
    uint64_t w = 0;
    for (uint32_t k = 0; i + k < len; ++k) w |= (uint64_t)p[i + k] << (8 * k);
    return upk::mix64(h ^ w ^ ((uint64_t)(len - i) << 56));
}

}  // namespace itn

#endif
