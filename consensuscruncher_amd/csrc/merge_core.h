// The rules of the merge of sorted record sets (samtools merge stand-in, ccio_merge_handles): the
// key, the record check, the searches and the place rule.  Plain C++ that compiles in the HIP kernels
// (bam_merge.hip.inc: k_merge_keys, k_merge_rank) and with a host compiler alone (merge_host below;
// tests/asan/merge_core_driver.cpp runs it under sanitizers), so both execute the same text.
//
// The contract (a bad source must never fault a device other people share):
//   * record() reads a record's block_size word only after its offset was checked against the
//     source's bytes, and its core only after block_size was checked against them: it is the only
//     function that may run on unchecked offsets, and refuses with a distinct code whatever does
//     not fit;
//   * lower() / upper() read keys[a, b) only; place() reads what they read.
#ifndef CC_MERGE_CORE_H
#define CC_MERGE_CORE_H

#include "assemble_core.h"

#if defined(__HIPCC__)
#define MRG_HD __host__ __device__ inline
#else
#define MRG_HD inline
#endif

namespace mrg {

using upk::W16;

constexpr int MRG_MAX_SRC = 8;   // inputs of one merge
constexpr int MRG_TILE = 256;    // records of one source per rank block (its threads)
constexpr int MRG_WIN = 1024;    // keys of one other source a rank block stages in LDS

// refusals (the first bad record's code is reported)
enum : uint32_t {
    ME_OFF = 1u,    // the record's offset lies outside its source
    ME_SHORT = 2u,  // fewer than 4 bytes left for the block_size word
    ME_BS = 3u,     // block_size < 32: no room for the core
    ME_PAST = 4u,   // the record runs past the source's bytes
};

// ccio.cpp's coord_key over the core's first 16 bytes (tid, pos, bin_mq_nl, flag_nc):
// (uint32 tid) << 32 | (uint32)(pos + 1) << 1 | reverse, so tid -1 sorts last and pos -1 first
MRG_HD uint64_t key(const W16& core) {
    return ((uint64_t)core.w[0] << 32) | ((uint64_t)(uint32_t)(core.w[1] + 1u) << 1) | ((core.w[3] >> 20) & 1u);
}

// The record at base[shift + rel ...) of a source of `bytes` bytes checked; *size is its size with
// the block_size word, *k its key.  F::fetch(base, a, valid): the bytes base[a, a + valid), zero
// from `valid` on.  Returns the refusal code, 0 when *size and *k are valid.
template <class F>
MRG_HD uint32_t record(const uint8_t* base, uint64_t shift, uint64_t bytes, uint64_t rel, uint32_t* size, uint64_t* k) {
    if (rel >= bytes) return ME_OFF;
    const uint64_t left = bytes - rel;
    if (left < 4) return ME_SHORT;
    const uint32_t bs = F::fetch(base, shift + rel, 4u).w[0];
    if (bs < 32u) return ME_BS;
    if ((uint64_t)bs + 4u > left || bs > 0xfffffffbu) return ME_PAST;
    *size = bs + 4u;
    *k = key(F::fetch(base, shift + rel + 4u, 16u));
    return 0;
}

// the first index of keys[a, b) (non-decreasing) whose key is not below k (b: none)
MRG_HD int64_t lower(const uint64_t* keys, int64_t a, int64_t b, uint64_t k) {
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (keys[m] < k) a = m + 1;
        else b = m;
    }
    return a;
}
// the first index of keys[a, b) whose key is above k
MRG_HD int64_t upper(const uint64_t* keys, int64_t a, int64_t b, uint64_t k) {
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (keys[m] <= k) a = m + 1;
        else b = m;
    }
    return a;
}

// The place rule: record i of source s (key k) goes to i + the records of every earlier source
// with a key up to k + the records of every later source with a key below k.  Ties go to the
// earlier input, then the earlier record: a stable sort of the concatenation.
// keys: the sources' keys side by side, source s2's at keys[first[s2], first[s2 + 1]).
MRG_HD int64_t place(const uint64_t* keys, const int64_t* first, int nsrc, int s, int64_t i, uint64_t k) {
    int64_t d = i;
    for (int s2 = 0; s2 < nsrc; ++s2) {
        if (s2 == s) continue;
        const uint64_t* k2 = keys + first[s2];
        const int64_t n2 = first[s2 + 1] - first[s2];
        d += s2 < s ? upper(k2, 0, n2, k) : lower(k2, 0, n2, k);
    }
    return d;
}

#if !defined(__HIPCC__)
// The whole merge on the host, as the device runs it: the keys pass (check, key, size, order), the
// place rule, the offsets, then the records.  header_bytes + records into out (resized), at[n + 1]
// and org[n].  Returns 0, or the refusal code with *bad_src / *bad_rec naming the record; an
// out-of-order pair is code ME_ORDER with the later record named.
enum : uint32_t { ME_ORDER = 16u };
inline uint32_t merge_host(const uint8_t* header, uint64_t header_bytes, const asmb::Src* src, int nsrc,
                           std::vector<uint8_t>& out, std::vector<uint64_t>& at, std::vector<uint32_t>& org,
                           int* bad_src, int64_t* bad_rec) {
    std::vector<int64_t> first((size_t)nsrc + 1, 0);
    for (int s = 0; s < nsrc; ++s) first[(size_t)s + 1] = first[(size_t)s] + src[s].nrec;
    const int64_t n = first[(size_t)nsrc];
    std::vector<uint64_t> keys((size_t)n);
    std::vector<uint32_t> sz((size_t)n);
    for (int s = 0; s < nsrc; ++s)
        for (int64_t i = 0; i < src[s].nrec; ++i) {
            const size_t g = (size_t)(first[(size_t)s] + i);
            const uint32_t e = record<asmb::ByteFetch>(src[s].base, src[s].shift, src[s].bytes, src[s].rec_off[i], &sz[g], &keys[g]);
            if (e || (i > 0 && keys[g] < keys[g - 1])) {
                *bad_src = s;
                *bad_rec = i;
                return e ? e : ME_ORDER;
            }
        }
    org.assign((size_t)n, 0);
    for (int s = 0; s < nsrc; ++s)
        for (int64_t i = 0; i < src[s].nrec; ++i) {
            const int64_t g = first[(size_t)s] + i;
            org[(size_t)place(keys.data(), first.data(), nsrc, s, i, keys[(size_t)g])] = (uint32_t)g;
        }
    at.assign((size_t)n + 1, 0);
    at[0] = header_bytes;
    for (int64_t o = 0; o < n; ++o) at[(size_t)o + 1] = at[(size_t)o] + sz[org[(size_t)o]];
    out.assign((size_t)at[(size_t)n], 0xee);
    for (uint64_t b = 0; b < header_bytes; ++b) out[(size_t)b] = header[b];
    for (int64_t o = 0; o < n; ++o) {
        const int64_t g = org[(size_t)o];
        int s = 0;
        while (g >= first[(size_t)s + 1]) ++s;
        const asmb::Src& S = src[s];
        const uint8_t* r = S.base + S.shift + S.rec_off[g - first[(size_t)s]];
        for (uint32_t b = 0; b < sz[(size_t)g]; ++b) out[(size_t)at[(size_t)o] + b] = r[b];
    }
    return 0;
}
#endif

}  // namespace mrg

#endif
