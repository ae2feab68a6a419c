// csrc/name_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: its host
// instantiation (nmc::csn_host / nmc::dcs_host: the sizes pass with its refusals, the offsets, and the
// names cut as the write kernels cut them) over the cases tests/test_name_core_host.py writes, each
// blob and off[] compared with ccio_format_csn_names / ccio_format_dcs_names.  Every table lies in a
// heap block of exactly its size and the blob has exactly `total` bytes, so a byte read or written
// past an accepted range is reported.
//
// case file: u32 cases, then per case  u32 kind (0 csn, 1 dcs), i64 refused (-1: every name must be
// accepted and the blob must match the host function's), u32 host (1: the host function is asked too)
//   csn: u32 n_bc, per string (u32 len, bytes);  u32 n_cg, likewise;  u64 n, 9 n i32 fields, n i64 suffixes
//   dcs: u32 len, the BAM's path;  u64 n, n i64 rec_tag, n i64 rec_ds
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../consensuscruncher_amd/csrc/name_core.h"
#include "../../include/consensuscruncher_amd.h"

namespace {

struct In {
    FILE* f;
    template <class T> T get() {
        T v;
        if (fread(&v, sizeof v, 1, f) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
        return v;
    }
    // exactly n bytes on the heap (n == 0: a one-byte block nobody may read)
    std::unique_ptr<uint8_t[]> bytes(uint64_t n) {
        std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
        if (n && fread(p.get(), 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
        return p;
    }
};

int fail(int c, const char* what) {
    printf("case %d: %s\n", c, what);
    return 1;
}

struct Table {
    std::unique_ptr<uint8_t[]> blob;
    std::vector<int64_t> off;
    nmc::Strs strs;
};

// n strings interned in order (their ids must be 0 .. n - 1) and laid side by side in an exact block
bool strings(In& in, ccio_interner* it, int kind, Table& t) {
    const uint32_t n = in.get<uint32_t>();
    std::string all;
    t.off.assign(1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t ln = in.get<uint32_t>();
        auto p = in.bytes(ln);
        const std::string s((const char*)p.get(), ln);
        if (ccio_interner_intern(it, kind, s.c_str()) != (int32_t)i) return false;
        all += s;
        t.off.push_back((int64_t)all.size());
    }
    // what the engine uploads: ccio_interner_blob's strings and offsets
    std::vector<int64_t> off(n + 1);
    const int64_t need = ccio_interner_blob(it, kind, nullptr, 0, off.data());
    if (need != (int64_t)all.size() || off != t.off) return false;
    t.blob.reset(new uint8_t[need ? need : 1]);
    if (ccio_interner_blob(it, kind, (char*)t.blob.get(), need, off.data()) != need) return false;
    if (memcmp(t.blob.get(), all.data(), all.size()) != 0) return false;
    if (need > 0 && ccio_interner_blob(it, kind, (char*)t.blob.get(), need - 1, off.data()) != -1) return false;
    t.strs = nmc::Strs{t.blob.get(), t.off.data(), (int64_t)n, (uint64_t)need};
    return true;
}

int verdict(int c, int64_t bad, uint32_t err, int64_t refused) {
    if (bad == refused) return 0;
    printf("case %d: first refused name %lld (bits %u), expected %lld\n", c, (long long)bad, err, (long long)refused);
    return 1;
}

int same(int c, const std::vector<uint8_t>& blob, const std::vector<int64_t>& off, const std::vector<char>& want,
         const std::vector<int64_t>& woff) {
    if (off != woff) return fail(c, "off[] differs from the host function's");
    if (blob.size() != want.size() || (!want.empty() && memcmp(blob.data(), want.data(), want.size()) != 0))
        return fail(c, "the blob differs from the host function's");
    return 0;
}

int csn(In& in, int c, int64_t refused, bool host, long long* names) {
    ccio_interner* it = ccio_interner_new();
    Table bc, cg;
    if (!strings(in, it, 0, bc) || !strings(in, it, 1, cg)) return fail(c, "ccio_interner_blob does not give the strings");
    const uint64_t n = in.get<uint64_t>();
    auto fb = in.bytes(n * 36);
    auto sb = in.bytes(n * 8);
    const int32_t* f9 = reinterpret_cast<const int32_t*>(fb.get());
    const int64_t* suf = reinterpret_cast<const int64_t*>(sb.get());
    std::vector<uint8_t> blob;
    std::vector<int64_t> off;
    uint32_t err = 0;
    const int64_t bad = nmc::csn_host((int64_t)n, f9, suf, bc.strs, cg.strs, blob, off, &err);
    *names += (long long)n;
    int rc = verdict(c, bad, err, refused);
    if (!rc && host) {
        std::vector<int64_t> woff(n + 1);
        const int64_t need = ccio_format_csn_names(it, (int64_t)n, f9, suf, nullptr, 0, woff.data());
        if (refused >= 0) {
            if (need != -1) rc = fail(c, "the host function accepts what the core refuses");
        } else if (need < 0) {
            rc = fail(c, ccio_last_error());
        } else {
            std::vector<char> want((size_t)need);
            ccio_format_csn_names(it, (int64_t)n, f9, suf, want.data(), need, woff.data());
            rc = same(c, blob, off, want, woff);
        }
    }
    ccio_interner_free(it);
    return rc;
}

int dcs(In& in, int c, int64_t refused, bool host, long long* names) {
    const uint32_t ln = in.get<uint32_t>();
    auto pp = in.bytes(ln);
    const std::string path((const char*)pp.get(), ln);
    ccio_bam* b = ccio_bam_open(path.c_str(), 2);
    if (!b) return fail(c, ccio_last_error());
    const uint64_t n = in.get<uint64_t>();
    auto tb = in.bytes(n * 8);
    auto db = in.bytes(n * 8);
    const int64_t* rec_tag = reinterpret_cast<const int64_t*>(tb.get());
    const int64_t* rec_ds = reinterpret_cast<const int64_t*>(db.get());
    // the table's qname slots (upk::qn_slot, zero padded) in a block of exactly their size
    const int64_t nr = ccio_bam_nrec(b);
    std::vector<int64_t> idx((size_t)nr);
    for (int64_t i = 0; i < nr; ++i) idx[(size_t)i] = i;
    const int64_t need = ccio_bam_pack(b, nr, idx.data(), nullptr, 0);
    std::vector<uint8_t> stream((size_t)need + 1);
    ccio_bam_pack(b, nr, idx.data(), stream.data(), need);
    std::vector<uint64_t> qn_off((size_t)nr);
    std::vector<uint16_t> qn_len((size_t)nr);
    std::vector<upk::Rec> recs((size_t)nr);
    uint64_t at = 0, slots = 0;
    std::vector<uint64_t> rec_at((size_t)nr);
    for (int64_t i = 0; i < nr; ++i) {
        if (!upk::parse(stream.data() + at, (uint64_t)need - at, recs[(size_t)i])) return fail(c, "a record does not parse");
        rec_at[(size_t)i] = at;
        qn_off[(size_t)i] = slots;
        qn_len[(size_t)i] = (uint16_t)recs[(size_t)i].qn_len;
        slots += upk::qn_slot((uint32_t)recs[(size_t)i].l_read_name);
        at += 4 + (uint64_t)recs[(size_t)i].bs;
    }
    std::unique_ptr<uint8_t[]> qb(new uint8_t[slots ? slots : 1]);
    memset(qb.get(), 0, slots ? slots : 1);
    for (int64_t i = 0; i < nr; ++i) memcpy(qb.get() + qn_off[(size_t)i], stream.data() + rec_at[(size_t)i] + 36, qn_len[(size_t)i]);
    std::vector<uint8_t> blob;
    std::vector<int64_t> off;
    uint32_t err = 0;
    const int64_t bad = nmc::dcs_host((int64_t)n, rec_tag, rec_ds, qb.get(), qn_off.data(), qn_len.data(), nr, blob, off, &err);
    *names += (long long)n;
    int rc = verdict(c, bad, err, refused);
    if (!rc && host) {
        if (ccio_dcs_names_plain(b, (int64_t)n, rec_tag, rec_ds) != 1) rc = fail(c, "the names are not plain");
        std::vector<int64_t> woff(n + 1);
        const int64_t wneed = rc ? 0 : ccio_format_dcs_names(b, (int64_t)n, rec_tag, rec_ds, nullptr, 0, woff.data());
        if (rc) {
        } else if (refused >= 0) {
            if (wneed != -1) rc = fail(c, "the host function accepts what the core refuses");
        } else if (wneed < 0) {
            rc = fail(c, ccio_last_error());
        } else {
            std::vector<char> want((size_t)wneed);
            ccio_format_dcs_names(b, (int64_t)n, rec_tag, rec_ds, want.data(), wneed, woff.data());
            rc = same(c, blob, off, want, woff);
        }
    }
    ccio_bam_close(b);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    In in{f};
    const uint32_t cases = in.get<uint32_t>();
    long long names = 0;
    int bad = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        const uint32_t kind = in.get<uint32_t>();
        const int64_t refused = in.get<int64_t>();
        const bool host = in.get<uint32_t>() != 0;
        bad += kind == 0 ? csn(in, (int)c, refused, host, &names) : dcs(in, (int)c, refused, host, &names);
    }
    fclose(f);
    if (bad) return 1;
    printf("ok %u %lld\n", cases, names);
    return 0;
}
