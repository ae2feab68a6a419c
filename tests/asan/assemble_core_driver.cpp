// csrc/assemble_core.h on the host under AddressSanitizer + UndefinedBehaviorSanitizer: its host
// instantiation (asmb::assemble_host: the layout with its refusals, the stable sort, the offsets and
// out16 cut as the copy kernel cuts it) over the cases tests/test_assemble_core_host.py writes, each
// stream and at[] compared with what ccio_write_bam_ex(..., CCIO_W_MEMORY) assembles.  Every table
// lies in a heap block of exactly its size, so a byte read past an accepted range is reported.
//
// case file: u32 cases, then per case
//   u32 nsrc, per source (u32 len, path);  u64 header bytes, header;  u32 sorted
//   u64 n, n cc_out_spec;  u64 n_names, (n_names + 1) i64 offsets, the names blob (offsets' last value)
//   u64 bytes, cons_seq;  u64 bytes, cons_qual;  u32 n_rg, per value (u32 len, bytes)
//   i64 refused (-1: every spec must be accepted and the stream must match the host writer's)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../consensuscruncher_amd/csrc/assemble_core.h"
#include "../../include/consensuscruncher_amd.h"

static_assert(sizeof(asmb::Spec) == sizeof(cc_out_spec), "asmb::Spec is cc_out_spec");

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

int one(In& in, int c, long long* records) {
    const uint32_t nsrc = in.get<uint32_t>();
    std::vector<ccio_bam*> bams;
    for (uint32_t s = 0; s < nsrc; ++s) {
        const uint32_t ln = in.get<uint32_t>();
        auto p = in.bytes(ln);
        const std::string path((const char*)p.get(), ln);
        ccio_bam* b = ccio_bam_open(path.c_str(), 2);
        if (!b) return fail(c, ccio_last_error());
        bams.push_back(b);
    }
    const uint64_t hb = in.get<uint64_t>();
    auto header = in.bytes(hb);
    const bool sorted = in.get<uint32_t>() != 0;
    const uint64_t n = in.get<uint64_t>();
    auto specb = in.bytes(n * sizeof(cc_out_spec));
    const cc_out_spec* spec = reinterpret_cast<const cc_out_spec*>(specb.get());
    const uint64_t n_names = in.get<uint64_t>();
    std::vector<int64_t> name_off(n_names + 1);
    for (auto& v : name_off) v = in.get<int64_t>();
    auto names = in.bytes((uint64_t)name_off.back());
    const uint64_t csb = in.get<uint64_t>();
    auto cs = in.bytes(csb);
    const uint64_t cqb = in.get<uint64_t>();
    auto cq = in.bytes(cqb);
    const uint32_t n_rg = in.get<uint32_t>();
    ccio_interner* it = ccio_interner_new();
    std::string rgb;
    std::vector<int64_t> rg_off(1, 0);
    for (uint32_t r = 0; r < n_rg; ++r) {
        const uint32_t ln = in.get<uint32_t>();
        auto p = in.bytes(ln);
        const std::string v((const char*)p.get(), ln);
        if (ccio_interner_intern(it, 2, v.c_str()) != (int32_t)r) return fail(c, "RG ids are not the table's order");
        rgb += v;
        rg_off.push_back((int64_t)rgb.size());
    }
    std::unique_ptr<uint8_t[]> rg(new uint8_t[rgb.size() ? rgb.size() : 1]);
    memcpy(rg.get(), rgb.data(), rgb.size());
    const int64_t refused = in.get<int64_t>();
    // the sources as the assembler sees them: each stream in a block of its own size
    std::vector<std::unique_ptr<uint8_t[]>> streams;
    std::vector<std::vector<uint64_t>> offs(nsrc);
    std::vector<asmb::Src> src(nsrc ? nsrc : 1);
    for (uint32_t s = 0; s < nsrc; ++s) {
        const int64_t nr = ccio_bam_nrec(bams[s]);
        std::vector<int64_t> idx((size_t)nr);
        for (int64_t i = 0; i < nr; ++i) idx[(size_t)i] = i;
        const int64_t need = ccio_bam_pack(bams[s], nr, idx.data(), nullptr, 0);
        streams.emplace_back(new uint8_t[need ? need : 1]);
        ccio_bam_pack(bams[s], nr, idx.data(), streams.back().get(), need);
        uint64_t at = 0;
        for (int64_t i = 0; i < nr; ++i) {
            offs[s].push_back(at);
            at += 4 + (uint64_t)upk::ld32(streams.back().get() + at);
        }
        src[s] = asmb::Src{streams.back().get(), 0, (uint64_t)need, offs[s].data(), nr};
    }
    asmb::Tables T{};
    T.src = src.data();
    T.nsrc = (int32_t)nsrc;
    T.n_rg = (int32_t)n_rg;
    T.names = names.get();
    T.name_off = name_off.data();
    T.n_names = (int64_t)n_names;
    T.names_bytes = (uint64_t)name_off.back();
    T.cons_seq = cs.get();
    T.cons_qual = cq.get();
    T.cons_seq_bytes = csb;
    T.cons_qual_bytes = cqb;
    T.rg = rg.get();
    T.rg_off = rg_off.data();
    T.rg_bytes = rgb.size();
    std::vector<uint8_t> out;
    std::vector<uint64_t> at;
    uint32_t err = 0;
    const int64_t bad = asmb::assemble_host(header.get(), hb, reinterpret_cast<const asmb::Spec*>(spec), (int64_t)n, T, sorted,
                                            out, at, &err);
    *records += (long long)n;
    int rc = 0;
    if (bad != refused) {
        printf("case %d: first refused spec %lld (bits %u), expected %lld\n", c, (long long)bad, err, (long long)refused);
        rc = 1;
    } else if (refused < 0) {
        ccio_bam* keep = nullptr;
        if (ccio_write_bam_ex("", bams[0], it, (int64_t)n, spec, bams.data(), (int)nsrc, (const char*)names.get(), name_off.data(),
                              cs.get(), cq.get(), 1, 2, CCIO_W_MEMORY | (sorted ? CCIO_W_SORT : 0), &keep) != 0)
            return fail(c, ccio_last_error());
        const int64_t nr = ccio_bam_nrec(keep);
        std::vector<int64_t> idx((size_t)nr);
        for (int64_t i = 0; i < nr; ++i) idx[(size_t)i] = i;
        const int64_t need = ccio_bam_pack(keep, nr, idx.data(), nullptr, 0);
        std::vector<uint8_t> want((size_t)need + 1);
        ccio_bam_pack(keep, nr, idx.data(), want.data(), need);
        if (nr != (int64_t)n || (uint64_t)need + hb != out.size() || memcmp(out.data(), header.get(), hb) != 0 ||
            memcmp(out.data() + hb, want.data(), (size_t)need) != 0)
            rc = fail(c, "the stream differs from the host writer's");
        uint64_t a = hb;
        for (int64_t i = 0; i < nr && !rc; ++i) {
            if (at[(size_t)i] != a) rc = fail(c, "at[] differs from the host writer's record starts");
            a += 4 + (uint64_t)upk::ld32(want.data() + (a - hb));
        }
        if (!rc && at[(size_t)n] != a) rc = fail(c, "at[n] is not the stream's size");
        ccio_bam_close(keep);
    }
    ccio_interner_free(it);
    for (ccio_bam* b : bams) ccio_bam_close(b);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    In in{f};
    const uint32_t cases = in.get<uint32_t>();
    long long records = 0;
    int bad = 0;
    for (uint32_t c = 0; c < cases; ++c) bad += one(in, (int)c, &records);
    fclose(f);
    if (bad) return 1;
    printf("ok %u %lld\n", cases, records);
    return 0;
}
