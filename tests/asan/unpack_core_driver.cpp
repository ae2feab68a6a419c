// csrc/unpack_core.h on the host under -fsanitize=address,undefined (tests/test_unpack_core_host.py
// builds and runs this; nothing is loaded into Python).  The parser, rec_digest and the slot writer
// run over streams held in heap blocks of exactly the stream's size, and write slots into heap
// blocks of exactly the slot's size, so a read or write outside the contract is a sanitizer report.
//
// Input file: cases, each  u32 stream_len, u32 n_records, stream bytes, then per record
//   u64 offset, u8 want (0 must be refused, 1 refused or parsed inside bounds, 2 must parse to:)
//   want 2 only: 13 x i32 (bs tid pos l_read_name mapq n_cigar flag lseq mtid mpos tlen qn_len qlen),
//                4 x u32 (cigar, seq, qual, aux offsets), u8 rflags, u64 rdig,
//                u32 payload slot bytes, u32 qname slot bytes, the two slots' bytes.
// Output: "ok <records> <accepted>", exit 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../consensuscruncher_amd/csrc/unpack_core.h"

namespace {

struct Reader {
    const uint8_t* p;
    const uint8_t* e;
    template <class T>
    T get() {
        T v;
        if (p + sizeof(T) > e) { fprintf(stderr, "case file truncated\n"); exit(2); }
        memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    const uint8_t* bytes(size_t n) {
        if (p + n > e) { fprintf(stderr, "case file truncated\n"); exit(2); }
        const uint8_t* q = p;
        p += n;
        return q;
    }
};

// slots of exactly their size on the heap; a chunk outside them is a failure before it is a write
struct HeapSink {
    uint8_t* pay;
    uint8_t* qn;
    uint32_t np, nq;
    bool ok = true;
    void pay16(uint32_t c, const upk::W16& w) {
        if (c >= np) { ok = false; return; }
        memcpy(pay + 16 * (size_t)c, w.w, 16);
    }
    void qn8(uint32_t c, const upk::W8& w) {
        if (c >= nq) { ok = false; return; }
        memcpy(qn + 8 * (size_t)c, w.w, 8);
    }
};

int fail(long rec, const char* what) {
    printf("FAIL record %ld: %s\n", rec, what);
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + k);
    fclose(f);
    Reader in{file.data(), file.data() + file.size()};
    long records = 0, accepted = 0;
    while (in.p < in.e) {
        const uint32_t len = in.get<uint32_t>(), n = in.get<uint32_t>();
        const uint8_t* src = in.bytes(len);
        uint8_t* blk = (uint8_t*)malloc(len ? len : 1);   // exactly the stream
        memcpy(blk, src, len);
        for (uint32_t r = 0; r < n; ++r, ++records) {
            const uint64_t off = in.get<uint64_t>();
            const uint8_t want = in.get<uint8_t>();
            if (off > len) return fail(records, "offset past the stream in the case file");
            upk::Rec got;
            const uint64_t avail = len - off;
            const bool ok = upk::parse(blk + off, avail, got);
            if (want == 0 && ok) return fail(records, "accepted a record that must be refused");
            if (want == 2 && !ok) return fail(records, "refused a valid record");
            if (ok) {
                ++accepted;
                const uint64_t end = 4 + (uint64_t)got.bs;
                if (end > avail || got.bs < 32 || got.lseq < 0) return fail(records, "accepted outside the stream");
                if (got.cig_off > end || got.seq_off > end || got.qual_off > end || got.aux_off > end ||
                    got.cig_off > got.seq_off || got.seq_off > got.qual_off || got.qual_off > got.aux_off)
                    return fail(records, "offsets outside the record");
                if (got.qn_len < 0 || got.qn_len > got.l_read_name) return fail(records, "qname length");
                // digest and slots over the accepted record, into heap blocks of exactly their size
                const upk::ByteSrc bs{blk + off};
                const uint64_t dig = upk::rec_digest(bs, got.bs);
                HeapSink out;
                out.np = (uint32_t)(upk::pay_slot(got.lseq) / 16);
                out.nq = upk::qn_slot((uint32_t)got.l_read_name) / 8;
                out.pay = (uint8_t*)malloc(16 * (size_t)out.np + 1);
                out.qn = (uint8_t*)malloc(8 * (size_t)out.nq + 1);
                memset(out.pay, 0xA5, 16 * (size_t)out.np);
                memset(out.qn, 0xA5, 8 * (size_t)out.nq);
                upk::write_slots(bs, got, out);
                int bad = out.ok ? 0 : fail(records, "slot chunk out of range");
                if (!bad && want == 2) {
                    int32_t w[13];
                    for (int i = 0; i < 13; ++i) w[i] = in.get<int32_t>();
                    uint32_t o[4];
                    for (int i = 0; i < 4; ++i) o[i] = in.get<uint32_t>();
                    const uint8_t rf = in.get<uint8_t>();
                    const uint64_t wdig = in.get<uint64_t>();
                    const uint32_t pl = in.get<uint32_t>(), ql = in.get<uint32_t>();
                    const uint8_t* wp = in.bytes(pl);
                    const uint8_t* wq = in.bytes(ql);
                    const int32_t g[13] = {got.bs, got.tid, got.pos, got.l_read_name, got.mapq, got.n_cigar, got.flag,
                                           got.lseq, got.mtid, got.mpos, got.tlen, got.qn_len, got.qlen};
                    if (memcmp(w, g, sizeof g)) bad = fail(records, "fields differ");
                    else if (o[0] != got.cig_off || o[1] != got.seq_off || o[2] != got.qual_off || o[3] != got.aux_off)
                        bad = fail(records, "offsets differ");
                    else if (rf != got.rflags) bad = fail(records, "rflags differ");
                    else if (wdig != dig) bad = fail(records, "digest differs");
                    else if (pl != 16 * out.np || ql != 8 * out.nq) bad = fail(records, "slot sizes differ");
                    else if (memcmp(wp, out.pay, pl)) bad = fail(records, "payload slot differs");
                    else if (memcmp(wq, out.qn, ql)) bad = fail(records, "qname slot differs");
                }
                free(out.pay);
                free(out.qn);
                if (bad) return bad;
            }
        }
        free(blk);
    }
    printf("ok %ld %ld\n", records, accepted);
    return 0;
}
