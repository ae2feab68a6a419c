/*
 * consensuscruncher_amd.h — C ABI of the MI355X consensus engine.
 *
 * Two shared libraries sit behind this header:
 *
 *   libccio.so  (host C++)  BAM/BGZF codec, SoA packing, output assembly.
 *                            Replaces pysam/htslib as used by the stage scripts
 *                            (consensus_helper.py:25; SSCS_maker.py:233-244;
 *                            DCS_maker.py:162-176; singleton_correction.py:146-164)
 *                            and the samtools sort/merge calls of
 *                            ConsensusCruncher.py:10-34,262-266,299-304.
 *   libccamd.so (HIP, gfx950) the consensus hot path on the GPU:
 *        cc_read_bam            <- consensus_helper.read_bam           (consensus_helper.py:308-506)
 *                                  + which_read/which_strand/cigar_order/sscs_qname/unique_tag (:57-305)
 *        cc_consensus_maker     <- SSCS_maker.consensus_maker + the SSCS region loop
 *                                  (SSCS_maker.py:81-168, 312-339) + create_aligned_segment
 *                                  /read_mode/consensus_flag (consensus_helper.py:509-619)
 *        cc_duplex_consensus    <- DCS_maker main pairing loop + duplex_consensus + duplex_tag
 *                                  (DCS_maker.py:99-123, 245-282; consensus_helper.py:639-683)
 *        cc_singleton_correction<- singleton_correction main loop + duplex_consensus/strand_correction
 *                                  (singleton_correction.py:61-111, 278-319)
 *
 * The reference has no FFI: its boundary is three Python scripts launched by
 * ConsensusCruncher.py consensus (ConsensusCruncher.py:171-185,206-213,230-237,
 * 280-287).  The Python stage scripts in consensuscruncher_amd/ keep those CLIs
 * and call these entry points through ctypes.
 *
 * Conventions: every function returns 0 on success and a negative CC_E_* code
 * on failure (text from cc_last_error / ccio_last_error).  Host buffers are
 * always owned by the caller; device buffers by the context.  No C++ types
 * cross the ABI.
 */
#ifndef CONSENSUSCRUNCHER_AMD_H
#define CONSENSUSCRUNCHER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ errors */
#define CC_OK 0
#define CC_E_INVALID -1        /* bad argument / handle */
#define CC_E_HIP -2            /* HIP runtime error */
#define CC_E_N_HIGHQ -3        /* N base with Q>=30 inside a family of size>=2 (SSCS_maker.py:129 IndexError) */
#define CC_E_BAD_BASE -4       /* base outside A,C,G,T,N in a voted family (SSCS_maker.py:122,127 ValueError) */
#define CC_E_SHORT_READ -5     /* member shorter than the inferred read length (IndexError) */
#define CC_E_NO_QUAL -6        /* qualities absent ('*') in a voted read (TypeError) */
#define CC_E_NO_CIGAR -7       /* infer_query_length() is None (TypeError) */
#define CC_E_DUP_QNAME -8      /* (no longer returned: qnames seen more than twice pair in stream order) */
#define CC_E_AMBIGUOUS -9      /* (retired, never returned: the region loops' deletions are followed; the
                                  number stays reserved) */
#define CC_E_COLLISION -10     /* internal 64-bit hash collision (callers retry with another seed) */
#define CC_E_UNSUPPORTED -11
#define CC_E_KEYERROR -12      /* the reference raises KeyError (DCS_maker.py:258: read_dict[duplex] deleted,
                                  reached with duplex keys that are not mutual) */
#define CC_E_REPLAY -13        /* cc_commit: a deferred planned pass did not hold; run the same calls again
                                  with deferral off */

/* record flags (cc_records.rflags) */
#define CC_RF_BAD_SPACER 1u    /* barcode delimiter absent from qname (consensus_helper.py:408) */
#define CC_RF_QUAL_MISSING 2u  /* BAM qual[0] == 0xff */
#define CC_RF_RG_UNSUPPORTED 4u/* RG tag of a type other than Z/A */

/* ---------------------------------------------------------- record SoA
 * One entry per BAM record, in file order.  The payload blob holds, per
 * record at pay_off[i] (16-byte aligned): qualities (lseq bytes, zero padded to
 * 16) then the BAM 4-bit sequence ((lseq+1)/2 bytes, first base in the high
 * nibble, zero padded to 16).  qn_blob holds each qname in an 8-byte aligned,
 * zero padded slot at qn_off[i].  String fields are exact interned ids
 * (ccio_interner): bc_id (barcode by stage mode, -1 if absent), cigar_id
 * (cigarstring, 'None' interned for no cigar), rg_id (-1 if no RG). */
typedef struct cc_records {
    int64_t n;
    int32_t *tid, *pos, *mtid, *mpos, *tlen;
    uint16_t *flag;
    uint8_t *mapq;
    int32_t *cigar_id, *qlen, *lseq, *bc_id, *rg_id;
    uint8_t *rflags;
    uint64_t *qn_off;
    uint16_t *qn_len;
    uint8_t *qn_blob;
    uint64_t qn_blob_bytes;
    uint64_t *pay_off;
    uint8_t *payload;
    uint64_t payload_bytes;
    uint64_t *rdig;     /* 64-bit digest of the whole record (every byte but bin): record equality,
                           pysam's AlignedSegment.__eq__, for the "line read twice" rule when a qname
                           occurs more than twice (consensus_helper.py:490-500) */
    /* Optional: the kernels' per-record layout, built by the decoder (ccio_bam_decode fills it when
     * meta is non-NULL, as one more pass over records it has in hand) so the device never re-packs the
     * columns above.  NULL meta (or n_deep < 0 after decode: a length beyond the 16-bit fields) and
     * cc_table_upload derives the same columns on the device (k_derive).
     *   rkey[i]    position key ((uint32)(tid < 0 ? -1 : tid) << 32 | (uint32)pos)
     *   meta[4i..] the votes' member record: pay_off / 16, tlen, lseq | qlen << 16 (0xffff: no cigar),
     *              flag & 0xfff | mapq << 12 | (rflags & 7) << 20 | rg7 << 24 (rg7 0x7f: none, 0x7e: id >= 126)
     *   core[8i..] tid (-1 when negative), pos, mtid, mpos, tlen, cigar_id, bc_id, flag | 1 << 16 when deep
     *   qn_ol[i]   qn_off << 16 | qn_len
     *   qdig[i]    the unseeded 64-bit qname digest (the engine's hcomb chain over the qname words)
     *   rdeep[i]   1 when the record's run of equal rkey holds more than 64 records ("deep")
     *   dlist      the first records of the deep runs (capacity n / 65 + 2), n_deep of them
     *   ext[t]     for t < n_ext (capacity: the header's reference count), the position (>= 0) of the
     *              last record of tid t's last run */
    uint64_t *rkey;
    uint32_t *meta;
    int32_t *core;
    uint64_t *qn_ol, *qdig;
    uint8_t *rdeep;
    int32_t *dlist;
    int64_t n_deep;
    int32_t *ext;
    int32_t n_ext;
} cc_records;

/* ---------------------------------------------------------- output spec */
#define CC_OUT_RAW 0     /* copy the source record unchanged */
#define CC_OUT_RENAME 1  /* source record with qname replaced (SSCS_maker.py:319-321) */
#define CC_OUT_NEW 2     /* new consensus record on the template (create_aligned_segment) */

typedef struct cc_out_spec {
    int32_t kind;
    int32_t src_file;   /* index into the srcs[] array passed to ccio_write_bam */
    int64_t src_rec;    /* record (template) index in that file */
    int64_t name_id;    /* index into the names blob (kinds 1, 2) */
    int32_t flag, mapq, tlen, rg_id;  /* kind 2 */
    int64_t cons_off;   /* kind 2: qual at cons_qual+cons_off, seq nibbles at cons_seq+cons_off/2 */
    int32_t cons_len;   /* kind 2 */
    int32_t pad;
} cc_out_spec;

/* ================================================================ libccio */
typedef struct ccio_interner ccio_interner;
typedef struct ccio_bam ccio_bam;

const char *ccio_last_error(void);
ccio_interner *ccio_interner_new(void);
void ccio_interner_free(ccio_interner *it);
int64_t ccio_interner_size(ccio_interner *it, int kind);               /* 0 barcode, 1 cigar, 2 RG */
int ccio_interner_get(ccio_interner *it, int kind, int64_t id, char *buf, int buflen);
int32_t ccio_interner_intern(ccio_interner *it, int kind, const char *s);
int64_t ccio_interner_swap_table(ccio_interner *it, int32_t *out, int64_t cap); /* duplex_tag barcode swap */

ccio_bam *ccio_bam_open(const char *path, int nthreads);
void ccio_bam_close(ccio_bam *b);
int64_t ccio_bam_nrec(ccio_bam *b);
int32_t ccio_bam_nref(ccio_bam *b);
int ccio_bam_ref(ccio_bam *b, int32_t i, char *name, int cap, int32_t *len);
int ccio_bam_qname(ccio_bam *b, int64_t i, char *buf, int cap);
int ccio_bam_layout(ccio_bam *b, uint64_t *qn_bytes, uint64_t *pay_bytes, int32_t *max_len, int nthreads);
/* mode 0: SSCS barcode = qname.split(delim)[1]; mode 1: duplex barcode = qname.split('_')[0] */
int ccio_bam_decode(ccio_bam *b, ccio_interner *it, int mode, const char *delim, cc_records *out, int nthreads);
/* The slim decode in front of the device unpacker (cc_table_unpack).  Fills, per record, out's tid,
 * pos, mtid, mpos, tlen, flag, mapq, lseq, qlen, qn_len, the interned cigar_id / bc_id / rg_id
 * (ccio_bam_decode's interner, modes and delimiter rules) and rflags (all three bits), and nothing
 * else: payload, qn_blob, qn_off, pay_off, rdig and the derived columns are not touched and may be
 * NULL.  *stream / *stream_bytes: the handle's records as one contiguous stream, block_size first;
 * it points into the handle (its own stream, or a packed copy for a combined view) and stays valid
 * until the handle is closed or decoded again.  rec_off[n]: each record's offset in the stream
 * (rec_off[i] + 4 + block_size = rec_off[i + 1]; the last one ends at stream_bytes).  *max_len: the
 * largest l_seq.  -1 (ccio_last_error names the record) for a record whose lengths do not fit its
 * block_size (csrc/unpack_core.h's refusals). */
int ccio_bam_decode_ids(ccio_bam *b, ccio_interner *it, int mode, const char *delim, cc_records *out, int nthreads,
                        const uint8_t **stream, uint64_t *stream_bytes, uint64_t *rec_off, int32_t *max_len);
/* ccio_bam_decode_ids without the string pass, in front of the device interner (cc_table_ids): the
 * same columns, stream, rec_off and max_len, but cigar_id / bc_id / rg_id are not touched and rflags
 * holds the parser's bit (CC_RF_QUAL_MISSING) only. */
int ccio_bam_decode_cols(ccio_bam *b, cc_records *out, int nthreads, const uint8_t **stream, uint64_t *stream_bytes,
                         uint64_t *rec_off, int32_t *max_len);
/* The host's part of the device interner: cc_table_ids' local ids turned into the interner's.  Per
 * table k (0 barcode, 1 cigar, 2 RG), in local-id order, the string of record first[k][j] (j < nd[k])
 * is extracted by ccio_bam_decode's own code and interned (under the interner's mutex): new strings
 * take the next ids in order of first occurrence, as ccio_bam_decode_ids gives them; then
 * bc_id / cigar_id / rg_id[n] = local[k][i] < 0 ? -1 : that string's id.  -1 (ccio_last_error) for a
 * first record outside the handle, one in which the host finds no string, or a local id outside
 * [0, nd[k]). */
int ccio_intern_first(ccio_bam *b, ccio_interner *it, int mode, const char *delim, const int32_t *const *first,
                      const int32_t *nd, const int32_t *const *local, int64_t n, int32_t *bc_id, int32_t *cigar_id,
                      int32_t *rg_id, int nthreads);
/* test entry: the device interner's key finders (csrc/intern_core.h) run on the host over b's n
 * records.  Table k's record r at [k * n + r]: the key's offset from the record's block_size word,
 * its length, and none (no key: id -1); flags[n]: CC_RF_BAD_SPACER | CC_RF_RG_UNSUPPORTED as they
 * apply; refuse[n]: 1 for a record the finders refuse.  -1 for a delimiter of more than 16 bytes. */
int ccio_intern_keys(ccio_bam *b, int mode, const char *delim, uint32_t *off, uint32_t *len, uint8_t *none,
                     uint8_t *flags, uint8_t *refuse);

/* sscs_qname fields (9 int32 per name: bc, tidLo, posLo, tidHi, posHi, cigA, cigB,
 * strand(0 pos/1 neg/2 None), |tlen|) + ':' + suffix.  blob NULL = size query. */
int64_t ccio_format_csn_names(ccio_interner *it, int64_t n, const int32_t *f9, const int64_t *suffix,
                              char *blob, int64_t cap, int64_t *off);
int ccio_dcs_name(const char *tag, const char *ds, char *out, int cap);
/* duplex_tag(tag) (consensus_helper.py:639-683): barcode halves swapped around the first '.' (else at
 * len // 2), field 8 R1 <-> R2 (anything but R1 -> R1).  Returns the length (snprintf), -1 for fewer
 * than 9 '_' fields (the reference's IndexError). */
int ccio_duplex_tag(const char *tag, char *out, int cap);
int64_t ccio_format_dcs_names(ccio_bam *b, int64_t n, const int64_t *rec_tag, const int64_t *rec_ds,
                              char *blob, int64_t cap, int64_t *off);
/* 1 when every name ccio_format_dcs_names reads for these pairs (l_read_name - 1 bytes) holds no NUL and
 * is terminated, so that it is the bytes a record table keeps (its qn_len is a strnlen); 0 when one
 * is not; -1 for a record index outside b. */
int ccio_dcs_names_plain(ccio_bam *b, int64_t n, const int64_t *rec_tag, const int64_t *rec_ds);
/* An interner table's strings side by side: off[0 .. ccio_interner_size] their offsets, string i is
 * blob[off[i], off[i + 1]).  Returns the bytes in all; blob NULL: the offsets only; -1 when cap is short. */
int64_t ccio_interner_blob(ccio_interner *it, int kind, char *blob, int64_t cap, int64_t *off);
int ccio_write_bam(const char *path, ccio_bam *tmpl, ccio_interner *it, int64_t n, const cc_out_spec *spec,
                   ccio_bam *const *srcs, int nsrc, const char *names, const int64_t *name_off,
                   const uint8_t *cons_seq, const uint8_t *cons_qual, int level, int nthreads);
int ccio_sort_bam(const char *in_path, const char *out_path, int level, int nthreads);
int ccio_merge_bams(const char *out_path, const char *const *in_paths, int nin, int level, int nthreads);
/* Writer flags of the orchestrator's fused steps (ConsensusCruncher.py:10-34 sort_index: the stage
 * output sorted and indexed as it is written, instead of written, re-read, sorted and re-read again
 * for the index).  CCIO_W_SORT: records in samtools-sort order (tid, pos, is_reverse; ties keep the
 * written order); CCIO_W_INDEX: also <path>.bai.  keep (non-null) receives a handle over the written
 * records, as ccio_bam_open(path) would return it. */
#define CCIO_W_SORT 1
#define CCIO_W_INDEX 2
/* CCIO_W_ASYNC: the file (and its index) is compressed and written by a thread of its own after the
 * call returns (the kept handle is usable at once); an entry point reading that path, or writing
 * it again, waits for it first; ccio_flush waits for all and reports the first failure */
#define CCIO_W_ASYNC 4
/* CCIO_W_MEMORY: no file at all; keep (required) receives the records, sorted under CCIO_W_SORT (the
 * multi-GPU driver keeps every stage output in memory and writes only the final files) */
#define CCIO_W_MEMORY 8
int ccio_flush(void);
/* An alternative encoder for the writers' BGZF members (the device encoder: cc_bgzf_hook below).
 * The writers cut a stream into pieces of at most 0xff00 bytes and compress them in rounds; with a
 * hook set, a round at level >= 1 goes to fn first:
 *   data, n   the round's bytes (pieces: ceil(n / 0xff00), the last one shorter);
 *   stage     piece j's whole member (18-byte header, raw DEFLATE, CRC32, ISIZE) goes to
 *             stage + j * slot (slot >= 65536);  out_len[j] = its size, 28..65536.
 * fn returns 0 when every member is written.  On any other return, or a member whose size or
 * BSIZE / ISIZE fields do not fit its piece, the host encoder compresses that round: a file is
 * never lost or left partial.  Level 0 never reaches fn.  fn is called from the CCIO_W_ASYNC
 * writer threads, several at once.  NULL unsets the hook; unset it before freeing what user
 * points to (after ccio_flush). */
typedef int (*ccio_deflate_fn)(void *user, const uint8_t *data, uint64_t n, uint8_t *stage, uint64_t slot,
                               uint32_t *out_len, int64_t pieces);
void ccio_set_deflate_hook(ccio_deflate_fn fn, void *user);
/* An alternative inflater for the readers' BGZF members (the device inflater: cc_bgzf_inflate_hook
 * below).  With a hook set, the whole-file open, the region reads and the header read hand their
 * non-empty members to fn first:
 *   comp, coff[j], clen[j]   member j's raw DEFLATE payload is comp[coff[j] .. coff[j] + clen[j]);
 *   out, uoff[j], ulen[j]    its ulen[j] (ISIZE) bytes go to out[uoff[j] .. uoff[j] + ulen[j]);
 *                            fn writes nowhere else in out;
 *   ok[j]                    1 when fn inflated member j, 0 when it did not.
 * fn returns 0 when ok[] is filled in.  libccio then compares the member's CRC32 field with the CRC
 * of the bytes fn wrote (the host path checks no CRCs).  A member with ok[j] == 0 or another CRC,
 * and every member after a nonzero return, is inflated by the host codec: a file is never misread
 * because of the hook, and a member the host codec cannot inflate either gives the error it gives
 * without one.  fn is called from any thread, several at once.  NULL unsets the hook; unset it
 * before freeing what user points to. */
typedef int (*ccio_inflate_fn)(void *user, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                               const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out, uint8_t *ok);
void ccio_set_inflate_hook(ccio_inflate_fn fn, void *user);
/* The inflate hook that also keeps what it inflated (the device inflater's resident streams:
 * cc_bgzf_inflate_keep_hook below).  Only the whole-file open (ccio_bam_open) uses it, in place of
 * the plain hook; the region reads, the header read and ccio_index_bam keep to the plain one.  keep
 * has ccio_inflate_fn's contract and also receives total, the inflated file's size; through *token
 * it names its copy of the file, in which every member with ok[j] == 1 lies at uoff[j] (0: it kept
 * none).  After the CRC checks libccio sends every member the host codec inflated instead (ok[j] ==
 * 0, or another CRC) through patch(user, token, off, bytes, n): the copy's [off, off + n) becomes
 * bytes[0 .. n).  When keep returns nonzero or a patch fails, the handle carries no token and the
 * open proceeds as with the plain hook.  libccio never frees a token: closing a handle calls nothing.
 * NULL keep unsets the pair. */
typedef int (*ccio_inflate_keep_fn)(void *user, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                                    const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out,
                                    uint8_t *ok, uint64_t total, int64_t *token);
typedef int (*ccio_resident_patch_fn)(void *user, int64_t token, uint64_t off, const uint8_t *bytes, uint64_t n);
void ccio_set_inflate_keep_hook(ccio_inflate_keep_fn keep, ccio_resident_patch_fn patch, void *user);
/* The two inflate hooks with a CRC of their own (the device CRC32: cc_bgzf_inflate_crc_hook and
 * cc_bgzf_inflate_keep_crc_hook below): the types above plus a trailing crc, where the hook leaves
 * crc[j] = the CRC32 of the bytes it produced for member j (read only where ok[j] == 1).  While a crc
 * hook is set it takes its plain sibling's place, whether or not that one is set too, and libccio
 * accepts member j when ok[j] == 1 and crc[j] equals the member's CRC32 field; it computes no CRC over
 * out.  Every other rule is the plain hooks': a refused member, a member whose CRC differs and every
 * member after a nonzero return are inflated by the host codec, and those of a kept copy go through
 * patch.  The trust this implies: the verdict is about the hook's own bytes (for the device inflater,
 * the bytes in device memory, which with a kept copy are the bytes the unpacker reads); that out
 * holds the same bytes is the hook's word, no longer checked here.  NULL unsets a crc hook and its
 * plain sibling, if set, serves again. */
typedef int (*ccio_inflate_crc_fn)(void *user, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                                   const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out, uint8_t *ok,
                                   uint32_t *crc);
typedef int (*ccio_inflate_keep_crc_fn)(void *user, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                                        const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out,
                                        uint8_t *ok, uint64_t total, int64_t *token, uint32_t *crc);
void ccio_set_inflate_crc_hook(ccio_inflate_crc_fn fn, void *user);
void ccio_set_inflate_keep_crc_hook(ccio_inflate_keep_crc_fn keep, ccio_resident_patch_fn patch, void *user);
/* 1, with the keep hook's token and the offset of b's first record in the inflated file (where its
 * records end for a file without any), when b came from ccio_bam_open with the keep hook set and its
 * records are still that stream's own; 0 for views, combined handles and region opens. */
int ccio_bam_resident(ccio_bam *b, int64_t *token, uint64_t *base);
/* An alternative assembler for ccio_write_bam_ex's records (the device assembler: cc_bam_assemble_hook
 * below).  With a hook set, a write whose source handles all hold their records in place and in order
 * in their own streams (ccio_bam_resident's condition on the records; views from ccio_bam_combine /
 * ccio_bam_route never reach the hook) goes to fn first:
 *   header, header_bytes    the output's encoded header;
 *   srcs[nsrc]              each source's records: its stream (block_size first), their offsets in it
 *                           and, when ccio_bam_resident names one, the keep hook's token and the offset
 *                           of the first record in that copy;
 *   spec[n], names, name_off, n_names, names_bytes, rg_blob, rg_off[n_rg + 1], flags (CCIO_W_SORT)
 *                           ccio_write_bam_ex's own; the RG values side by side;
 *   cons_seq, cons_qual     the caller's arrays with the extent the specs use, or both NULL when the
 *                           caller passed none (the hook then brings its own: cc_bam_assemble_group);
 *   alloc(actx, total)      called once, after fn knows the stream's size: the buffer the stream goes to;
 *   at[n + 1], *total       each output record's offset in the stream, at[n] = *total = its size.
 * fn returns 0 when the whole stream (header, then the records) is written.  libccio then checks, in
 * one parallel pass, that at[0] is the header's size, at is strictly increasing, every record's
 * block_size + 4 is at[i + 1] - at[i] and at[n] is the total.  On any other return or a failed check
 * the host assembles the records exactly as without a hook: a file is never lost.  NULL unsets it. */
typedef struct cc_asm_src {
    const uint8_t *stream;   /* the records in host memory; may be NULL for a resident source */
    uint64_t bytes;          /* their size */
    int64_t resident_id;     /* the resident stream (cc_bgzf_inflate_keep) holding them, 0: none; with a
                              * host stream as well, the resident one is read while it still exists */
    uint64_t base;           /* where they start in it */
    const uint64_t *rec_off; /* nrec offsets, from stream / base */
    int64_t nrec;
} cc_asm_src;
typedef uint8_t *(*cc_asm_alloc_fn)(void *actx, uint64_t total);
typedef int (*ccio_assemble_fn)(void *user, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs,
                                int32_t nsrc, const cc_out_spec *spec, int64_t n, const char *names,
                                const int64_t *name_off, int64_t n_names, uint64_t names_bytes, const uint8_t *cons_seq,
                                uint64_t cons_seq_bytes, const uint8_t *cons_qual, uint64_t cons_qual_bytes,
                                const char *rg_blob, const int64_t *rg_off, int32_t n_rg, int flags,
                                cc_asm_alloc_fn alloc, void *actx, uint64_t *at, uint64_t *total);
void ccio_set_assemble_hook(ccio_assemble_fn fn, void *user);
/* What the BAI needs of one record (csrc/index_core.h): rl holds the reference length (the M / D / N /
 * = / X op lengths summed, 0 for an unmapped record, saturating at 2^31 - 1) in bits 0..30 and the
 * record's flag & 4 in bit 31. */
typedef struct cc_index_field {
    int32_t tid, pos;
    uint32_t block_size;
    uint32_t rl;
} cc_index_field;
/* The output stream kept where the assembler built it (the device: cc_out_resident_hooks below).
 * With the set installed, ccio_write_bam_ex goes to it in place of the plain assemble hook, under
 * the same condition on the sources:
 *   assemble_keep   ccio_assemble_fn's contract, plus need_host and *token.  It leaves the stream in
 *                   a place of its own named by *token (> 0) and always fills at[n + 1] and *total;
 *                   it calls alloc and writes the stream to the host only when need_host is 1, which
 *                   it is exactly when the caller asked for a kept handle or for CCIO_W_MEMORY.
 *   deflate         ccio_deflate_fn with (token, off) in place of data: the members of the stream's
 *                   bytes [off, off + n).  off is a multiple of 0xff00 * 1024 (the writers' round).
 *   index_fields    fields[i] for the record at at[i], i < n; nonzero when any record is refused.
 *   fetch           the stream's bytes [off, off + n) copied to dst.
 *   release         the token is dead: called exactly once per token assemble_keep returned, by the
 *                   thread that finished (or gave up) the file; for CCIO_W_ASYNC the writer thread.
 * Without a host copy libccio fetches and compares the header's bytes, checks at[0], that at is
 * strictly increasing and at[n] == total, and (from index_fields) every record's block_size + 4
 * against at[i + 1] - at[i]; with a host copy the plain hook's checks run as well.  When
 * assemble_keep returns nonzero or a check fails, the token (if any) is released and the write goes
 * on to the plain assemble hook or the host assembler, exactly as without the set.  Every encoder
 * round at level >= 1 goes to deflate first, with the plain deflate hook's checks on what it
 * returns; a round it refuses is fetched and compressed by the host codec.  With CCIO_W_INDEX the
 * .bai is built from the fields, byte for byte what the walk over the stream writes; when
 * index_fields refuses, the stream is fetched and walked.  A file is never lost or left partial.
 * A kept handle owns only its host copy.  The callbacks are called from the CCIO_W_ASYNC writer
 * threads, several at once.  NULL cb unsets the set; unset it (after ccio_flush) before freeing
 * what user points to. */
typedef int (*ccio_assemble_keep_fn)(void *user, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs,
                                     int32_t nsrc, const cc_out_spec *spec, int64_t n, const char *names,
                                     const int64_t *name_off, int64_t n_names, uint64_t names_bytes,
                                     const uint8_t *cons_seq, uint64_t cons_seq_bytes, const uint8_t *cons_qual,
                                     uint64_t cons_qual_bytes, const char *rg_blob, const int64_t *rg_off, int32_t n_rg,
                                     int flags, cc_asm_alloc_fn alloc, void *actx, int need_host, uint64_t *at,
                                     uint64_t *total, int64_t *token);
typedef int (*ccio_deflate_resident_fn)(void *user, int64_t token, uint64_t off, uint64_t n, uint8_t *stage,
                                        uint64_t slot, uint32_t *out_len, int64_t pieces);
typedef int (*ccio_index_fields_fn)(void *user, int64_t token, const uint64_t *at, int64_t n, cc_index_field *fields);
typedef int (*ccio_resident_fetch_fn)(void *user, int64_t token, uint64_t off, uint64_t n, uint8_t *dst);
typedef void (*ccio_resident_release_fn)(void *user, int64_t token);
typedef struct ccio_out_resident {
    ccio_assemble_keep_fn assemble_keep;
    ccio_deflate_resident_fn deflate;
    ccio_index_fields_fn index_fields;
    ccio_resident_fetch_fn fetch;
    ccio_resident_release_fn release;
} ccio_out_resident;
void ccio_set_out_resident(const ccio_out_resident *cb, void *user);
/* b's records (which must lie in place in its own stream, ccio_bam_resident's condition) named as
 * bytes [base, ...) of the resident copy `token`: ccio_bam_resident then answers with them and the
 * assemble hooks read that copy (cc_resident_put uploads one).  Token 0 clears it.  -1 for a view. */
int ccio_bam_set_resident(ccio_bam *b, int64_t token, uint64_t base);
/* the stream of a handle whose records lie in place (what cc_resident_put uploads for it): its bytes
 * and the offset of its first record in them (its size without records); -1 for a view */
int ccio_bam_stream(ccio_bam *b, const uint8_t **data, uint64_t *bytes, uint64_t *rec_base);
/* per value 0..maxv of v[0..n): count and first index (n when absent), one pass (read_families.txt) */
int ccio_value_census(const int32_t *v, int64_t n, int32_t maxv, int64_t *first, int64_t *count);
/* (cons_seq and cons_qual both NULL with CC_OUT_NEW specs: only an assemble hook that brings its own
 * consensus arrays can write the file; when it does not, nothing is written and the result is -2.
 * names NULL means "the names are with the hook" (cc_bam_assemble_names): name_off stays a host array,
 * from which the hooks' n_names and names_bytes are derived, and the hooks receive names as NULL.  When
 * no hook takes such a write and a spec of kind RENAME or NEW has name_id >= 0, nothing is written and
 * the result is -3, "write_bam: names not in host memory"; specs that need no name are written by the
 * host as always) */
int ccio_write_bam_ex(const char *path, ccio_bam *tmpl, ccio_interner *it, int64_t n, const cc_out_spec *spec,
                      ccio_bam *const *srcs, int nsrc, const char *names, const int64_t *name_off,
                      const uint8_t *cons_seq, const uint8_t *cons_qual, int level, int nthreads, int flags,
                      ccio_bam **keep);
int ccio_sort_bam_ex(const char *in_path, const char *out_path, int level, int nthreads, int flags);
/* samtools merge of coordinate-sorted record sets held in memory (ties keep input order) */
int ccio_merge_handles(const char *out_path, ccio_bam *const *ins, int nin, int level, int nthreads, int flags,
                       ccio_bam **keep);
/* An alternative merger for ccio_merge_handles (the device merge: cc_bam_merge_hooks below, or any
 * functions with its contract).  merge receives the header, the inputs as cc_asm_src (as the assemble
 * hook receives its sources) and alloc / actx for the stream; it fills at[n + 1] (the output records'
 * offsets, n the inputs' records together), org[n] (each output record's index in the concatenation
 * of the inputs) and *total.  keep is the same plus need_host and *token: the stream stays in a place
 * of its own named by *token (> 0), which then belongs to the resident output set's deflate,
 * index_fields, fetch and release (ccio_set_out_resident); alloc is called only when need_host is 1.
 * ccio_merge_handles goes to the hooks only when every input holds its records in place and in
 * order in its own stream (views from ccio_bam_combine / ccio_bam_route never do), there are at most
 * 8 inputs and every input is in key order; it tries keep first when the resident output set is
 * installed, then merge, then merges on the host as without hooks.  What a hook returns is checked
 * against the host records in one parallel pass: at[0] is the header's size, at is strictly
 * increasing and at[n] == total; org is a permutation of 0..n-1; along the output the keys are
 * non-decreasing and equal keys have increasing org (input order, then record order);
 * at[i + 1] - at[i] is 4 + block_size of record org[i]; with a host copy the header's bytes and every
 * record's block_size word are compared, without one the fetched header bytes and the index_fields
 * block sizes.  The first failure releases the token (if any) and the merge goes on to the next
 * path: a file is never lost.  NULL unsets a hook. */
typedef int (*ccio_merge_fn)(void *user, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs,
                             int32_t nsrc, cc_asm_alloc_fn alloc, void *actx, uint64_t *at, uint32_t *org,
                             uint64_t *total);
typedef int (*ccio_merge_keep_fn)(void *user, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs,
                                  int32_t nsrc, cc_asm_alloc_fn alloc, void *actx, int need_host, uint64_t *at,
                                  uint32_t *org, uint64_t *total, int64_t *token);
void ccio_set_merge_hooks(ccio_merge_fn merge, ccio_merge_keep_fn keep, void *user);
/* records of the inputs in file order, one file after the other (sharded stage parts, rank order) */
int ccio_concat_bams(const char *out_path, const char *const *in_paths, int nin, int level, int nthreads);
/* <path>.bai for a coordinate-sorted BAM (samtools index, ConsensusCruncher.py:10-34) */
int ccio_index_bam(const char *path);
/* fastq2bam's UMI extraction (extract_barcodes.py:144-481; replaces its per-pair loop :287-405).
 * pattern (N = barcode base, A/C/G/T = spacer) or, with pattern NULL, the barcode list blist[nblist]
 * (distinct entries; the reference's --skipcheck path).  Writes <out_prefix>_barcode_R1.fastq and
 * _R2.fastq (list mode also _r1/_r2_bad_barcodes.txt).  counts[4] = read pairs, missing spacer, bad
 * barcodes, passing; r1_hist/r2_hist: pattern mode plen x 5 (A,C,G,T,N per barcode position), list
 * mode one count per list entry; *n_written = pairs written before a stop.  Returns 0, -1 (I/O or
 * FASTQ format), -2 (read ids differ: the reference's AssertionError at :291, earlier pairs written)
 * or -3 (a read shorter than the barcode). */
int ccio_extract_barcodes(const char *read1, const char *read2, const char *out_prefix, const char *pattern,
                          const char *const *blist, int32_t nblist, int nthreads, int64_t *counts,
                          int64_t *r1_hist, int64_t *r2_hist, int64_t *n_written);
/* The same extraction with the per-pair decisions made on the GPU (cc_extract_barcodes): the FASTQs
 * read and indexed, stopping where the reference stops (ids differ at a pair: *stop = -2; pattern
 * mode, a read shorter than min_len: -3); the first `width` bases of each pair's reads; the outputs
 * written from the decisions (status 0: passing, header barcode bc + i * bc_stride (NUL terminated),
 * reads cut by cut1 / cut2; list mode, bad-barcode lines per read mask: bit j the prefix of length
 * min(lens[j], read length), bit 31 that of the last length once more). */
typedef struct ccio_fq ccio_fq;
ccio_fq *ccio_fq_open(const char *read1, const char *read2, int32_t min_len, int nthreads);
void ccio_fq_close(ccio_fq *f);
int ccio_fq_info(ccio_fq *f, int64_t *n, int32_t *stop);
int ccio_fq_heads(ccio_fq *f, int32_t width, uint8_t *h1, uint8_t *h2, int32_t *len1, int32_t *len2);
int ccio_fq_write(ccio_fq *f, const char *out_prefix, int list_mode, const uint8_t *status, const char *bc,
                  int32_t bc_stride, const int32_t *cut1, const int32_t *cut2, const uint32_t *bad1,
                  const uint32_t *bad2, const int32_t *lens, int32_t nlens, int nthreads);
/* rank-local record sets of the multi-GPU driver (consensuscruncher_amd/sharded.py) */
/* records with tid == tid[i] and beg[i] <= pos < end[i] for some region i (pysam region fetch +
 * consensus_helper.py:391-396), file order, each once; only the blocks <path>.bai names are read */
ccio_bam *ccio_bam_open_regions(const char *path, int32_t n, const int32_t *tid, const int64_t *beg,
                                const int64_t *end, int nthreads);
int ccio_bam_cores(ccio_bam *b, int32_t *tid, int32_t *pos, int32_t *mtid, int32_t *mpos, uint16_t *flag);
/* raw records idx[0..n) concatenated, block_size first; out NULL: size query */
int64_t ccio_bam_pack(ccio_bam *b, int64_t n, const int64_t *idx, uint8_t *out, int64_t cap);
/* parts' records, then the blobs' raw records, stably sorted by key (0: tid,pos; 1: samtools sort
 * stand-in tid,pos,is_reverse; 2: none); header from tmpl or parts[0].  A view: the parts' records
 * are not copied (their streams live with the new handle; the parts may be closed first) */
ccio_bam *ccio_bam_combine(ccio_bam *tmpl, ccio_bam *const *parts, int32_t n, const uint8_t *const *blobs,
                           const int64_t *blob_bytes, int32_t nb, int key, int nthreads);
int ccio_bam_origin(ccio_bam *b, int64_t *out);   /* each record's input index in its combine */
int ccio_bam_write_all(const char *path, ccio_bam *b, int level, int nthreads);
/* b's stream written to path with the writer flags CCIO_W_INDEX (b in samtools-sort order) and
 * CCIO_W_ASYNC (b waits for the write before it is freed) */
int ccio_bam_write_ex(const char *path, ccio_bam *b, int level, int nthreads, int flags);
/* a rank's part of a routed record set (sharded.py): the blobs' records with own's records that have
 * keep[i] != 0 placed before blob own_at (sender order), stably sorted by key (as ccio_bam_combine;
 * keep NULL: all of own's); a view of own's records, as ccio_bam_combine */
ccio_bam *ccio_bam_route(ccio_bam *own, const uint8_t *keep, int32_t own_at, const uint8_t *const *blobs,
                         const int64_t *blob_bytes, int32_t nb, int key, int nthreads);
/* the multi-GPU driver's sends of a rank's own stream entries (sharded.Geometry.sent): per entry the
 * bed region of its mate's position (sorted non-overlapping intervals iv_lo <= tid<<32|pos < iv_hi of
 * region iv_reg), its owner rank by the world-1 cuts (cut_r, cut_k) into to (-1: no region), and
 * send = the mate is streamed later by another rank */
int ccio_stream_sent(int64_t n, const int32_t *rec, const int32_t *reg, const int32_t *tid, const int32_t *pos,
                     const int32_t *mtid, const int32_t *mpos, int32_t niv, const int64_t *iv_lo, const int64_t *iv_hi,
                     const int32_t *iv_reg, int32_t ncut, const int64_t *cut_r, const int64_t *cut_k, int32_t rank,
                     uint8_t *send, int64_t *to);
/* 1 when b's records are in key order (0: tid, pos, unmapped last; 1: samtools sort's), else 0 */
int ccio_bam_is_sorted(ccio_bam *b, int key);
/* the bed-region stream of (tid, pos)-sorted records for regions r0 <= r < r1 (bed order): records with
 * tid == rtid[r] and max(rbeg[r], 0) <= pos < max(rend[r], 0), in record order, and their regions;
 * returns the count (out_rec NULL: count only), -1 when the records are not sorted */
int64_t ccio_region_stream(int64_t n, const int32_t *tid, const int32_t *pos, int32_t r0, int32_t r1,
                           const int32_t *rtid, const int64_t *rbeg, const int64_t *rend, int32_t *out_rec,
                           int32_t *out_reg);
int64_t ccio_bai_mapped(const char *path);        /* AlignmentFile.mapped from <path>.bai */
int ccio_bai_region_bytes(const char *path, int32_t n, const int32_t *tid, const int64_t *beg, const int64_t *end,
                          int64_t *out);          /* compressed bytes per region: shard-plan weights */
int ccio_write_columns(const char *path, const char *header_text, int32_t nref, const char *const *ref_names,
                       const int32_t *ref_lens, int64_t n, const int32_t *tid, const int32_t *pos,
                       const int32_t *mtid, const int32_t *mpos, const int32_t *tlen, const uint16_t *flag,
                       const uint8_t *mapq, const uint8_t *qn_blob, const int64_t *qn_off, const int32_t *cig_id,
                       const uint32_t *cig_ops, const int64_t *cig_off, int32_t read_len, const uint8_t *seq_ascii,
                       const uint8_t *qual, const int32_t *rg_id, const char *const *rg_vals, int level,
                       int nthreads);

/* ================================================================ libccamd */
typedef struct cc_ctx cc_ctx;

/* counters written by cc_read_bam (consensus_helper.py:383-387, 506) */
enum {
    CC_CNT_COUNTER = 0,       /* records fetched minus is_unmapped */
    CC_CNT_UNMAPPED,          /* is_unmapped */
    CC_CNT_UNMAPPED_MATE,     /* flag in {73,89,121,153,185,137} */
    CC_CNT_MULTIPLE_MAPPING,  /* secondary + supplementary */
    CC_CNT_BAD_SPACER,
    CC_CNT_PAIRS,             /* completed pairs */
    CC_CNT_READ_ENDS,         /* read ends (2 per pair) */
    CC_CNT_FAMILIES,          /* tags (tag_dict entries) */
    CC_CNT_ENTRIES,           /* csn_pair_dict entries */
    CC_CNT_UNPAIRED,          /* pair_dict leftovers */
    CC_CNT_ORPHAN_TAGS,       /* tags beyond two per consensus tag ("NOT UNIQUE") */
    CC_CNT_DROPPED,           /* "line read twice" drops (tag equal to its mate's tag) */
    CC_CNT_BAD_LISTED,        /* records routed to badReads */
    CC_CNT_FOREIGN,           /* stream entries counted on another shard (moved / foreign entries) */
    CC_NUM_COUNTERS = 16
};

typedef struct cc_read_bam_params {
    int32_t delim_filter;  /* SSCS: qname without delimiter is a bad read */
    int32_t badread_file;  /* 1: filtered records go to badReads and are not paired (SSCS) */
    int32_t scope_by_run;  /* singleton_correction's SSCS side: dicts reset per chromosome run */
    int32_t coord_sorted;  /* table is coordinate-sorted (tid, pos): group tags per position group */
    uint64_t seed;         /* hash seed (retry with another on CC_E_COLLISION) */
} cc_read_bam_params;

int cc_create(int device_id, cc_ctx **ctx);
int cc_destroy(cc_ctx *ctx);
const char *cc_last_error(cc_ctx *ctx);
void *cc_host_alloc(cc_ctx *ctx, uint64_t bytes);   /* pinned host memory */
void cc_host_free(cc_ctx *ctx, void *p);
int cc_set_profiling(cc_ctx *ctx, int on);
/* restrict profiling to the newline-separated kernel scopes in names (NULL or "": all) */
int cc_profile_only(cc_ctx *ctx, const char *names);
/* name, total ms, launches for every profiled kernel: returns count */
int cc_kernel_times(cc_ctx *ctx, char *names, int names_cap, double *ms, int64_t *launches, int cap);
int cc_synchronize(cc_ctx *ctx);
/* BGZF members on the device (k_bgzf_deflate: one workgroup per piece; hash matching, a greedy
 * parse, and the smallest of a stored, a fixed-Huffman and a dynamic-Huffman block).  data[0..n) is
 * cut at every 0xff00 bytes; piece j's framed member goes to stage + j * slot (slot >= 65536) and
 * out_len[j] gets its size (<= 65536).  Returns the member count, ceil(n / 0xff00) (0 for n == 0),
 * or a negative CC_E_*; more pieces than cap is CC_E_INVALID.  The same bytes give the same
 * members on every call.  The encoder has its own streams and buffers and serialises concurrent
 * callers: it may run from any thread while the context's stream is busy.  With profiling on, the
 * kernel's time is reported by cc_kernel_times as "bgzf_deflate", its copies as "bgzf_upload" and
 * "bgzf_download". */
int64_t cc_bgzf_deflate(cc_ctx *ctx, const uint8_t *data, uint64_t n, uint8_t *stage, uint64_t slot,
                        uint32_t *out_len, int64_t cap);
/* the pair to hand to ccio_set_deflate_hook; unset the hook before cc_destroy */
int cc_bgzf_hook(cc_ctx *ctx, ccio_deflate_fn *fn, void **user);
/* The encoder's effort: 1 (the default: one candidate per hash from earlier 512-position tiles, a
 * greedy parse) or 2 (buckets of the four most recent positions per hash, entered 64 positions at a
 * time so that a position also sees its own tile, and a one-step lazy parse: smaller members, a
 * slower kernel, one workgroup per CU).  Anything else is CC_E_INVALID and changes nothing.  The
 * setting holds for later cc_bgzf_deflate calls and hook rounds of this context; a round that is
 * running finishes at the effort it started with (the call waits for it).  Either effort gives the
 * same members for the same bytes on every call. */
int cc_bgzf_set_effort(cc_ctx *ctx, int effort);
/* Raw DEFLATE members inflated on the device (k_bgzf_inflate: one wave per member, many members in
 * flight; the decode tables, a ring of the compressed bytes and the last 32 KiB of output live in
 * LDS).  Member j is comp[coff[j] .. coff[j] + clen[j]) and must inflate to exactly ulen[j] bytes,
 * which go to out[uoff[j] .. uoff[j] + ulen[j]); nothing else in out is written.  ok[j] = 1 for a
 * good member, 0 for one the device refused: corrupt (a distance before the first byte, an
 * over-subscribed or incomplete code, symbols 286 / 287 / 30 / 31, LEN != ~NLEN, no final block, more
 * or fewer bytes than ulen[j]) or larger than a BGZF member (clen or ulen over 65536).  What a
 * refused member's range of out holds is unspecified.  Returns the number of members with
 * ok == 0, or a negative CC_E_*.  Rounds of at most 1024 members alternate between the encoder's
 * two streams; concurrent callers are serialised.  With profiling on, cc_kernel_times reports the
 * kernel as "bgzf_inflate" and its copies as "bgzf_in_upload" and "bgzf_in_download". */
int64_t cc_bgzf_inflate(cc_ctx *ctx, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                        const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out, uint8_t *ok);
/* the pair to hand to ccio_set_inflate_hook; unset the hook before cc_destroy */
int cc_bgzf_inflate_hook(cc_ctx *ctx, ccio_inflate_fn *fn, void **user);
/* cc_bgzf_inflate that also leaves the inflated bytes on the device.  out and ok are cc_bgzf_inflate's;
 * in addition every member with ok[j] == 1 lies at [uoff[j], uoff[j] + ulen[j]) of a new resident
 * stream: a device buffer of `total` bytes the context owns, named by *resident_id (> 0), which the
 * kernel writes directly (the rounds' downloads read it).  A refused member's range of it is
 * unspecified until cc_resident_patch fills it.  Every [uoff[j], uoff[j] + ulen[j]) must lie inside
 * total and no two may overlap: otherwise CC_E_INVALID, before any launch.  Without device memory
 * for the stream the call is cc_bgzf_inflate and *resident_id = 0.  cc_destroy frees the streams
 * that are left. */
int64_t cc_bgzf_inflate_keep(cc_ctx *ctx, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                             const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out, uint8_t *ok,
                             uint64_t total, int64_t *resident_id);
/* the pair (and their user) to hand to ccio_set_inflate_keep_hook; unset it before cc_destroy */
int cc_bgzf_inflate_keep_hook(cc_ctx *ctx, ccio_inflate_keep_fn *keep, ccio_resident_patch_fn *patch, void **user);
/* [off, off + n) of a resident stream overwritten from host memory (a member the host codec
 * inflated); done when the call returns.  An id that is unknown, freed or another context's is
 * CC_E_INVALID here and in every call that takes one, and nothing else happens. */
int cc_resident_patch(cc_ctx *ctx, int64_t id, uint64_t off, const uint8_t *bytes, uint64_t n);
int cc_resident_free(cc_ctx *ctx, int64_t id);
/* test hooks: a resident stream's size, at most cap of its bytes copied to dst (NULL: none); the
 * number of resident streams the context holds */
int64_t cc_resident_fetch(cc_ctx *ctx, int64_t id, uint8_t *dst, uint64_t cap);
int64_t cc_resident_count(cc_ctx *ctx);
/* Host bytes uploaded as a new resident stream (*id > 0), with the streams' padding: a stage's source
 * uploaded once for all of its writes (ccio_bam_set_resident names it to the assemble hooks).
 * Without device memory for it CC_E_HIP and *id = 0; the coders stay usable. */
int cc_resident_put(cc_ctx *ctx, const uint8_t *bytes, uint64_t n, int64_t *id);
/* cc_bgzf_deflate over bytes [off, off + n) of resident stream id: k_bgzf_deflate reads its pieces
 * where they lie (no pinned staging copy, no upload; with profiling on nothing is added to
 * "bgzf_upload").  off must be a multiple of 256, the kernel's alignment assumption: anything else,
 * a range outside the stream or an unknown id is CC_E_INVALID.  The members' CRC32 fields always come
 * from k_crc32 over the device bytes, whatever cc_bgzf_set_crc says (there is no host copy to
 * hash).  The same bytes give, byte for byte, cc_bgzf_deflate's members, at either effort.  Runs
 * under the encoder's mutex on its two streams, from any thread. */
int64_t cc_bgzf_deflate_resident(cc_ctx *ctx, int64_t id, uint64_t off, uint64_t n, uint8_t *stage, uint64_t slot,
                                 uint32_t *out_len, int64_t cap);
/* One cc_index_field per record of resident stream id (k_index_fields, csrc/bam_index.hip.inc: a
 * record per lane, index_core.h's arithmetic): record i's block_size word is the stream's byte at[i],
 * at[n + 1] offsets in all.  The records may sit at any byte offset; nothing outside
 * [at[i], at[i + 1]) is looked at.  CC_E_INVALID, cc_last_error naming the first such record, when
 * block_size < 32, at[i] + 4 + block_size != at[i + 1] (offsets out of order or past the stream
 * included) or 32 + l_read_name + 4 * n_cigar_op > block_size; also when at[n] lies past the stream
 * or the id is unknown.  fields then holds nothing of use.  Runs on the coders' first stream under
 * the encoder's mutex, from any thread; with profiling on, cc_kernel_times reports the kernel as
 * "index_fields". */
int cc_index_fields(cc_ctx *ctx, int64_t id, const uint64_t *at, int64_t n, cc_index_field *fields);
/* CRC-32 (zlib's) on the device (k_crc32: one workgroup of 256 threads per segment of at most 65,536
 * bytes at any byte address; slice-by-4 tables and a "through 4,080 zero bytes" operator built in LDS
 * from the polynomial; csrc/crc_core.h holds the arithmetic and the per-lane rule).  crc[i] = the
 * CRC32 of data[off[i] .. off[i] + len[i]) for n ranges, which may overlap and may be of any length:
 * data is uploaded once, a range longer than 65,536 bytes is cut into segments on the host and their
 * CRCs are joined (crc32_combine's arithmetic); an empty range gives 0.  A range outside [0, nbytes)
 * is CC_E_INVALID.  Runs on the encoder's streams, under its mutex and latch, like everything below;
 * with profiling on, cc_kernel_times reports every launch of the kernel as "bgzf_crc32". */
int cc_crc32(cc_ctx *ctx, const uint8_t *data, uint64_t nbytes, const uint64_t *off, const uint64_t *len, int64_t n,
             uint32_t *crc);
/* the same over a resident stream's bytes, in place (no upload) */
int cc_resident_crc32(cc_ctx *ctx, int64_t id, const uint64_t *off, const uint64_t *len, int64_t n, uint32_t *crc);
/* cc_bgzf_inflate and cc_bgzf_inflate_keep with one more output: crc[j] = the CRC32 of the bytes the
 * device wrote for member j, defined where ok[j] == 1 (0 elsewhere).  In every round k_crc32 follows
 * k_bgzf_inflate on the same stream, over the round's descriptors and its output base (the round's
 * buffer, or the resident stream itself), and the values come back with the status words. */
int64_t cc_bgzf_inflate_crc(cc_ctx *ctx, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                            const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out, uint8_t *ok,
                            uint32_t *crc);
int64_t cc_bgzf_inflate_keep_crc(cc_ctx *ctx, const uint8_t *comp, const uint64_t *coff, const uint32_t *clen,
                                 const uint64_t *uoff, const uint32_t *ulen, int64_t members, uint8_t *out, uint8_t *ok,
                                 uint64_t total, int64_t *resident_id, uint32_t *crc);
/* what to hand to ccio_set_inflate_crc_hook and ccio_set_inflate_keep_crc_hook; unset them before cc_destroy */
int cc_bgzf_inflate_crc_hook(cc_ctx *ctx, ccio_inflate_crc_fn *fn, void **user);
int cc_bgzf_inflate_keep_crc_hook(cc_ctx *ctx, ccio_inflate_keep_crc_fn *keep, ccio_resident_patch_fn *patch,
                                  void **user);
/* The encoder's CRC32 fields: 0 (the default: the calling thread computes them on the host while the
 * device encodes) or nonzero (k_crc32 computes them over the pieces in the device input buffer, four
 * bytes per piece come back with the lengths, and the calling thread computes no CRC).  The members
 * are byte for byte the same either way.  Holds like cc_bgzf_set_effort: for later cc_bgzf_deflate
 * calls and hook rounds; a running round finishes the way it began. */
int cc_bgzf_set_crc(cc_ctx *ctx, int on);
/* Deferred end-of-pass checks (no reference counterpart: the reference has no device).  With
 * deferral on, a stage call that re-runs a planned pass (cc_read_bam_rerun, cc_consensus_maker,
 * cc_duplex_consensus, cc_singleton_correction on a group that ran before) enqueues its check and
 * returns without waiting; cc_commit waits once and returns CC_E_REPLAY when any deferred pass
 * must be re-run (the caller repeats the same calls with deferral off).  Counters and results of
 * deferred passes are valid only after cc_commit returned 0. */
int cc_defer(cc_ctx *ctx, int on);
int cc_commit(cc_ctx *ctx);
/* test hook: shifts one planned total (e.g. "scan_pairs") of a group by delta, so that the group's
 * next planned pass fails its check and re-runs exactly */
int cc_debug_skew_plan(cc_ctx *ctx, int32_t group_id, const char *name, int64_t delta);
/* 1 for the debug build (libccamd_debug.so, compiled with -DCC_DEBUG_BOUNDS): its kernels check record,
 * qname, payload, slot and vote indices against their arrays, replace a bad index by 0 and record the
 * first failure; every call that waits for the device (and cc_synchronize) then returns CC_E_INVALID
 * naming the check.  0 for the release build (no checks). */
int cc_debug_build(void);
/* device operations this process's contexts have enqueued so far (kernel launches, memsets, async
 * copies; a rocPRIM sort counts once): the difference over a step is its launch count */
int64_t cc_launch_count(void);
/* planned passes of this context re-run because a guarded device index was outside its array (the
 * release build's containment: an index read from a slot no kernel of the pass wrote is replaced by 0
 * and the pass re-runs exactly instead of faulting) */
int64_t cc_guard_reruns(cc_ctx *ctx);
/* the same per group: out[0] its planned passes re-run exactly because a plan did not hold, out[1] those
 * of them after a guarded index, out[2] the events of other lanes its calls made their lane wait for */
int cc_group_reruns(cc_ctx *ctx, int32_t group_id, int64_t *out);
/* test hook: group buffer `name` grown to at least `bytes` and every byte set to `value` */
int cc_debug_poison(cc_ctx *ctx, int32_t group_id, const char *name, int64_t bytes, int32_t value);
/* test hook: the engine's prefix scan (scan_launch: k_scan_reduce + k_scan_down, or the single-launch
 * look-back k_scan_one; tiles of 4096 elements) on the caller's input, on the context's stream, with
 * the engine's own consumers.  kind selects the instantiation class:
 *   0  in = n uint32 values   ScanStore       out_a = exclusive prefix[n]
 *   1  in = n uint8 flags     ScanStore       out_a = exclusive prefix[n]
 *   2  in = n uint8 flags     EmitList        out_a = vslot[n] (the flagged element's rank, else -1),
 *                                             out_b = list[total] (the flagged indices, int32)
 *   3  in = n uint8 flags     EmitVotePairs   out_a = vslot[n], out_b = vpair[total] as 4 x int32
 *                                             {t_rec[i], p_rec[i], dec[i], i}; aux = t_rec[n], p_rec[n],
 *                                             dec[n] (3 * n int32)
 * Byte flags must be 0 or 1 (the reduce kernel sums four of them in one multiply), and the sums must
 * stay below 2^32.  engine: 0 reduce-then-scan, 1 look-back, -1 the engine's own choice (look-back up
 * to 64 tiles); the hook sets the context's switch for the call and restores it, CC_SCAN1 is not read.
 * The device input is padded to a multiple of 16 bytes with 0xff bytes, so a scan that read past n
 * would count them.  Every output array has 64 more elements than named above, in the caller's
 * arrays too: out_a holds n + 64 words, out_b n + 64 elements (kind 2: int32, kind 3: 4 x int32; unused
 * and may be NULL for kinds 0 and 1).  The device arrays are pre-filled with 0xA5A5A5A5 words and copied
 * back whole, so every element behind the last one written (out_a from n, out_b from total) must
 * still hold that word.  n == 0 launches nothing and returns total 0.  *total receives the scan's
 * total.  A look-back that waited past its bound is reported as CC_E_INVALID (no re-run).
 * These four kinds are every path of the scan: it is an exclusive sum only, and an emitter fed uint32
 * input does not compile (uint32 input only meets ScanStore).  EmitList has no call site but this
 * one: the engine's other unstaged emitters (EmitGather, EmitFamStarts, ...) share its path. */
int cc_debug_scan(cc_ctx *ctx, int32_t kind, int32_t engine, const void *in, int64_t n, const int32_t *aux,
                  void *out_a, void *out_b, int64_t *total);
/* test hook: the engine's stable LSD radix sort (sort_pairs: k_rs_hist, the scan, k_rs_scatter per 8-bit
 * digit) on the caller's n (key, value) pairs; engine chooses the digit scans' engine as above.  The
 * sort works in whole digits: it orders by key bits
 * [begin_bit, min(64, begin_bit + 8 * ceil((end_bit - begin_bit) / 8))), stably, and moves whole keys;
 * begin_bit == end_bit copies the pairs.  begin_bit <= end_bit <= 64.  out_keys and out_vals hold
 * n + 64 elements: the 64 behind the result keep the pre-filled 0xA5 bytes. */
int cc_debug_sort_pairs(cc_ctx *ctx, int32_t engine, const uint64_t *keys, const uint32_t *vals, int64_t n,
                        uint32_t begin_bit, uint32_t end_bit, uint64_t *out_keys, uint32_t *out_vals);

/* copy a record SoA into HBM; returns a table id.  With the decoder's layout (rec->meta non-NULL,
 * rec->n_deep >= 0) its columns are uploaded as they are; otherwise k_derive builds them on the device */
int cc_table_upload(cc_ctx *ctx, const cc_records *rec, int32_t max_len, int32_t *table_id);
/* The same table built on the device from raw BAM records (opt-in; the default path is
 * ccio_bam_decode + cc_table_upload).  recs: `bytes` bytes of records, block_size first, rec_off[n]
 * each record's offset (strictly increasing, inside the stream); cigar_id, bc_id, rg_id, rflags: the
 * string-derived columns of ccio_bam_decode_ids.  The stream and the four columns are uploaded, and
 * kernels build every other column and both blobs: byte for byte what ccio_bam_decode +
 * cc_table_upload give for the same records (padding and blob tails included), with the derived
 * columns built by k_derive as for any table uploaded without the decoder's layout.  *max_len: the
 * largest l_seq.  Every record is checked on the device before anything is read through its lengths
 * (csrc/unpack_core.h): an offset out of range or out of order, block_size < 32 or past the stream,
 * l_seq < 0, lengths overrunning block_size, or a CC_RF_QUAL_MISSING bit in rflags that disagrees
 * with the record is CC_E_INVALID (cc_last_error names the first such record); l_seq > 0xffff or a
 * payload of 64 GiB or more is CC_E_UNSUPPORTED.  After any error no table exists and nothing stays
 * allocated. */
int cc_table_unpack(cc_ctx *ctx, const uint8_t *recs, uint64_t bytes, const uint64_t *rec_off, int64_t n,
                    const int32_t *cigar_id, const int32_t *bc_id, const int32_t *rg_id, const uint8_t *rflags,
                    int32_t *max_len, int32_t *table_id);
/* The output stream of one stage file (the header's bytes, then n records) assembled on the device
 * from ccio_write_bam_ex's specs, byte for byte what the host writer assembles (csrc/assemble_core.h).
 *   srcs[nsrc]       the sources the specs' src_file indexes: a host stream, uploaded for the call, or
 *                    (stream NULL) a resident stream read in place, as cc_table_unpack_resident reads it;
 *   names, name_off[n_names + 1], names_bytes; rg_blob, rg_off[n_rg + 1]: the names and RG values;
 *   cons_group < 0   cons_seq[cons_seq_bytes] / cons_qual[cons_qual_bytes] are host arrays;
 *   cons_group >= 0  that group's cons_seq / cons_qual device buffers are read where they lie;
 *   flags            CCIO_W_SORT: samtools-sort order, ties in spec order.
 * out NULL is a size query (*total only).  Otherwise out[cap] receives the stream, at[n + 1] every
 * record's offset (at[0] = header_bytes, at[n] = *total).  A spec the shared layout refuses (an index
 * out of range, a template whose lengths do not fit its block_size, a consensus or RG range outside
 * its array, a new name longer than 254 bytes) is CC_E_INVALID and cc_last_error names the first such
 * spec; more than 2^31 - 1 records is CC_E_UNSUPPORTED.  After an error out holds nothing of use.
 * CC_ASM_SLICE_BYTES (environment) lowers the bytes whose offsets one scan covers (default 2^32 - 1). */
int cc_bam_assemble(cc_ctx *ctx, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs, int32_t nsrc,
                    const cc_out_spec *spec, int64_t n, const char *names, const int64_t *name_off, int64_t n_names,
                    uint64_t names_bytes, const uint8_t *cons_seq, uint64_t cons_seq_bytes, const uint8_t *cons_qual,
                    uint64_t cons_qual_bytes, int32_t cons_group, const char *rg_blob, const int64_t *rg_off,
                    int32_t n_rg, int flags, uint8_t *out, uint64_t cap, uint64_t *at, uint64_t *total);
/* the pair to hand to ccio_set_assemble_hook; unset the hook before cc_destroy */
int cc_bam_assemble_hook(cc_ctx *ctx, ccio_assemble_fn *fn, void **user);
/* cc_bam_assemble that leaves the stream on the device: the same kernels, but the stream is built in
 * a buffer registered in the resident table (cc_resident_fetch, _free, _count, _crc32 and the calls
 * above serve it; same padding) and named by *resident_id (> 0).  at[n + 1] and *total are always
 * returned (both required); the stream is downloaded only when out is non-NULL (out[cap], as for
 * cc_bam_assemble).  After any error *resident_id = 0, no resident stream remains and nothing the
 * call allocated stays allocated. */
int cc_bam_assemble_keep(cc_ctx *ctx, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs,
                         int32_t nsrc, const cc_out_spec *spec, int64_t n, const char *names, const int64_t *name_off,
                         int64_t n_names, uint64_t names_bytes, const uint8_t *cons_seq, uint64_t cons_seq_bytes,
                         const uint8_t *cons_qual, uint64_t cons_qual_bytes, int32_t cons_group, const char *rg_blob,
                         const int64_t *rg_off, int32_t n_rg, int flags, uint8_t *out, uint64_t cap, uint64_t *at,
                         uint64_t *total, int64_t *resident_id);
/* the set to hand to ccio_set_out_resident (assemble-keep, resident deflate, index fields, fetch and
 * release over this context); unset it before cc_destroy */
int cc_out_resident_hooks(cc_ctx *ctx, ccio_out_resident *cb, void **user);
/* The merge of nsrc (at most 8) coordinate-sorted record sets built on the device, byte for byte what
 * ccio_merge_handles gathers on the host (csrc/merge_core.h, bam_merge.hip.inc): the header's bytes,
 * then every source's records in key order, ties to the earlier source, then the earlier record.
 * srcs as for cc_bam_assemble.  With n the sources' records together: at[n + 1] receives the output
 * records' offsets, org[n] (may be NULL) each output record's index in the concatenation of the
 * sources, *total the stream's size; out NULL is a size query (only *total is written).
 * CC_E_INVALID, with a message naming the source and the record, for a record whose offset lies
 * outside its source, with fewer than 4 bytes left, with block_size < 32 or running past the source's
 * bytes, and for a source that is not in key order; CC_E_UNSUPPORTED for more than 8 sources or more
 * than 2^31 - 1 records.  Nothing is read through a record's length before every record was accepted. */
int cc_bam_merge(cc_ctx *ctx, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs, int32_t nsrc,
                 uint8_t *out, uint64_t cap, uint64_t *at, uint32_t *org, uint64_t *total);
/* cc_bam_merge that leaves the stream on the device as resident stream *resident_id (> 0), with the
 * resident streams' padding (cc_bgzf_deflate_resident, cc_index_fields, cc_resident_fetch and
 * cc_resident_free serve it).  at and total are required; the stream is downloaded only when out is
 * non-NULL.  After any error *resident_id = 0 and nothing stays resident. */
int cc_bam_merge_keep(cc_ctx *ctx, const uint8_t *header, uint64_t header_bytes, const cc_asm_src *srcs, int32_t nsrc,
                      uint8_t *out, uint64_t cap, uint64_t *at, uint32_t *org, uint64_t *total, int64_t *resident_id);
/* the functions to hand to ccio_set_merge_hooks; unset them before cc_destroy */
int cc_bam_merge_hooks(cc_ctx *ctx, ccio_merge_fn *merge, ccio_merge_keep_fn *keep, void **user);
/* the group whose consensus buffers the hook's next call uses when libccio passes it no arrays (that
 * call consumes it); -1 clears it */
int cc_bam_assemble_group(cc_ctx *ctx, int32_t group_id);
/* The name set (cc_names_keep, below) that cc_bam_assemble, cc_bam_assemble_keep and both hooks read in
 * place of host names from now on; 0 clears it, an unknown id is CC_E_INVALID.  A call uses the set when
 * its names argument is NULL and names_bytes > 0: the set's blob and device offsets are the names
 * table, nothing of either is uploaded and the call's name_off is not read.  n_names and names_bytes
 * must not exceed the set's (else CC_E_INVALID before any launch); without a selected set such a call
 * is CC_E_INVALID as before.  Unlike cc_bam_assemble_group's, the selection is not consumed: a stage
 * writes several files from one set, and the caller clears it (cc_names_free of the selected set
 * clears it too).  With profiling on, cc_kernel_times reports the upload of host names (names_bytes > 0)
 * as "asm_names_upload"; a call that reads a set never adds to it. */
int cc_bam_assemble_names(cc_ctx *ctx, int64_t names_id);
/* The consensus read names formatted on the device (csrc/name_core.h, name_format.hip.inc), byte for
 * byte what ccio_format_csn_names / ccio_format_dcs_names give.  Both take host arrays, write
 * off[n + 1] (name i is bytes [off[i], off[i + 1]) of the blob) and *total (= off[n]), and leave the
 * blob in a device buffer the context owns until cc_names_read fetches it or cc_names_keep keeps it;
 * a new format call or cc_destroy releases a blob nobody read.
 *   csn: f9 holds nine int32 fields per name, suffix one int64; the barcode strings (field 0) and the
 *     cigar strings (fields 5, 6) come side by side with n_bc + 1 / n_cg + 1 offsets
 *     (ccio_interner_blob).
 *   dcs: rec_tag / rec_ds are record indices into `table`, whose qname slots hold the two names.
 * A name the shared rules refuse (csn: field 0 outside the barcode table, field 5 or 6 outside the
 * cigar table; dcs: no '_' or no ':' in the tag name, no ':' in the partner name, a record index
 * outside the table) is CC_E_INVALID, and cc_last_error names the first such name and the reason; a
 * blob of 2^32 bytes or more, or more than 2^31 - 1 names, is CC_E_UNSUPPORTED.  After any error no
 * blob exists and nothing the call allocated stays allocated.  With profiling on, cc_kernel_times
 * reports the kernels as "name_sizes" and "name_write", the offsets' scan as "name_scan", the blob's
 * download as "name_download" and cc_format_csn_names' upload of f9 and suffix as "name_fields_upload". */
int cc_format_csn_names(cc_ctx *ctx, int64_t n, const int32_t *f9, const int64_t *suffix, const char *bc_blob,
                        const int64_t *bc_off, int64_t n_bc, const char *cg_blob, const int64_t *cg_off, int64_t n_cg,
                        int64_t *off, int64_t *total);
int cc_format_dcs_names(cc_ctx *ctx, int32_t table, int64_t n, const int64_t *rec_tag, const int64_t *rec_ds,
                        int64_t *off, int64_t *total);
/* The last formatted blob copied to blob[0, total) and its device buffer released.  cap < total is
 * CC_E_INVALID and keeps the buffer, as does a call without a blob to read. */
int cc_names_read(cc_ctx *ctx, char *blob, int64_t cap);
/* cc_format_csn_names with the fields read where the SSCS stage left them: n is the count of group_id's
 * emit_n, name i takes its nine fields from emit_ckey[9 * (i >> 1)] (an emitted entry's row serves its
 * two names) and its suffix from emit_n[i].  Only the two string tables are uploaded.  A group that is
 * unknown, has not run cc_consensus_maker, lacks either buffer, or whose emit_ckey does not hold exactly
 * one row per two values of emit_n (checked on the host from the buffers' used sizes, before any
 * launch) is CC_E_INVALID.  Everything else (refusals, limits, cc_last_error texts, profile scopes, the
 * pending blob) is cc_format_csn_names'. */
int cc_format_csn_names_group(cc_ctx *ctx, int32_t group_id, const char *bc_blob, const int64_t *bc_off, int64_t n_bc,
                              const char *cg_blob, const int64_t *cg_off, int64_t n_cg, int64_t *off, int64_t *total);
/* Name sets: the last formatted blob kept on the device with its 64-bit offsets, for the assembler to
 * read in place (cc_bam_assemble_names).  The blob is 16-byte aligned and allocated as
 * align16(total) + 32 bytes with the tail zero, the assembler's read contract.  A context owns its sets
 * under positive ids that are unique across contexts; an unknown, freed or foreign id is CC_E_INVALID
 * in every call, and cc_destroy frees what is left.
 *   cc_names_keep    the pending blob becomes a set (*names_id) without a download and is no longer
 *                    pending, as after cc_names_read; 0 names or 0 bytes give a valid empty set; without
 *                    a pending blob CC_E_INVALID and *names_id = 0
 *   cc_names_fetch   the set's bytes copied to blob[0, total), the set left as it is; returns total
 *                    (blob NULL: a size query); cap < total is CC_E_INVALID and copies nothing
 *   cc_names_free    frees a set
 *   cc_names_count   the live sets (leak checks) */
int cc_names_keep(cc_ctx *ctx, int64_t *names_id);
int64_t cc_names_fetch(cc_ctx *ctx, int64_t names_id, char *blob, int64_t cap);
int cc_names_free(cc_ctx *ctx, int64_t names_id);
int64_t cc_names_count(cc_ctx *ctx);
/* cc_table_unpack with the records read in place from a resident stream (cc_bgzf_inflate_keep): they
 * are its bytes [base, base + bytes), which must lie inside it (else CC_E_INVALID), and rec_off counts
 * from base, as ccio_bam_decode_ids gives it.  Checks, errors and the table are cc_table_unpack's;
 * only rec_off and the four columns are uploaded.  The call waits for the inflater's streams first
 * and does not free the resident stream.  With profiling on, cc_kernel_times reports cc_table_unpack's
 * upload of the record stream as "unpack_stream_upload"; this call never adds to it. */
int cc_table_unpack_resident(cc_ctx *ctx, int64_t id, uint64_t base, uint64_t bytes, const uint64_t *rec_off,
                             int64_t n, const int32_t *cigar_id, const int32_t *bc_id, const int32_t *rg_id,
                             const uint8_t *rflags, int32_t *max_len, int32_t *table_id);
/* The device interner: the three interned-id columns of the records recs[0 .. bytes) (rec_off[n] as
 * cc_table_unpack takes them) as local ids, and rflags with all three bits, by kernels over the raw
 * records (csrc/table_ids.hip.inc, the rules of csrc/intern_core.h: ccio_bam_decode's modes and
 * delimiter rules).  local_bc / local_cigar / local_rg[n]: each record's key as its rank among the
 * table's distinct keys in order of first occurrence in record order, -1 for a record without one;
 * first_bc / first_cigar / first_rg (capacity n): the record of each local id's first occurrence,
 * nd[k] of them (k: 0 barcode, 1 cigar, 2 RG).  The cigar's key is the raw cigar bytes, so two local
 * ids may print one string; ccio_intern_first turns the local ids into the interner's.
 * A record the shared parser refuses, or whose aux fields hold a value that does not lie whole inside
 * the record (a B header or array cut by the record's end, a negative B count, a fixed-width value
 * past the end: where the host's walk would read outside the record), is CC_E_INVALID and
 * cc_last_error names the first such record.  A delimiter of more than 16 bytes or more than
 * 2^31 - 1 records is CC_E_UNSUPPORTED (before any launch).  Keys are compared byte for byte within
 * a run of equal 64-bit hashes: a collision runs the call again under another seed, and under the
 * fourth is CC_E_COLLISION.  After any error nothing stays allocated and the outputs hold nothing of
 * use.  Profile scopes: ids_stream_upload, ids_keys, ids_sort, ids_heads, ids_scan, ids_assign,
 * ids_download. */
int cc_table_ids(cc_ctx *ctx, const uint8_t *recs, uint64_t bytes, const uint64_t *rec_off, int64_t n, int mode,
                 const char *delim, int32_t *local_bc, int32_t *local_cigar, int32_t *local_rg, uint8_t *rflags,
                 int32_t *first_bc, int32_t *first_cigar, int32_t *first_rg, int32_t nd[3]);
/* cc_table_ids with the records read in place from resident stream id's bytes [base, base + bytes), as
 * cc_table_unpack_resident reads them: it waits for the inflater's streams first, uploads only rec_off
 * and does not free the stream. */
int cc_table_ids_resident(cc_ctx *ctx, int64_t id, uint64_t base, uint64_t bytes, const uint64_t *rec_off, int64_t n,
                          int mode, const char *delim, int32_t *local_bc, int32_t *local_cigar, int32_t *local_rg,
                          uint8_t *rflags, int32_t *first_bc, int32_t *first_cigar, int32_t *first_rg, int32_t nd[3]);
/* test hook: cc_table_ids keeps only the low `bits` bits (1 .. 64; 64 is the default) of a key's hash,
 * so that small inputs collide */
int cc_debug_ids_hash_bits(cc_ctx *ctx, int32_t bits);
int cc_table_free(cc_ctx *ctx, int32_t table_id);
/* the table's derived columns (member records, position keys, qname digests, record cores and deep
 * bits, the deep-group list) built again from its record columns, on the context's stream without a
 * host wait: a repeated step's first work on a resident table (bench.py), so that the step times
 * everything from the uploaded columns on.  A no-op for a table uploaded with the decoder's layout:
 * those columns are part of its input, as the record columns are */
int cc_table_derive(cc_ctx *ctx, int32_t table_id);
/* test hook: a table's derived column ("rkey", "meta", "core", "qn_ol", "qdig", "rdeep", "dlist",
 * "ext"), base column ("tid", "pos", "mtid", "mpos", "tlen", "flag", "mapq", "cigar_id", "qlen",
 * "lseq", "bc_id", "rg_id", "rflags", "qn_off", "qn_len", "pay_off", "rdig") or blob ("qn_blob" with
 * its 16-byte tail, "payload" with its 64-byte tail) copied to dst (cap bytes); returns its byte
 * size, or a CC_E_* code */
int64_t cc_table_fetch(cc_ctx *ctx, int32_t table_id, const char *name, void *dst, int64_t cap);

/* read_bam over a record stream (region-major order; stream_rec indexes the
 * table, stream_region gives the region of each stream position,
 * region_run[r] the chromosome-run id of region r).  Multi-GPU sharding: a
 * first-streamed end whose pair completes on another shard is MOVED there.  On
 * the receiver it is a foreign entry, region -(r+1): it pairs and is counted
 * there, is never listed as a bad read, and is neither paired nor counted when
 * it is a bad read of a pass that lists them.  On the sender it keeps its own
 * entry with region r | CC_REGION_MOVED: never paired, counted and listed only
 * as such a bad read.  Each record is thus counted once over the shards.
 * CC_CNT_FOREIGN counts the entries not counted here.  Produces a group id. */
#define CC_REGION_MOVED (1 << 30)
int cc_read_bam(cc_ctx *ctx, int32_t table_id, int64_t n_stream, const int32_t *stream_rec,
                const int32_t *stream_region, int32_t n_regions, const int32_t *region_run,
                const cc_read_bam_params *params, int32_t *group_id);
int cc_group_counters(cc_ctx *ctx, int32_t group_id, int64_t *counters /* CC_NUM_COUNTERS */);
int cc_group_free(cc_ctx *ctx, int32_t group_id);

/* SSCS: consensus_maker over every family emitted by the region loop.  The
 * cutoff test count/pass >= cutoff is evaluated in IEEE double on the GPU,
 * exactly as Python evaluates it (SSCS_maker.py:154-155). */
int cc_consensus_maker(cc_ctx *ctx, int32_t group_id, double cutoff, int64_t *n_out);
/* re-run read_bam on a resident stream with a new hash seed */
int cc_read_bam_rerun(cc_ctx *ctx, int32_t group_id, uint64_t seed);
/* DCS: duplex pairing + duplex_consensus. bc_swap from ccio_interner_swap_table. */
int cc_duplex_consensus(cc_ctx *ctx, int32_t group_id, const int32_t *bc_swap, int32_t n_bc, int64_t *n_out);
/* Singleton correction against an SSCS group (scope_by_run=1). */
int cc_singleton_correction(cc_ctx *ctx, int32_t singleton_group, int32_t sscs_group, const int32_t *bc_swap,
                            int32_t n_bc, int64_t *n_out);

/* Copy a named result array of a group to host memory; returns bytes copied
 * (or the needed size when dst is NULL).  Names are documented in engine.py. */
int64_t cc_fetch(cc_ctx *ctx, int32_t group_id, const char *name, void *dst, int64_t cap);

/* ---------------------------------------------------------- function-level boundary
 * The reference's per-family functions on caller-given reads.  The reads are
 * records of an uploaded table (cc_table_upload); results are written row by row, out_stride bytes
 * of quality and out_stride/2 bytes of BAM sequence nibbles per row (first base in the high nibble,
 * out_stride even and >= the table's longest read); out_meta[5*k..] = consensus length, mapq,
 * tlen, flag, RG id (-1: none): create_aligned_segment's fields (consensus_helper.py:568-619). */

/* SSCS_maker.consensus_maker(readList, cutoff) (SSCS_maker.py:81-168) for nfam families:
 * family k is the records member_index[fam_offsets[k] .. fam_offsets[k+1]) in readList order
 * (fam_offsets[0] == 0, nfam + 1 entries); the count/pass >= cutoff test in IEEE double.  Returns the
 * CC_E_* of the reference's raise (CC_E_N_HIGHQ, CC_E_BAD_BASE, CC_E_SHORT_READ ...) for any family;
 * CC_E_INVALID for an empty family (readList[0], SSCS_maker.py:107). */
int cc_sscs_vote(cc_ctx *ctx, int32_t table_id, const int32_t *member_index, const int64_t *fam_offsets,
                 int64_t nfam, double cutoff, uint8_t *out_seq_nib, uint8_t *out_qual, int32_t *out_meta,
                 int32_t out_stride);
/* duplex_consensus(read1, read2) for n pairs: read1 = record rec_a[i] of table_a, read2 = rec_b[i] of
 * table_b.  mode 0: DCS_maker.duplex_consensus (DCS_maker.py:99-123; equal bases, min(60, q1+q2));
 * mode 1: singleton_correction.duplex_consensus (singleton_correction.py:61-86; also q1 > 29 and
 * q2 > 29), the record fields then from read1 alone (strand_correction, :89-111). */
int cc_pair_vote(cc_ctx *ctx, int32_t mode, int32_t table_a, int32_t table_b, const int32_t *rec_a,
                 const int32_t *rec_b, int64_t n, uint8_t *out_seq_nib, uint8_t *out_qual, int32_t *out_meta,
                 int32_t out_stride);

/* read_dict / tag_dict grouping (consensus_helper.py:426-500: read_dict[tag].append(read) in input
 * order; families in order of their first read, tag_dict's insertion order) on caller-given keys:
 * n keys of key_bytes bytes each (a multiple of 4, <= 256), compared exactly.  Family k is
 * out_perm[out_fam_offsets[k] .. out_fam_offsets[k+1]) (input indices, increasing); out_fam_offsets
 * holds *out_nfam + 1 entries (capacity n + 1).  The output feeds cc_sscs_vote's member_index /
 * fam_offsets directly.  Replaces SURVEY.md §8b item 3. */
int cc_group(cc_ctx *ctx, int64_t n, const void *keys, int32_t key_bytes, int32_t *out_perm,
             int64_t *out_fam_offsets, int64_t *out_nfam);
/* The duplex pairing on caller-given tags.  Entries i = 0..n-1 are processed
 * in index order (csn_pair_dict order); keys[i] is entry i's tag and partner_keys[i] its duplex_tag
 * (ccio_duplex_tag; any key map works, mutual or not), key_bytes bytes each, compared exactly; the
 * keys of one call are distinct (CC_E_INVALID otherwise).
 *   mode 0, DCS_maker.py:245-282: decision 0 = DCS with entry out_partner[i]; 1 = sscs.singleton
 *     (partner absent); 2 = skipped (the partner made a DCS before: duplex_dict).  CC_E_KEYERROR where
 *     the reference raises (read_dict[ds] deleted: a non-mutual partner processed before).
 *   mode 1, singleton_correction.py:278-319 (entries = singleton tags, x_keys[m] = SSCS tags):
 *     0 = corrected by SSCS x entry out_partner[i] (consumed); 1 = corrected by singleton entry
 *     out_partner[i] (correction_dict bookkeeping); 2 = uncorrected.
 * With out_seq non-NULL the joined pairs are also voted (duplex_consensus, DCS_maker.py:99-123 /
 * singleton_correction.py:61-86 with create_aligned_segment's fields): entry i's read is record
 * rec_a[i] of table_a, SSCS entry k's rec_x[k] of table_x; row i of out_seq / out_qual / out_meta
 * (as cc_pair_vote) holds entry i's consensus when it has one. */
int cc_duplex_join(cc_ctx *ctx, int32_t mode, int64_t n, const void *keys, const void *partner_keys, int64_t m,
                   const void *x_keys, int32_t key_bytes, int32_t *out_decision, int64_t *out_partner,
                   int32_t table_a, const int32_t *rec_a, int32_t table_x, const int32_t *rec_x,
                   uint8_t *out_seq_nib, uint8_t *out_qual, int32_t *out_meta, int32_t out_stride);

/* fastq2bam's UMI extraction decision (extract_barcodes.py:287-405) for n read
 * pairs on the GPU: h1 / h2 hold the first 32 bases of each pair's reads (zero padded, ccio_fq_heads),
 * len1 / len2 the read lengths.  pattern (N = barcode base, A/C/G/T = spacer; <= 32) or the distinct
 * barcode list blist[nblist] (<= 1024 entries of <= 32 bases; the reference's --skipcheck path).
 * Per pair: out_status 0 passing / 1 missing spacer / 2 bad barcode, out_bc (72 bytes per pair: the
 * header barcode 'R1.R2', NUL terminated), out_cut1 / out_cut2 (bases removed), list mode
 * out_bad1 / out_bad2 (ccio_fq_write's masks).  counts[3] = missing spacer, bad barcodes, passing;
 * r1_hist / r2_hist as ccio_extract_barcodes.  CC_E_UNSUPPORTED beyond those sizes (the host path
 * takes them). */
int cc_extract_barcodes(cc_ctx *ctx, int64_t n, const uint8_t *h1, const uint8_t *h2, const int32_t *len1,
                        const int32_t *len2, const char *pattern, const char *const *blist, int32_t nblist,
                        uint8_t *out_status, char *out_bc, int32_t *out_cut1, int32_t *out_cut2, uint32_t *out_bad1,
                        uint32_t *out_bad2, int64_t *counts, int64_t *r1_hist, int64_t *r2_hist);

/* ---------------------------------------------------------- multi-GPU reduction (RCCL over xGMI)
 * The sharded pipeline's one collective.  Rank 0 makes the 128-byte id
 * (cc_comm_unique_id) and hands it to every rank (e.g. torch.distributed broadcast); each rank calls
 * cc_comm_init on its own context's GPU.  RCCL is loaded at run time (dlopen librccl.so.1). */
typedef struct cc_comm cc_comm;
int cc_comm_unique_id(char *id, int32_t cap /* >= 128 */);
int cc_comm_init(cc_ctx *ctx, int32_t world, int32_t rank, const char *id, cc_comm **comm);
int cc_comm_destroy(cc_comm *comm);
/* stats.txt counters and read_families' per-size counts summed, each size's first-seen key
 * (rank << 40 | place) min-reduced, in place; comm NULL (one process): unchanged.  Replaces the
 * reference's per-process counters (SSCS_maker.py:353-408, DCS_maker.py:287-304,
 * singleton_correction.py:324-336) for one sample split over ranks. */
int cc_reduce_stats(cc_ctx *ctx, cc_comm *comm, int64_t *counters, int32_t n_counters, int64_t *fam_count,
                    int64_t *fam_first, int32_t fam_len);
/* v[n] max-reduced in place (the family table's length, per-rank times) */
int cc_allreduce_max(cc_ctx *ctx, cc_comm *comm, int64_t *v, int32_t n);


#ifdef __cplusplus
}
#endif
#endif
