"""ctypes bindings for libccio.so (host BAM I/O) and libccamd.so (HIP engine).

The libraries are built in-tree by ``__graft_entry__.build()`` into
``consensuscruncher_amd/lib/``.  Loading fails loudly: there is no CPU fallback
for the GPU engine (tests and bench rely on that).
"""
import ctypes as C
import os

import numpy as np

LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")

CC_E = {
    -1: "CC_E_INVALID", -2: "CC_E_HIP", -3: "CC_E_N_HIGHQ", -4: "CC_E_BAD_BASE", -5: "CC_E_SHORT_READ",
    -6: "CC_E_NO_QUAL", -7: "CC_E_NO_CIGAR", -8: "CC_E_DUP_QNAME",
    -9: "CC_E_AMBIGUOUS",   # retired: never returned, the number stays reserved
    -10: "CC_E_COLLISION", -11: "CC_E_UNSUPPORTED", -12: "CC_E_KEYERROR",
    -13: "CC_E_REPLAY",
}
CC_E_INVALID = -1
CC_E_N_HIGHQ = -3
CC_E_COLLISION = -10
CC_E_UNSUPPORTED = -11
CC_E_KEYERROR = -12
CC_E_REPLAY = -13

CNT = dict(COUNTER=0, UNMAPPED=1, UNMAPPED_MATE=2, MULTIPLE_MAPPING=3, BAD_SPACER=4, PAIRS=5, READ_ENDS=6,
           FAMILIES=7, ENTRIES=8, UNPAIRED=9, ORPHAN_TAGS=10, DROPPED=11, BAD_LISTED=12, FOREIGN=13)
NUM_COUNTERS = 16
REGION_MOVED = 1 << 30   # CC_REGION_MOVED: a stream entry moved to another shard (cc_read_bam)

OUT_RAW, OUT_RENAME, OUT_NEW = 0, 1, 2
W_SORT, W_INDEX, W_ASYNC, W_MEMORY = 1, 2, 4, 8   # ccio writer flags (CCIO_W_SORT, _INDEX, _ASYNC, _MEMORY)

RF_BAD_SPACER, RF_QUAL_MISSING, RF_RG_UNSUPPORTED = 1, 2, 4


class CCError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "%s (%d): %s" % (CC_E.get(code, "CC_E?"), code, msg))
        self.code = code


P = C.c_void_p
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)


class cc_records(C.Structure):
    _fields_ = [("n", C.c_int64),
                ("tid", P), ("pos", P), ("mtid", P), ("mpos", P), ("tlen", P),
                ("flag", P), ("mapq", P),
                ("cigar_id", P), ("qlen", P), ("lseq", P), ("bc_id", P), ("rg_id", P),
                ("rflags", P),
                ("qn_off", P), ("qn_len", P), ("qn_blob", P), ("qn_blob_bytes", C.c_uint64),
                ("pay_off", P), ("payload", P), ("payload_bytes", C.c_uint64), ("rdig", P),
                # the decoder's kernel layout (optional; include/consensuscruncher_amd.h)
                ("rkey", P), ("meta", P), ("core", P), ("qn_ol", P), ("qdig", P), ("rdeep", P), ("dlist", P),
                ("n_deep", C.c_int64), ("ext", P), ("n_ext", C.c_int32)]


class cc_out_spec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("src_file", C.c_int32), ("src_rec", C.c_int64), ("name_id", C.c_int64),
                ("flag", C.c_int32), ("mapq", C.c_int32), ("tlen", C.c_int32), ("rg_id", C.c_int32),
                ("cons_off", C.c_int64), ("cons_len", C.c_int32), ("pad", C.c_int32)]


OUT_SPEC_DTYPE = np.dtype([("kind", "<i4"), ("src_file", "<i4"), ("src_rec", "<i8"), ("name_id", "<i8"),
                           ("flag", "<i4"), ("mapq", "<i4"), ("tlen", "<i4"), ("rg_id", "<i4"),
                           ("cons_off", "<i8"), ("cons_len", "<i4"), ("pad", "<i4")], align=True)
assert OUT_SPEC_DTYPE.itemsize == C.sizeof(cc_out_spec)


class cc_read_bam_params(C.Structure):
    _fields_ = [("delim_filter", C.c_int32), ("badread_file", C.c_int32), ("scope_by_run", C.c_int32),
                ("coord_sorted", C.c_int32), ("seed", C.c_uint64)]


# ccio_deflate_fn (include/consensuscruncher_amd.h): user, data, n, stage, slot, out_len, pieces
DEFLATE_FN = C.CFUNCTYPE(C.c_int, P, P, C.c_uint64, P, C.c_uint64, C.POINTER(C.c_uint32), C.c_int64)
# ccio_inflate_fn: user, comp, coff, clen, uoff, ulen, members, out, ok
INFLATE_FN = C.CFUNCTYPE(C.c_int, P, P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                         C.POINTER(C.c_uint32), C.c_int64, P, C.POINTER(C.c_uint8))
# ccio_inflate_keep_fn: the same, then total, token; ccio_resident_patch_fn: user, token, off, bytes, n
INFLATE_KEEP_FN = C.CFUNCTYPE(C.c_int, P, P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                              C.POINTER(C.c_uint32), C.c_int64, P, C.POINTER(C.c_uint8), C.c_uint64,
                              C.POINTER(C.c_int64))
RESIDENT_PATCH_FN = C.CFUNCTYPE(C.c_int, P, C.c_int64, C.c_uint64, P, C.c_uint64)
# ccio_inflate_crc_fn and ccio_inflate_keep_crc_fn: their plain siblings, then crc
INFLATE_CRC_FN = C.CFUNCTYPE(C.c_int, P, P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                             C.POINTER(C.c_uint32), C.c_int64, P, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32))
INFLATE_KEEP_CRC_FN = C.CFUNCTYPE(C.c_int, P, P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint32), C.c_int64, P, C.POINTER(C.c_uint8), C.c_uint64,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_uint32))


class cc_asm_src(C.Structure):
    _fields_ = [("stream", P), ("bytes", C.c_uint64), ("resident_id", C.c_int64), ("base", C.c_uint64),
                ("rec_off", P), ("nrec", C.c_int64)]


# cc_asm_alloc_fn: actx, total -> the stream's buffer
ASM_ALLOC_FN = C.CFUNCTYPE(P, P, C.c_uint64)
# ccio_assemble_fn: user, header, header_bytes, srcs, nsrc, spec, n, names, name_off, n_names, names_bytes,
# cons_seq, cons_seq_bytes, cons_qual, cons_qual_bytes, rg_blob, rg_off, n_rg, flags, alloc, actx, at, total
ASSEMBLE_FN = C.CFUNCTYPE(C.c_int, P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, P, C.c_int64, P, P, C.c_int64,
                          C.c_uint64, P, C.c_uint64, P, C.c_uint64, P, P, C.c_int32, C.c_int, ASM_ALLOC_FN, P,
                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
# ccio_merge_fn: user, header, header_bytes, srcs, nsrc, alloc, actx, at, org, total; ccio_merge_keep_fn: the
# same with need_host before at and token at the end
MERGE_FN = C.CFUNCTYPE(C.c_int, P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, ASM_ALLOC_FN, P,
                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64))
MERGE_KEEP_FN = C.CFUNCTYPE(C.c_int, P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, ASM_ALLOC_FN, P, C.c_int,
                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64))


class cc_index_field(C.Structure):
    _fields_ = [("tid", C.c_int32), ("pos", C.c_int32), ("block_size", C.c_uint32), ("rl", C.c_uint32)]


INDEX_FIELD_DTYPE = np.dtype([("tid", "<i4"), ("pos", "<i4"), ("block_size", "<u4"), ("rl", "<u4")])
assert INDEX_FIELD_DTYPE.itemsize == C.sizeof(cc_index_field) == 16

# the resident output set (ccio_set_out_resident).  ccio_assemble_keep_fn: ccio_assemble_fn's arguments up to
# actx, then need_host, at, total, token
ASSEMBLE_KEEP_FN = C.CFUNCTYPE(C.c_int, P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, P, C.c_int64, P, P,
                               C.c_int64, C.c_uint64, P, C.c_uint64, P, C.c_uint64, P, P, C.c_int32, C.c_int,
                               ASM_ALLOC_FN, P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_int64))
# ccio_deflate_resident_fn: user, token, off, n, stage, slot, out_len, pieces
DEFLATE_RESIDENT_FN = C.CFUNCTYPE(C.c_int, P, C.c_int64, C.c_uint64, C.c_uint64, P, C.c_uint64, C.POINTER(C.c_uint32),
                                  C.c_int64)
# ccio_index_fields_fn: user, token, at, n, fields
INDEX_FIELDS_FN = C.CFUNCTYPE(C.c_int, P, C.c_int64, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(cc_index_field))
# ccio_resident_fetch_fn: user, token, off, n, dst; ccio_resident_release_fn: user, token
RESIDENT_FETCH_FN = C.CFUNCTYPE(C.c_int, P, C.c_int64, C.c_uint64, C.c_uint64, P)
RESIDENT_RELEASE_FN = C.CFUNCTYPE(None, P, C.c_int64)


class ccio_out_resident(C.Structure):
    _fields_ = [("assemble_keep", P), ("deflate", P), ("index_fields", P), ("fetch", P), ("release", P)]


_io = None
_amd = None

IO_SIGS = {
    "ccio_last_error": (C.c_char_p, []),
    "ccio_flush": (C.c_int, []),
    "ccio_set_deflate_hook": (None, [P, P]),
    "ccio_set_assemble_hook": (None, [P, P]),
    "ccio_set_merge_hooks": (None, [P, P, P]),
    "ccio_set_inflate_hook": (None, [P, P]),
    "ccio_set_inflate_keep_hook": (None, [P, P, P]),
    "ccio_set_inflate_crc_hook": (None, [P, P]),
    "ccio_set_inflate_keep_crc_hook": (None, [P, P, P]),
    "ccio_bam_resident": (C.c_int, [P, i64p, C.POINTER(C.c_uint64)]),
    "ccio_set_out_resident": (None, [C.POINTER(ccio_out_resident), P]),
    "ccio_bam_set_resident": (C.c_int, [P, C.c_int64, C.c_uint64]),
    "ccio_bam_stream": (C.c_int, [P, C.POINTER(P), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ccio_value_census": (C.c_int, [P, C.c_int64, C.c_int32, P, P]),
    "ccio_interner_new": (P, []),
    "ccio_interner_free": (None, [P]),
    "ccio_interner_size": (C.c_int64, [P, C.c_int]),
    "ccio_interner_get": (C.c_int, [P, C.c_int, C.c_int64, C.c_char_p, C.c_int]),
    "ccio_interner_intern": (C.c_int32, [P, C.c_int, C.c_char_p]),
    "ccio_interner_swap_table": (C.c_int64, [P, P, C.c_int64]),
    "ccio_bam_open": (P, [C.c_char_p, C.c_int]),
    "ccio_bam_close": (None, [P]),
    "ccio_bam_nrec": (C.c_int64, [P]),
    "ccio_bam_nref": (C.c_int32, [P]),
    "ccio_bam_ref": (C.c_int, [P, C.c_int32, C.c_char_p, C.c_int, i32p]),
    "ccio_bam_qname": (C.c_int, [P, C.c_int64, C.c_char_p, C.c_int]),
    "ccio_bam_layout": (C.c_int, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i32p, C.c_int]),
    "ccio_bam_decode": (C.c_int, [P, P, C.c_int, C.c_char_p, C.POINTER(cc_records), C.c_int]),
    "ccio_bam_decode_ids": (C.c_int, [P, P, C.c_int, C.c_char_p, C.POINTER(cc_records), C.c_int, C.POINTER(P),
                                      C.POINTER(C.c_uint64), P, i32p]),
    "ccio_bam_decode_cols": (C.c_int, [P, C.POINTER(cc_records), C.c_int, C.POINTER(P), C.POINTER(C.c_uint64), P, i32p]),
    "ccio_intern_first": (C.c_int, [P, P, C.c_int, C.c_char_p, P, P, P, C.c_int64, P, P, P, C.c_int]),
    "ccio_intern_keys": (C.c_int, [P, C.c_int, C.c_char_p, P, P, P, P, P]),
    "ccio_format_csn_names": (C.c_int64, [P, C.c_int64, P, P, P, C.c_int64, P]),
    "ccio_dcs_name": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "ccio_duplex_tag": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int]),
    "ccio_format_dcs_names": (C.c_int64, [P, C.c_int64, P, P, P, C.c_int64, P]),
    "ccio_dcs_names_plain": (C.c_int, [P, C.c_int64, P, P]),
    "ccio_interner_blob": (C.c_int64, [P, C.c_int, P, C.c_int64, P]),
    "ccio_write_bam": (C.c_int, [C.c_char_p, P, P, C.c_int64, P, P, C.c_int, P, P, P, P, C.c_int, C.c_int]),
    "ccio_sort_bam": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
    "ccio_merge_bams": (C.c_int, [C.c_char_p, P, C.c_int, C.c_int, C.c_int]),
    "ccio_write_bam_ex": (C.c_int, [C.c_char_p, P, P, C.c_int64, P, P, C.c_int, P, P, P, P, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(P)]),
    "ccio_sort_bam_ex": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]),
    "ccio_merge_handles": (C.c_int, [C.c_char_p, P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)]),
    "ccio_concat_bams": (C.c_int, [C.c_char_p, P, C.c_int, C.c_int, C.c_int]),
    "ccio_index_bam": (C.c_int, [C.c_char_p]),
    "ccio_extract_barcodes": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, P, C.c_int32, C.c_int, P, P,
                                        P, P]),
    "ccio_fq_open": (P, [C.c_char_p, C.c_char_p, C.c_int32, C.c_int]),
    "ccio_fq_close": (None, [P]),
    "ccio_fq_info": (C.c_int, [P, i64p, i32p]),
    "ccio_fq_heads": (C.c_int, [P, C.c_int32, P, P, P, P]),
    "ccio_fq_write": (C.c_int, [P, C.c_char_p, C.c_int, P, P, C.c_int32, P, P, P, P, P, C.c_int32, C.c_int]),
    "ccio_bam_open_regions": (P, [C.c_char_p, C.c_int32, P, P, P, C.c_int]),
    "ccio_bam_cores": (C.c_int, [P, P, P, P, P, P]),
    "ccio_bam_pack": (C.c_int64, [P, C.c_int64, P, P, C.c_int64]),
    "ccio_bam_combine": (P, [P, P, C.c_int32, P, P, C.c_int32, C.c_int, C.c_int]),
    "ccio_bam_origin": (C.c_int, [P, P]),
    "ccio_bam_write_all": (C.c_int, [C.c_char_p, P, C.c_int, C.c_int]),
    "ccio_bam_write_ex": (C.c_int, [C.c_char_p, P, C.c_int, C.c_int, C.c_int]),
    "ccio_bam_route": (P, [P, P, C.c_int32, P, P, C.c_int32, C.c_int, C.c_int]),
    "ccio_bam_is_sorted": (C.c_int, [P, C.c_int]),
    "ccio_region_stream": (C.c_int64, [C.c_int64, P, P, C.c_int32, C.c_int32, P, P, P, P, P]),
    "ccio_stream_sent": (C.c_int, [C.c_int64, P, P, P, P, P, P, C.c_int32, P, P, P, C.c_int32, P, P, C.c_int32, P, P]),
    "ccio_bai_mapped": (C.c_int64, [C.c_char_p]),
    "ccio_bai_region_bytes": (C.c_int, [C.c_char_p, C.c_int32, P, P, P, P]),
    "ccio_write_columns": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, P, P, C.c_int64, P, P, P, P, P, P, P, P,
                                     P, P, P, P, C.c_int32, P, P, P, P, C.c_int, C.c_int]),
}

AMD_SIGS = {
    "cc_create": (C.c_int, [C.c_int, C.POINTER(P)]),
    "cc_destroy": (C.c_int, [P]),
    "cc_last_error": (C.c_char_p, [P]),
    "cc_host_alloc": (P, [P, C.c_uint64]),
    "cc_host_free": (None, [P, P]),
    "cc_set_profiling": (C.c_int, [P, C.c_int]),
    "cc_profile_only": (C.c_int, [P, C.c_char_p]),
    "cc_kernel_times": (C.c_int, [P, C.c_char_p, C.c_int, P, P, C.c_int]),
    "cc_synchronize": (C.c_int, [P]),
    "cc_bgzf_deflate": (C.c_int64, [P, P, C.c_uint64, P, C.c_uint64, P, C.c_int64]),
    "cc_bgzf_hook": (C.c_int, [P, C.POINTER(P), C.POINTER(P)]),
    "cc_bgzf_set_effort": (C.c_int, [P, C.c_int]),
    "cc_bgzf_inflate": (C.c_int64, [P, P, P, P, P, P, C.c_int64, P, P]),
    "cc_bgzf_inflate_hook": (C.c_int, [P, C.POINTER(P), C.POINTER(P)]),
    "cc_bgzf_inflate_keep": (C.c_int64, [P, P, P, P, P, P, C.c_int64, P, P, C.c_uint64, i64p]),
    "cc_bgzf_inflate_keep_hook": (C.c_int, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
    "cc_resident_patch": (C.c_int, [P, C.c_int64, C.c_uint64, P, C.c_uint64]),
    "cc_resident_free": (C.c_int, [P, C.c_int64]),
    "cc_resident_fetch": (C.c_int64, [P, C.c_int64, P, C.c_uint64]),
    "cc_resident_count": (C.c_int64, [P]),
    "cc_crc32": (C.c_int, [P, P, C.c_uint64, P, P, C.c_int64, P]),
    "cc_resident_crc32": (C.c_int, [P, C.c_int64, P, P, C.c_int64, P]),
    "cc_bgzf_inflate_crc": (C.c_int64, [P, P, P, P, P, P, C.c_int64, P, P, P]),
    "cc_bgzf_inflate_keep_crc": (C.c_int64, [P, P, P, P, P, P, C.c_int64, P, P, C.c_uint64, i64p, P]),
    "cc_bgzf_inflate_crc_hook": (C.c_int, [P, C.POINTER(P), C.POINTER(P)]),
    "cc_bgzf_inflate_keep_crc_hook": (C.c_int, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
    "cc_bgzf_set_crc": (C.c_int, [P, C.c_int]),
    "cc_defer": (C.c_int, [P, C.c_int]),
    "cc_commit": (C.c_int, [P]),
    "cc_debug_skew_plan": (C.c_int, [P, C.c_int32, C.c_char_p, C.c_int64]),
    "cc_debug_build": (C.c_int, []),
    "cc_launch_count": (C.c_int64, []),
    "cc_table_upload": (C.c_int, [P, C.POINTER(cc_records), C.c_int32, i32p]),
    "cc_table_unpack": (C.c_int, [P, P, C.c_uint64, P, C.c_int64, P, P, P, P, i32p, i32p]),
    "cc_table_unpack_resident": (C.c_int, [P, C.c_int64, C.c_uint64, C.c_uint64, P, C.c_int64, P, P, P, P, i32p,
                                           i32p]),
    "cc_table_ids": (C.c_int, [P, P, C.c_uint64, P, C.c_int64, C.c_int, C.c_char_p, P, P, P, P, P, P, P, P]),
    "cc_table_ids_resident": (C.c_int, [P, C.c_int64, C.c_uint64, C.c_uint64, P, C.c_int64, C.c_int, C.c_char_p, P, P, P,
                                        P, P, P, P, P]),
    "cc_debug_ids_hash_bits": (C.c_int, [P, C.c_int32]),
    "cc_bam_assemble": (C.c_int, [P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, P, C.c_int64, P, P, C.c_int64,
                                  C.c_uint64, P, C.c_uint64, P, C.c_uint64, C.c_int32, P, P, C.c_int32, C.c_int, P,
                                  C.c_uint64, P, C.POINTER(C.c_uint64)]),
    "cc_bam_assemble_hook": (C.c_int, [P, C.POINTER(P), C.POINTER(P)]),
    "cc_bam_assemble_keep": (C.c_int, [P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, P, C.c_int64, P, P,
                                       C.c_int64, C.c_uint64, P, C.c_uint64, P, C.c_uint64, C.c_int32, P, P, C.c_int32,
                                       C.c_int, P, C.c_uint64, P, C.POINTER(C.c_uint64), i64p]),
    "cc_out_resident_hooks": (C.c_int, [P, C.POINTER(ccio_out_resident), C.POINTER(P)]),
    "cc_bam_merge": (C.c_int, [P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, P, C.c_uint64, P, P,
                               C.POINTER(C.c_uint64)]),
    "cc_bam_merge_keep": (C.c_int, [P, P, C.c_uint64, C.POINTER(cc_asm_src), C.c_int32, P, C.c_uint64, P, P,
                                    C.POINTER(C.c_uint64), i64p]),
    "cc_bam_merge_hooks": (C.c_int, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
    "cc_bgzf_deflate_resident": (C.c_int64, [P, C.c_int64, C.c_uint64, C.c_uint64, P, C.c_uint64, P, C.c_int64]),
    "cc_index_fields": (C.c_int, [P, C.c_int64, P, C.c_int64, P]),
    "cc_resident_put": (C.c_int, [P, P, C.c_uint64, i64p]),
    "cc_bam_assemble_group": (C.c_int, [P, C.c_int32]),
    "cc_format_csn_names": (C.c_int, [P, C.c_int64, P, P, P, P, C.c_int64, P, P, C.c_int64, P, i64p]),
    "cc_format_dcs_names": (C.c_int, [P, C.c_int32, C.c_int64, P, P, P, i64p]),
    "cc_names_read": (C.c_int, [P, P, C.c_int64]),
    "cc_format_csn_names_group": (C.c_int, [P, C.c_int32, P, P, C.c_int64, P, P, C.c_int64, P, i64p]),
    "cc_names_keep": (C.c_int, [P, i64p]),
    "cc_names_fetch": (C.c_int64, [P, C.c_int64, P, C.c_int64]),
    "cc_names_free": (C.c_int, [P, C.c_int64]),
    "cc_names_count": (C.c_int64, [P]),
    "cc_bam_assemble_names": (C.c_int, [P, C.c_int64]),
    "cc_table_free": (C.c_int, [P, C.c_int32]),
    "cc_table_derive": (C.c_int, [P, C.c_int32]),
    "cc_table_fetch": (C.c_int64, [P, C.c_int32, C.c_char_p, P, C.c_int64]),
    "cc_guard_reruns": (C.c_int64, [P]),
    "cc_group_reruns": (C.c_int, [P, C.c_int32, i64p]),
    "cc_debug_poison": (C.c_int, [P, C.c_int32, C.c_char_p, C.c_int64, C.c_int32]),
    "cc_debug_scan": (C.c_int, [P, C.c_int32, C.c_int32, P, C.c_int64, P, P, P, i64p]),
    "cc_debug_sort_pairs": (C.c_int, [P, C.c_int32, P, P, C.c_int64, C.c_uint32, C.c_uint32, P, P]),
    "cc_read_bam": (C.c_int, [P, C.c_int32, C.c_int64, P, P, C.c_int32, P, C.POINTER(cc_read_bam_params), i32p]),
    "cc_read_bam_rerun": (C.c_int, [P, C.c_int32, C.c_uint64]),
    "cc_group_counters": (C.c_int, [P, C.c_int32, P]),
    "cc_group_free": (C.c_int, [P, C.c_int32]),
    "cc_consensus_maker": (C.c_int, [P, C.c_int32, C.c_double, i64p]),
    "cc_duplex_consensus": (C.c_int, [P, C.c_int32, P, C.c_int32, i64p]),
    "cc_singleton_correction": (C.c_int, [P, C.c_int32, C.c_int32, P, C.c_int32, i64p]),
    "cc_fetch": (C.c_int64, [P, C.c_int32, C.c_char_p, P, C.c_int64]),
    "cc_sscs_vote": (C.c_int, [P, C.c_int32, P, P, C.c_int64, C.c_double, P, P, P, C.c_int32]),
    "cc_pair_vote": (C.c_int, [P, C.c_int32, C.c_int32, C.c_int32, P, P, C.c_int64, P, P, P, C.c_int32]),
    "cc_group": (C.c_int, [P, C.c_int64, P, C.c_int32, P, P, i64p]),
    "cc_duplex_join": (C.c_int, [P, C.c_int32, C.c_int64, P, P, C.c_int64, P, C.c_int32, P, P, C.c_int32, P,
                                 C.c_int32, P, P, P, P, C.c_int32]),
    "cc_extract_barcodes": (C.c_int, [P, C.c_int64, P, P, P, P, C.c_char_p, P, C.c_int32, P, P, P, P, P, P, P, P, P]),
    "cc_comm_unique_id": (C.c_int, [C.c_char_p, C.c_int32]),
    "cc_comm_init": (C.c_int, [P, C.c_int32, C.c_int32, C.c_char_p, C.POINTER(P)]),
    "cc_comm_destroy": (C.c_int, [P]),
    "cc_reduce_stats": (C.c_int, [P, P, P, C.c_int32, P, P, C.c_int32]),
    "cc_allreduce_max": (C.c_int, [P, P, P, C.c_int32]),
}


def _bind(lib, sigs):
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def io():
    global _io
    if _io is None:
        path = os.path.join(LIBDIR, "libccio.so")
        if not os.path.exists(path):
            raise ImportError("libccio.so not built; run __graft_entry__.build()")
        _io = _bind(C.CDLL(path), IO_SIGS)
    return _io


def amd_path():
    """The engine library this process loads: CCAMD_LIB (an alternative in-tree build of the same
    engine, tuning variants) or the in-tree lib/libccamd.so."""
    return os.environ.get("CCAMD_LIB") or os.path.join(LIBDIR, "libccamd.so")


def lib_sha(path=None):
    """Build identity of an engine library: the first 16 hex digits of its file's SHA-256 (bench.py
    stamps its line and the PMC / kernel-trace summaries with it, and quotes PMC traffic only from
    summaries of the same build)."""
    import hashlib
    h = hashlib.sha256()
    with open(path or amd_path(), "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def amd():
    """The HIP engine.  Raises if the extension is missing: no CPU fallback."""
    global _amd
    if _amd is None:
        path = amd_path()
        if not os.path.exists(path):
            raise ImportError("libccamd.so (HIP engine) not built; run __graft_entry__.build()")
        _amd = _bind(C.CDLL(path), AMD_SIGS)
    return _amd


def ptr(a):
    return None if a is None else a.ctypes.data_as(P)


def io_error():
    return io().ccio_last_error().decode(errors="replace")
