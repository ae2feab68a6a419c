// The device CRC32 of the BGZF coders (k_crc32): included by cc_engine.hip before
// bgzf_deflate.hip.inc, whose encoder and whose inflater (bgzf_inflate.hip.inc) launch it on their
// own two streams; cc_crc32 and cc_resident_crc32 (at the end of bgzf_inflate.hip.inc) are its
// function-level entry points.
//
// k_crc32: one workgroup of 256 threads per segment, a segment being at most 65,536 bytes at any
// byte address.  The slice-by-4 tables and the "through 4,080 zero bytes" operator (4 x 256 entries
// each, 8 KiB together) are built in LDS by the workgroup from the polynomial; nothing is uploaded.
// Thread t takes the aligned 16-byte words t, t + 256, ... of the segment (a wave's load is 1 KiB
// contiguous) by crc_core.h's lane rule: the word's 16 bytes through the slice tables, the stride
// operator between two of its words, one advance over the bytes behind its last word.  The 256
// registers are XOR-reduced by shuffles and one LDS step; thread 0 adds the initial-value term and
// the final XOR and stores the result.  No carry-less multiply, no inline assembly.
//
// Bounds: the kernel reads only aligned 16-byte words that overlap [p, p + len); the host side
// guarantees that the allocation covers them (a resident stream's align16(total) + 32 bytes, the
// inflater's packed 16-byte slots, the encoder's input buffer of a 16-byte multiple, cc_crc32's
// padded upload).  Every LDS index is a byte value.
#include "crc_core.h"

namespace {

constexpr int CR_T = (int)crc::LANES;
static_assert(CR_T == 256 && CR_T % 64 == 0, "the stride operator is made for 256 lanes");

// where a launch's segments come from
enum { CR_SEG = 0,      // seg[j] = {offset low, offset high, length, -}
       CR_MEMBER = 1,   // seg[j] = the inflater's descriptor: {-, -, offset, length}
       CR_PIECE = 2 };  // the encoder's pieces of `total` bytes: j * 0xff00, the last one shorter

struct CrSrc {
    const uint4* w;   // word 0 of the segment
    __device__ crc::W16 word16(uint32_t i) const {
        const uint4 v = w[i];
        return crc::W16{{v.x, v.y, v.z, v.w}};
    }
};

__global__ __launch_bounds__(CR_T) void k_crc32(const uint8_t* __restrict__ base, const uint4* __restrict__ seg, int form,
                                                uint64_t total, uint32_t* __restrict__ out, int n) {
    __shared__ uint32_t s_slice[crc::SLICES * 256];
    __shared__ uint32_t s_stride[4 * 256];
    __shared__ uint32_t s_part[CR_T / 64];
    const int j = (int)blockIdx.x;
    if (j >= n) return;
    const uint32_t t = threadIdx.x;
    uint64_t off;
    uint32_t len;
    if (form == CR_PIECE) {
        off = (uint64_t)j * 0xff00u;
        len = off < total ? (uint32_t)(total - off < 0xff00u ? total - off : 0xff00u) : 0;
    } else {
        const uint4 d = seg[j];
        off = form == CR_SEG ? ((uint64_t)d.y << 32) | d.x : d.z;
        len = form == CR_SEG ? d.z : d.w;
    }
    {
        const uint32_t xs = crc::xpow8n(crc::STRIDE_BYTES);   // (a constant the compiler may fold)
        for (int k = 0; k < crc::SLICES; ++k) {
            s_slice[256 * k + t] = crc::slice_entry(k, t);
            s_stride[256 * k + t] = crc::stride_entry(k, t, xs);
        }
    }
    __syncthreads();
    const uint8_t* p = base + off;
    const uint32_t pad = (uint32_t)((uintptr_t)p & 15);
    const crc::Tables T = {s_slice, s_stride};
    uint32_t r = crc::lane(T, CrSrc{(const uint4*)(p - pad)}, pad, len, t);
    for (int d = 32; d >= 1; d >>= 1) r ^= __shfl_xor(r, d);
    if ((t & 63) == 0) s_part[t >> 6] = r;
    __syncthreads();
    if (t == 0) {
        uint32_t raw0 = 0;
        for (int k = 0; k < CR_T / 64; ++k) raw0 ^= s_part[k];
        out[j] = crc::finish(raw0, len);
    }
}

// one launch of k_crc32 on st, between ev[0] and ev[1] when ev is given
inline hipError_t crc_launch(hipStream_t st, hipEvent_t* ev, const uint8_t* base, const uint4* seg, int form, uint64_t total,
                             uint32_t* out, int n) {
    hipError_t e = hipSuccess;
    if (ev) e = hipEventRecord(ev[0], st);
    if (e != hipSuccess) return e;
    klaunch(st, k_crc32, (unsigned)n, CR_T, base, seg, form, total, out, n);
    e = hipGetLastError();
    if (e == hipSuccess && ev) e = hipEventRecord(ev[1], st);
    return e;
}

// What a coder needs for its CRCs, one set per stream: the values on the device and in pinned
// memory, and the events around the kernel.  Made by the first round that asks for CRCs.
struct CrcBufs {
    bool ready = false;
    uint32_t* d[2] = {nullptr, nullptr};
    uint32_t* h[2] = {nullptr, nullptr};
    hipEvent_t ev[2][2] = {};
    bool timed[2] = {false, false};
};

inline hipError_t crc_bufs_init(CrcBufs* B, size_t count) {
    if (B->ready) return hipSuccess;
    for (int b = 0; b < 2; ++b) {
        hipError_t e = B->d[b] ? hipSuccess : hipMalloc((void**)&B->d[b], count * sizeof(uint32_t));
        if (e == hipSuccess && !B->h[b]) e = hipHostMalloc((void**)&B->h[b], count * sizeof(uint32_t));
        for (int k = 0; k < 2 && e == hipSuccess; ++k)
            if (!B->ev[b][k]) e = hipEventCreate(&B->ev[b][k]);
        if (e != hipSuccess) return e;
    }
    B->ready = true;
    return hipSuccess;
}

inline void crc_bufs_free(CrcBufs* B) {
    for (int b = 0; b < 2; ++b) {
        if (B->d[b]) (void)hipFree(B->d[b]);
        if (B->h[b]) (void)hipHostFree(B->h[b]);
        for (int k = 0; k < 2; ++k)
            if (B->ev[b][k]) (void)hipEventDestroy(B->ev[b][k]);
    }
    *B = CrcBufs();
}

}  // namespace
