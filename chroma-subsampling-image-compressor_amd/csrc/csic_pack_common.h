// csic_pack_common.h -- what the device codecs of the group coding (csic_pack.hip) and of the Rice coding (csic_rice.hip) share: the kernels'
// argument, the checked accessors of the PLANAR_BITS and the coded frames, the block scan, the load of a group with its folded residuals,
// and the launch of the scan over a frame's block totals (k_pack_scan itself lives in csic_pack.hip).
#pragma once
#include "csic_kernel_ops.h"

namespace csic {

typedef const uint8_t CSIC_GLOBAL *gpsrc_t;
typedef uint8_t CSIC_GLOBAL *gpdst_t;

constexpr int PK_T = 256, PK_WAVES = PK_T / 64;

// the kernels' argument
struct PkArgs {
    uint8_t *bits;                 // PLANAR_BITS frames, frame_bytes apart (pack reads, unpack writes)
    uint8_t *coded;                // coded frames, bound_bytes apart (pack writes, unpack reads)
    uint32_t *ws;                  // [frame][block]: the blocks' sums of w, after the scan their payload offsets in dwords
    unsigned long long *sizes;     // [frame] coded_bytes (pack; NULL for unpack)
    int64_t frame_bytes, bound_bytes;
    int64_t off[3], bytes[3];      // the planes' payload ranges inside a PLANAR_BITS frame
    int64_t payload_offset;        // = fixed_bytes
    uint32_t n[3], groups[3];      // samples, groups per plane
    int32_t q[3];                  // bits per code
    uint32_t woff[3], aoff[3];     // byte offsets of the widths / anchors sections
    uint32_t adw[3];               // dwords of an anchors section
    uint32_t block0[3], nblocks;   // a plane's first block number; blocks per frame
    int32_t plane0;                // plane of blockIdx.y = 0
};

#if defined(CSIC_DEBUG) && CSIC_DEBUG
#define CSIC_PCHECK(lim, off, cnt) CSIC_CHECK((int64_t)(off) >= 0 && (int64_t)(off) + (cnt) <= (int64_t)(lim))
#else
#define CSIC_PCHECK(lim, off, cnt) do { } while (0)
#endif

// the PLANAR_BITS frame: a dword (4-byte aligned) or a byte at a byte offset
template <bool NT> __device__ __forceinline__ uint32_t pk_bits_ld4(const PkArgs &e, gpdst_t fb, int64_t off)
{
    CSIC_PCHECK(e.frame_bytes, off, 4); (void)e;
    return ld1<NT>((gin_t)(fb + off));
}
__device__ __forceinline__ uint32_t pk_bits_ld1(const PkArgs &e, gpdst_t fb, int64_t off)
{
    CSIC_PCHECK(e.frame_bytes, off, 1); (void)e;
    return fb[off];
}
template <bool NT> __device__ __forceinline__ void pk_bits_st4(const PkArgs &e, gpdst_t fb, int64_t off, uint32_t v)
{
    CSIC_PCHECK(e.frame_bytes, off, 4); (void)e;
    st1<NT>((gout_t)(fb + off), v);
}
__device__ __forceinline__ void pk_bits_st1(const PkArgs &e, gpdst_t fb, int64_t off, uint32_t v)
{
    CSIC_PCHECK(e.frame_bytes, off, 1); (void)e;
    fb[off] = (uint8_t)v;
}
// the coded frame: dwords
__device__ __forceinline__ uint32_t pk_coded_ld4(const PkArgs &e, gpdst_t cb, int64_t off)
{
    CSIC_PCHECK(e.bound_bytes, off, 4); (void)e;
    return *(gin_t)(cb + off);
}
__device__ __forceinline__ void pk_coded_st4(const PkArgs &e, gpdst_t cb, int64_t off, uint32_t v)
{
    CSIC_PCHECK(e.bound_bytes, off, 4); (void)e;
    *(gout_t)(cb + off) = v;
}
// the workspace entry of block `b` of this block's frame (`frame` < 65535: the grid's z or, for the scan, x)
__device__ __forceinline__ gout_t pk_ws(const PkArgs &e, uint32_t frame, uint32_t b)
{
    CSIC_CHECK(b < e.nblocks && frame < 65535u);
    return (gout_t)(uintptr_t)e.ws + ((uint64_t)frame * e.nblocks + b);
}

__device__ __forceinline__ gpdst_t pk_bits_frame(const PkArgs &e) { return (gpdst_t)(uintptr_t)e.bits + (int64_t)blockIdx.z * e.frame_bytes; }
__device__ __forceinline__ gpdst_t pk_coded_frame(const PkArgs &e) { return (gpdst_t)(uintptr_t)e.coded + (int64_t)blockIdx.z * e.bound_bytes; }

// Exclusive scan of one value per thread over the block, and the block's total.  Every thread of the block calls it.
__device__ __forceinline__ uint32_t pk_block_scan(uint32_t v, uint32_t *s_tot, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= (uint32_t)d) inc += t;
    }
    if (lane == 63u) s_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < PK_WAVES; ++k) {
        const uint32_t t = s_tot[k];
        if ((uint32_t)k < wave) before += t;
        total += t;
    }
    __syncthreads();                                   // s_tot may be written again at once
    return before + inc - v;
}

// Group g of a plane -> its 32 folded residuals, its width (returned) and its anchor.
template <int Q, bool NT>
__device__ __forceinline__ uint32_t pk_fold_group(const PkArgs &e, gpdst_t fb, int plane, uint32_t g, uint32_t (&u)[32], uint32_t &anchor)
{
    constexpr uint32_t MASK = (1u << Q) - 1u, HALF = 1u << (Q - 1);
    const uint32_t n = e.n[plane];
    const int64_t base = e.off[plane] + 4 * (int64_t)g * Q;
    const bool whole = 32u * g + 32u <= n;             // (g < 2^26)
    uint32_t d[Q];
    if (whole) {
#pragma unroll
        for (int i = 0; i < Q; ++i) d[i] = pk_bits_ld4<NT>(e, fb, base + 4 * i);
    } else {
        // the plane ends in this group: byte by byte up to the last byte that holds a sample
        const int64_t end = e.off[plane] + e.bytes[plane];
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            d[i] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (base + 4 * i + k < end) d[i] |= pk_bits_ld1(e, fb, base + 4 * i + k) << (8 * k);
        }
    }
    uint32_t c[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const int w = (j * Q) >> 5, s = (j * Q) & 31;
        uint32_t v = d[w] >> s;
        if (s + Q > 32) v |= d[(w + 1) % Q] << ((32 - s) & 31);     // (w + 1 < Q whenever a code straddles)
        c[j] = v & MASK;
    }
    if (!whole) {
        // behind the last sample: the last real code again (bits there are never read into a value)
#pragma unroll
        for (int j = 1; j < 32; ++j)
            if (32u * g + (uint32_t)j >= n) c[j] = c[j - 1];
    }
    anchor = c[0];
    uint32_t any = 0;
    u[0] = 0;
#pragma unroll
    for (int j = 1; j < 32; ++j) {
        const uint32_t r = (c[j] - c[j - 1]) & MASK;
        u[j] = r < HALF ? 2u * r : 2u * (MASK + 1u - r) - 1u;
        any |= u[j];
    }
    return any ? 32u - (uint32_t)__builtin_clz(any) : 0u;
}

// k_pack_scan on `nframes` frames: the workspace's block totals -> their exclusive prefix sums, e.sizes[frame] (when not NULL) =
// e.payload_offset + 4 * the frame's total
int pack_scan_launch(PkArgs &e, int nframes, hipStream_t stream);

} // namespace csic
