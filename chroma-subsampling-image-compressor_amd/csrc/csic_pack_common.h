// csic_pack_common.h -- what the device codecs of the group coding (csic_pack.hip), of the Rice coding (csic_rice.hip) and of the rANS
// coding (csic_rans.hip) share, and the temporal layer in front of them (csic_delta.hip) with them.
// Device: the kernels' argument, the checked accessors of the PLANAR_BITS and the coded frames, the block scan, the load of a group's
// dwords with the ragged-tail rule, the cut of one code and the fold of one residual, and from them the load of a group with its folded
// residuals, the store of a block's nibble and anchors sections, the reads of a group's nibble and anchor, and the
// accumulator that a decoded group is repacked in and stored from (the unfold u -> e is rice_unfold of csic_rice_decode.h, shared with
// the host codecs).  Host: the filler of the argument from pack_geometry and a coding's own offsets, the refusals and the workspace
// size of the entry points, the launch of one kernel per run of planes of equal width, the launch of the scan over a frame's block
// totals and the kernel-name formatter (their bodies, like k_pack_scan itself, live in csic_pack.hip).
#pragma once
#include "csic_kernel_ops.h"
#include "csic_rice_decode.h"

namespace csic {

typedef const uint8_t CSIC_GLOBAL *gpsrc_t;
typedef uint8_t CSIC_GLOBAL *gpdst_t;

constexpr int PK_T = 256, PK_WAVES = PK_T / 64;
static_assert(PK_T == RICE_BLOCK, "a block of the kernels is a block of the format: pack_geometry numbers both");

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

// the PLANAR_BITS frame: a dword (4-byte aligned) or a byte at a byte offset into its frame_bytes
template <bool NT> __device__ __forceinline__ uint32_t pk_bits_ld4(const PkArgs &e, gpdst_t fb, int64_t off) { return by_ld4<NT>(e.frame_bytes, fb, off); }
__device__ __forceinline__ uint32_t pk_bits_ld1(const PkArgs &e, gpdst_t fb, int64_t off) { return by_ld1(e.frame_bytes, fb, off); }
template <bool NT> __device__ __forceinline__ void pk_bits_st4(const PkArgs &e, gpdst_t fb, int64_t off, uint32_t v) { by_st4<NT>(e.frame_bytes, fb, off, v); }
__device__ __forceinline__ void pk_bits_st1(const PkArgs &e, gpdst_t fb, int64_t off, uint32_t v) { by_st1<false>(e.frame_bytes, fb, off, v); }
// the coded frame: dwords at a byte offset into its bound_bytes
__device__ __forceinline__ uint32_t pk_coded_ld4(const PkArgs &e, gpdst_t cb, int64_t off) { return by_ld4<false>(e.bound_bytes, cb, off); }
__device__ __forceinline__ void pk_coded_st4(const PkArgs &e, gpdst_t cb, int64_t off, uint32_t v) { by_st4<false>(e.bound_bytes, cb, off, v); }
// the workspace entry of block `b` of this block's frame (`frame` < 65535: the grid's z or, for the scan, x)
__device__ __forceinline__ gout_t pk_ws(const PkArgs &e, uint32_t frame, uint32_t b)
{
    CSIC_CHECK(b < e.nblocks && frame < 65535u);
    return (gout_t)(uintptr_t)e.ws + ((uint64_t)frame * e.nblocks + b);
}

__device__ __forceinline__ gpdst_t pk_bits_frame(const PkArgs &e) { return frame_at_z(e.bits, e.frame_bytes); }
__device__ __forceinline__ gpdst_t pk_coded_frame(const PkArgs &e) { return frame_at_z(e.coded, e.bound_bytes); }

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

// The Q dwords of group g of a plane: whole dwords, or -- the plane ends in this group -- byte by byte up to the last byte that holds
// a sample (the bytes behind it read as 0).
template <int Q, bool NT>
__device__ __forceinline__ void pk_load_group(const PkArgs &e, gpdst_t fb, int plane, uint32_t g, uint32_t (&d)[Q])
{
    const int64_t base = e.off[plane] + 4 * (int64_t)g * Q;
    if (32u * g + 32u <= e.n[plane]) {                 // (g < 2^26)
#pragma unroll
        for (int i = 0; i < Q; ++i) d[i] = pk_bits_ld4<NT>(e, fb, base + 4 * i);
    } else {
        const int64_t end = e.off[plane] + e.bytes[plane];
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            d[i] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (base + 4 * i + k < end) d[i] |= pk_bits_ld1(e, fb, base + 4 * i + k) << (8 * k);
        }
    }
}

// the code of slot j of a group's Q dwords (j a constant of an unrolled loop: compile-time shifts)
template <int Q> __device__ __forceinline__ uint32_t pk_code(const uint32_t (&d)[Q], int j)
{
    const int w = (j * Q) >> 5, s = (j * Q) & 31;
    uint32_t v = d[w] >> s;
    if (s + Q > 32) v |= d[(w + 1) % Q] << ((32 - s) & 31);         // (w + 1 < Q whenever a code straddles)
    return v & ((1u << Q) - 1u);
}

// the folded, centred residual u of a difference r = (c_j - c_(j - 1)) mod 2^Q
template <int Q> __device__ __forceinline__ uint32_t pk_fold(uint32_t r)
{
    constexpr uint32_t MASK = (1u << Q) - 1u, HALF = 1u << (Q - 1);
    return r < HALF ? 2u * r : 2u * (MASK + 1u - r) - 1u;
}

// Group g of a plane -> its 32 folded residuals, its width (returned) and its anchor.
template <int Q, bool NT>
__device__ __forceinline__ uint32_t pk_fold_group(const PkArgs &e, gpdst_t fb, int plane, uint32_t g, uint32_t (&u)[32], uint32_t &anchor)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    const uint32_t n = e.n[plane];
    const bool whole = 32u * g + 32u <= n;
    uint32_t d[Q];
    pk_load_group<Q, NT>(e, fb, plane, g, d);
    uint32_t c[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) c[j] = pk_code<Q>(d, j);
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
        u[j] = pk_fold<Q>((c[j] - c[j - 1]) & MASK);
        any |= u[j];
    }
    return any ? 32u - (uint32_t)__builtin_clz(any) : 0u;
}

// The block's 256 anchors (one per thread in LDS, 0 behind the plane's last group, published by a barrier) -> the 8 Q dwords of the
// plane's anchors section that the block owns; threads 64 .. 64 + 8 Q store one each.  Every thread of the block may call it.
template <int Q>
__device__ __forceinline__ void pk_store_anchors(const PkArgs &e, gpdst_t cb, int plane, const uint32_t *s_a)
{
    const uint32_t t = threadIdx.x;
    if (t >= 64u && t < 64u + 8u * Q) {
        // wave 1: dword a of the block's anchors = bits [32 a, 32 a + 32) of 256 codes at Q bits
        const uint32_t a = t - 64u, dw = blockIdx.x * (8u * Q) + a;
        if (dw < e.adw[plane]) {
            uint32_t v = 0;
            for (uint32_t i = 32u * a / Q; i * Q < 32u * a + 32u; ++i) {    // (i < 256: the block's string is 256 Q bits)
                const int sh = (int)(i * Q) - (int)(32u * a);
                v |= sh >= 0 ? s_a[i] << sh : s_a[i] >> -sh;
            }
            pk_coded_st4(e, cb, (int64_t)e.aoff[plane] + 4 * (int64_t)dw, v);
        }
    }
}

// The block's nibbles and anchors (one per thread in LDS, 0 behind the plane's last group: the sections' padding, and published by a
// barrier) -> the dwords of the plane's nibble and anchors sections.  A block's first group g0 is a multiple of 256: both strings start
// on a dword.  Every thread of the block calls it.
template <int Q>
__device__ __forceinline__ void pk_store_sections(const PkArgs &e, gpdst_t cb, int plane, uint32_t G, uint32_t g0, const uint32_t *s_nib, const uint32_t *s_a)
{
    const uint32_t t = threadIdx.x;
    if (t < 32u) {
        // wave 0: dword t of the block's nibbles = groups g0 + 8 t .. + 7
        if (g0 + 8u * t < G) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v |= s_nib[8u * t + (uint32_t)k] << (4 * k);
            pk_coded_st4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(g0 / 8u + t), v);
        }
    } else {
        pk_store_anchors<Q>(e, cb, plane, s_a);
    }
}

// the nibble of group g as the coded frame holds it
__device__ __forceinline__ uint32_t pk_nibble(const PkArgs &e, gpdst_t cb, int plane, uint32_t g)
{
    return (pk_coded_ld4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(g >> 3)) >> (4u * (g & 7u))) & 15u;
}

// the anchor of group g: Q bits at [g Q, g Q + Q) of the anchors section (g Q < 2^29)
template <int Q> __device__ __forceinline__ uint32_t pk_anchor(const PkArgs &e, gpdst_t cb, int plane, uint32_t g)
{
    const uint32_t abit = g * Q, as = abit & 31u;
    const int64_t aat = (int64_t)e.aoff[plane] + 4 * (int64_t)(abit >> 5);
    uint32_t c = pk_coded_ld4(e, cb, aat) >> as;
    if (as + Q > 32u) c |= pk_coded_ld4(e, cb, aat + 4) << (32u - as);     // (a straddling code has both dwords inside the section)
    return c & ((1u << Q) - 1u);
}

// The Q dwords of a decoded group in a lane's registers: slot j takes its code (j a constant of an unrolled loop: compile-time shifts),
// store() writes group g of the plane -- whole dwords, or byte by byte up to the plane's last byte when the plane ends in this group.
template <int Q> struct PkGroupOut {
    uint32_t d[Q];
    __device__ __forceinline__ PkGroupOut()
    {
#pragma unroll
        for (int i = 0; i < Q; ++i) d[i] = 0;
    }
    __device__ __forceinline__ void put(int j, uint32_t v)
    {
        const int wi = (j * Q) >> 5, s = (j * Q) & 31;
        d[wi] |= v << s;
        if (s + Q > 32) d[(wi + 1) % Q] |= v >> ((32 - s) & 31);
    }
    template <bool NT> __device__ __forceinline__ void store(const PkArgs &e, gpdst_t fb, int plane, uint32_t g) const
    {
        const int64_t base = e.off[plane] + 4 * (int64_t)g * Q;
        if (32u * g + 32u <= e.n[plane]) {
#pragma unroll
            for (int i = 0; i < Q; ++i) pk_bits_st4<NT>(e, fb, base + 4 * i, d[i]);
        } else {
            const int64_t end = e.off[plane] + e.bytes[plane];
#pragma unroll
            for (int i = 0; i < Q; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (base + 4 * i + k < end) pk_bits_st1(e, fb, base + 4 * i + k, (d[i] >> (8 * k)) & 0xFFu);
        }
    }
};

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The PkArgs of a coding from the group coding's geometry and the coding's own nibble and anchors offsets, payload_offset and
// bound_bytes; everything else is zero.  `entry` names the pack entry point in the refusal of a frame of 2^31 pixels or more.
int pk_fill_args(const csic_plan *pl, const PackGeometry &G, const int64_t (&nibbles_offset)[3], const int64_t (&anchors_offset)[3],
                 int64_t payload_offset, int64_t bound_bytes, const char *entry, PkArgs *e);

// the bytes of a workspace of one uint32 per block of `nframes` frames
inline size_t pk_workspace_need(int32_t nframes, uint32_t nblocks) { return ((size_t)nframes * nblocks * sizeof(uint32_t) + 7) / 8 * 8; }

// Below, Args is the argument struct of a coding's kernels: PkArgs, or a struct derived from it; fill(plan, &args) fills it from the
// plan's parameters.
// What the four device entry points refuse before any device is touched, then the arguments filled; `has_ws` is false for the one
// entry point without a workspace.  need(nframes, nblocks) is the coding's workspace size: one uint32 per block unless it says more.
int pk_check_buffers(const csic_plan *plan, const void *d_bits, const void *d_coded, int32_t nframes, bool has_ws, const void *d_workspace);
template <class Args>
int pk_prepare(const csic_plan *plan, const void *d_bits, const void *d_coded, int32_t nframes, bool has_ws, const void *d_workspace,
               size_t workspace_bytes, int (*fill)(const csic_plan *, Args *), Args *e, size_t (*need)(int32_t, uint32_t) = pk_workspace_need)
{
    int st = pk_check_buffers(plan, d_bits, d_coded, nframes, has_ws, d_workspace);
    if (st == CSIC_OK) st = fill(plan, e);
    if (st != CSIC_OK) return st;
    if (has_ws && workspace_bytes < need(nframes, e->nblocks))
        return set_error(CSIC_EINVAL_SIZE, "workspace of %zu bytes, %d frames need %zu", workspace_bytes, nframes, need(nframes, e->nblocks));
    e->bits = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_bits));
    e->coded = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_coded));
    e->ws = const_cast<uint32_t *>(static_cast<const uint32_t *>(d_workspace));
    return CSIC_OK;
}

// *_workspace_bytes of both codings
template <class Args>
int pk_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes, int (*fill)(const csic_plan *, Args *), size_t (*need)(int32_t, uint32_t) = pk_workspace_need)
{
    if (!plan || !bytes) return set_error(CSIC_EINVAL_NULL, "plan or bytes is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    Args e;
    const int st = fill(plan, &e);
    if (st != CSIC_OK) return st;
    *bytes = need(nframes, e.nblocks);
    clear_error();
    return CSIC_OK;
}

// One launch per run of planes of equal width; choose(Q, NT) maps the two constants to the kernel.  A block of `threads` threads takes
// `block_groups` consecutive groups of one plane (the group and Rice codings: 256 and 256; the rANS coding's wave per block: 1024 and 64).
template <class Args, class Choose>
int pk_launch_planes(const csic_plan *plan, Args &e, int nframes, hipStream_t stream, Choose choose, uint32_t block_groups = PK_T, uint32_t threads = PK_T)
{
    for (int p0 = 0; p0 < 3;) {
        int p1 = p0 + 1;
        while (p1 < 3 && e.q[p1] == e.q[p0]) ++p1;
        uint32_t gmax = 0;
        for (int p = p0; p < p1; ++p) gmax = e.groups[p] > gmax ? e.groups[p] : gmax;
        if (gmax > 0) {
            e.plane0 = p0;
            void (*const fn)(Args) = with_const<true, false>(!plan->tune.no_nt, [&](auto nt) {
                return with_const<1, 2, 3, 4, 5, 6, 7, 8>(e.q[p0], [&](auto q) -> void (*)(Args) { return choose(q, nt); });
            });
            const int st = launch(fn, dim3((gmax + block_groups - 1) / block_groups, (unsigned)(p1 - p0), (unsigned)nframes), dim3(threads, 1, 1), stream, e);
            if (st != CSIC_OK) return st;
        }
        p0 = p1;
    }
    return CSIC_OK;
}

// k_pack_scan on `nframes` frames: the workspace's block totals -> their exclusive prefix sums, e.sizes[frame] (when not NULL) =
// e.payload_offset + 4 * the frame's total
int pack_scan_launch(PkArgs &e, int nframes, hipStream_t stream);

// "<family><q y,cb,cr,nt|cached>" in a thread-local buffer: csic_pack_kernel_name, csic_rice_kernel_name
const char *pk_kernel_name(const char *family, const csic_plan *plan);

} // namespace csic
