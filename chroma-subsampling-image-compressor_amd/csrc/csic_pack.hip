// csic_pack.hip -- the device codec of the group coding (csic_pack_device, csic_unpack_device): CSIC_FMT_PLANAR_BITS frames to coded
// frames and back, lossless.  The format is stated in include/csic.h; csic_pack_host.cpp is the host codec and owns the geometry.
//
// Mapping (as k_cstat_bits): one lane per GROUP of 32 samples = exactly Q dwords of the source, Q a template parameter, so every code
// is cut out with compile-time shifts; 256-thread blocks of 256 consecutive groups of one plane; plane = plane0 + blockIdx.y, frame =
// blockIdx.z; planes of different widths go out as separate launches.  A frame's blocks are numbered Y, Cb, Cr (block0[plane] +
// blockIdx.x) and own one uint32 each in the workspace, [frame][block].  Per direction three passes in stream order -- the launches are
// the only ordering, no block ever waits for another:
//   pack    k_pack_widths<Q, NT>    a lane loads its group, folds the residuals and finds w.  Through LDS the block assembles its 256
//                                   nibbles into 32 dwords and its 256 anchors into 8 Q dwords (a block's first group is a multiple of
//                                   256: both strings start on a dword) and stores them whole; the block's sum of w -> workspace.
//           k_pack_scan             one block per frame: exclusive scan of the frame's block totals in place, looping when there are
//                                   more blocks than threads; d_sizes[frame] = fixed_bytes + 4 * total.
//           k_pack_emit<Q, NT>      recomputes u from the source (about one byte per pixel: a second read is cheaper than a stash), a
//                                   block-local scan of w gives each lane's dword offset behind the block's, the lane writes its w
//                                   dwords one after the other (lanes write runs of w dwords side by side: not whole lines).
//   unpack  k_unpack_sums           a lane reads its nibble, w = min(nibble, q); the block's sum -> workspace.
//           k_pack_scan             the same kernel, without d_sizes.
//           k_unpack_emit<Q, NT>    a lane reads its anchor, w and its w dwords -- one at a time, as the 32-step prefix in registers
//                                   uses them up -- and stores Q dwords.
// The plane's last group may be ragged: it is loaded and stored byte by byte up to the last byte that holds a sample, its slots
// behind the last sample repeat the last code (pack) and are stored as zero bits (unpack).  Nothing is validated on the device: with
// w <= q no payload offset leaves fixed_bytes + 4 sum G_p q_p <= bound_bytes, whatever the nibbles say.
// Every global access goes through the accessors of csic_pack_common.h (shared with csic_rice.hip), which the CSIC_DEBUG build checks against frame_bytes, bound_bytes and the
// workspace's entries.  CSIC_TUNE_NONTEMPORAL selects the accesses of the PLANAR_BITS frames; the block size is fixed.
#include <cstdio>
#include <cstring>

#include "csic_pack_common.h"

namespace csic {

// ------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_pack_widths(PkArgs e)
{
    __shared__ uint32_t s_w[PK_T], s_a[PK_T], s_tot[PK_WAVES];
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x;
    if (g0 >= G) return;                                                    // block-uniform, before any barrier
    const gpdst_t cb = pk_coded_frame(e);
    uint32_t w = 0, anchor = 0;
    if (g0 + t < G) {
        uint32_t u[32];
        w = pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g0 + t, u, anchor);
    }
    s_w[t] = w;                                                             // groups behind the plane's last: 0, the sections' padding
    s_a[t] = anchor;
    uint32_t total;
    (void)pk_block_scan(w, s_tot, total);                                   // (its barriers also publish s_w and s_a)
    if (t == 0) *pk_ws(e, blockIdx.z, e.block0[plane] + blockIdx.x) = total;
    if (t < 32u) {
        // wave 0: dword t of the block's nibbles = groups g0 + 8 t .. + 7
        if (g0 + 8u * t < G) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v |= s_w[8u * t + (uint32_t)k] << (4 * k);
            pk_coded_st4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(g0 / 8u + t), v);
        }
    } else if (t >= 64u && t < 64u + 8u * Q) {
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

// One block per frame (blockIdx.x): the frame's block totals -> their exclusive prefix sums, in place.
__global__ void __launch_bounds__(PK_T) k_pack_scan(PkArgs e)
{
    __shared__ uint32_t s_tot[PK_WAVES];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < e.nblocks; b0 += PK_T) {                     // block-uniform
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < e.nblocks ? *pk_ws(e, blockIdx.x, b) : 0u;
        uint32_t total;
        const uint32_t before = pk_block_scan(v, s_tot, total);
        if (b < e.nblocks) *pk_ws(e, blockIdx.x, b) = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0 && e.sizes)
        ((unsigned long long CSIC_GLOBAL *)(uintptr_t)e.sizes)[blockIdx.x] = (unsigned long long)e.payload_offset + 4ull * carry;
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_pack_emit(PkArgs e)
{
    __shared__ uint32_t s_tot[PK_WAVES];
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x;
    if (g0 >= G) return;
    uint32_t u[32], w = 0, anchor = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = 0;
    if (g0 + t < G) w = pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g0 + t, u, anchor);
    uint32_t total;
    const uint32_t before = pk_block_scan(w, s_tot, total);
    if (w == 0) return;
    const gpdst_t cb = pk_coded_frame(e);
    int64_t at = e.payload_offset + 4 * ((int64_t)*pk_ws(e, blockIdx.z, e.block0[plane] + blockIdx.x) + before);
    uint64_t acc = 0;
    uint32_t fill = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {                                          // 32 w bits: exactly w stores
        acc |= (uint64_t)u[j] << fill;
        fill += w;
        if (fill >= 32u) {
            pk_coded_st4(e, cb, at, (uint32_t)acc);
            at += 4;
            acc >>= 32;
            fill -= 32u;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// unpack
// ------------------------------------------------------------------------------------------------
// the width of group g as the device takes it: never above q
__device__ __forceinline__ uint32_t pk_width(const PkArgs &e, gpdst_t cb, int plane, uint32_t g)
{
    const uint32_t d = pk_coded_ld4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(g >> 3));
    return min((d >> (4u * (g & 7u))) & 15u, (uint32_t)e.q[plane]);
}

__global__ void __launch_bounds__(PK_T) k_unpack_sums(PkArgs e)
{
    __shared__ uint32_t s_tot[PK_WAVES];
    const int plane = (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x;
    if (g0 >= G) return;
    const uint32_t w = g0 + t < G ? pk_width(e, pk_coded_frame(e), plane, g0 + t) : 0u;
    uint32_t total;
    (void)pk_block_scan(w, s_tot, total);
    if (t == 0) *pk_ws(e, blockIdx.z, e.block0[plane] + blockIdx.x) = total;
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_unpack_emit(PkArgs e)
{
    constexpr uint32_t MASK = (1u << Q) - 1u;
    __shared__ uint32_t s_tot[PK_WAVES];
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t;
    if (g0 >= G) return;
    const gpdst_t cb = pk_coded_frame(e);
    const uint32_t w = g < G ? pk_width(e, cb, plane, g) : 0u;
    uint32_t total;
    const uint32_t before = pk_block_scan(w, s_tot, total);
    if (g >= G) return;
    // the anchor: Q bits at [g Q, g Q + Q) of the anchors section (g Q < 2^29)
    const uint32_t abit = g * Q, as = abit & 31u;
    const int64_t aat = (int64_t)e.aoff[plane] + 4 * (int64_t)(abit >> 5);
    uint32_t c = pk_coded_ld4(e, cb, aat) >> as;
    if (as + Q > 32u) c |= pk_coded_ld4(e, cb, aat + 4) << (32u - as);     // (a straddling code has both dwords inside the section)
    c &= MASK;
    // 32 steps of the prefix, the payload dwords loaded as they are used up: 32 w bits = exactly w loads
    const uint32_t n = e.n[plane], wmask = (1u << w) - 1u;
    int64_t at = e.payload_offset + 4 * ((int64_t)*pk_ws(e, blockIdx.z, e.block0[plane] + blockIdx.x) + before);
    uint64_t acc = 0;
    uint32_t have = 0, d[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) d[i] = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (have < w) {
            acc |= (uint64_t)pk_coded_ld4(e, cb, at) << have;
            at += 4;
            have += 32u;
        }
        const uint32_t uu = (uint32_t)acc & wmask;
        acc >>= w;
        have -= w;
        if (j > 0) c = (c + (((uu & 1u) ? ~(uu >> 1) : (uu >> 1)))) & MASK;
        const uint32_t v = 32u * g + (uint32_t)j < n ? c : 0u;              // slots behind the last sample: zero bits
        const int wi = (j * Q) >> 5, s = (j * Q) & 31;
        d[wi] |= v << s;
        if (s + Q > 32) d[(wi + 1) % Q] |= v >> ((32 - s) & 31);
    }
    const gpdst_t fb = pk_bits_frame(e);
    const int64_t base = e.off[plane] + 4 * (int64_t)g * Q;
    if (32u * g + 32u <= n) {
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

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using PkFn = void (*)(PkArgs);

static int fill_pk_args(const csic_plan *pl, PkArgs *e)
{
    std::memset(e, 0, sizeof *e);
    PackGeometry G;
    const int st = pack_geometry(&pl->p, &G);
    if (st != CSIC_OK) return st;
    if ((int64_t)pl->g.W * pl->g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for csic_pack_device");
    e->frame_bytes = G.bits.frame_bytes;
    e->bound_bytes = G.layout.bound_bytes;
    e->payload_offset = G.layout.payload_offset;
    uint32_t blocks = 0;
    for (int p = 0; p < 3; ++p) {
        e->off[p] = G.src_offset[p];
        e->bytes[p] = G.src_bytes[p];
        e->n[p] = (uint32_t)G.n[p];
        e->groups[p] = (uint32_t)G.layout.groups[p];
        e->q[p] = G.q[p];
        e->woff[p] = (uint32_t)G.layout.widths_offset[p];
        e->aoff[p] = (uint32_t)G.layout.anchors_offset[p];
        e->adw[p] = (uint32_t)((G.layout.groups[p] * G.q[p] + 31) / 32);
        e->block0[p] = blocks;
        blocks += (e->groups[p] + PK_T - 1) / PK_T;
    }
    e->nblocks = blocks;
    return CSIC_OK;
}

static PkFn pk_kernel(int which, int q, bool nt)       // 0 = k_pack_widths, 1 = k_pack_emit, 2 = k_unpack_emit
{
    return with_const<true, false>(nt, [&](auto n) -> PkFn {
        constexpr bool NT = CSIC_CONST(n);
        return with_const<1, 2, 3, 4, 5, 6, 7, 8>(q, [&](auto qq) -> PkFn {
            constexpr int Q = CSIC_CONST(qq);
            return which == 0 ? k_pack_widths<Q, NT> : which == 1 ? k_pack_emit<Q, NT> : k_unpack_emit<Q, NT>;
        });
    });
}

// one launch per run of planes of equal width
static int pk_launch_planes(const csic_plan *plan, PkArgs &e, int which, int nframes, hipStream_t stream)
{
    for (int p0 = 0; p0 < 3;) {
        int p1 = p0 + 1;
        while (p1 < 3 && e.q[p1] == e.q[p0]) ++p1;
        uint32_t gmax = 0;
        for (int p = p0; p < p1; ++p) gmax = e.groups[p] > gmax ? e.groups[p] : gmax;
        if (gmax > 0) {
            e.plane0 = p0;
            const PkFn fn = pk_kernel(which, e.q[p0], !plan->tune.no_nt);
            void *params[1] = {&e};
            HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(fn), dim3((gmax + PK_T - 1) / PK_T, (unsigned)(p1 - p0), (unsigned)nframes),
                                    dim3(PK_T, 1, 1), params, 0, stream));
        }
        p0 = p1;
    }
    return CSIC_OK;
}

static int pk_launch(PkFn fn, PkArgs &e, dim3 grid, hipStream_t stream)
{
    void *params[1] = {&e};
    HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(fn), grid, dim3(PK_T, 1, 1), params, 0, stream));
    return CSIC_OK;
}

int pack_scan_launch(PkArgs &e, int nframes, hipStream_t stream) { return pk_launch(k_pack_scan, e, dim3((unsigned)nframes, 1, 1), stream); }

// everything both directions refuse, before any device is touched
static int pk_prepare(const csic_plan *plan, const void *d_bits, const void *d_coded, int32_t nframes, const void *d_workspace,
                      size_t workspace_bytes, PkArgs *e)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_bits || !d_coded || !d_workspace) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if (((uintptr_t)d_bits | (uintptr_t)d_coded) & 255u) return set_error(CSIC_EINVAL_SIZE, "PLANAR_BITS and coded frame buffers must be 256-byte aligned");
    if ((uintptr_t)d_workspace & 7u) return set_error(CSIC_EINVAL_SIZE, "d_workspace must be 8-byte aligned");
    const int st = fill_pk_args(plan, e);
    if (st != CSIC_OK) return st;
    const size_t need = ((size_t)nframes * e->nblocks * sizeof(uint32_t) + 7) / 8 * 8;
    if (workspace_bytes < need) return set_error(CSIC_EINVAL_SIZE, "workspace of %zu bytes, %d frames need %zu", workspace_bytes, nframes, need);
    e->bits = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_bits));
    e->coded = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_coded));
    e->ws = const_cast<uint32_t *>(static_cast<const uint32_t *>(d_workspace));
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_pack_kernel_name(const csic_plan *plan)
{
    static thread_local char buf[64];
    if (!plan) return "";
    std::snprintf(buf, sizeof buf, "k_pack<q%d,%d,%d,%s>", plan->p.y_bits, plan->p.cb_bits, plan->p.cr_bits, plan->tune.no_nt ? "cached" : "nt");
    return buf;
}

int csic_pack_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes)
{
    if (!plan || !bytes) return set_error(CSIC_EINVAL_NULL, "plan or bytes is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    PkArgs e;
    const int st = fill_pk_args(plan, &e);
    if (st != CSIC_OK) return st;
    *bytes = ((size_t)nframes * e.nblocks * sizeof(uint32_t) + 7) / 8 * 8;
    clear_error();
    return CSIC_OK;
}

int csic_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace,
                     size_t workspace_bytes, void *hip_stream)
{
    if (plan && !d_sizes) return set_error(CSIC_EINVAL_NULL, "d_sizes is NULL");
    PkArgs e;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, d_workspace, workspace_bytes, &e);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_sizes & 7u) return set_error(CSIC_EINVAL_SIZE, "d_sizes must be 8-byte aligned");
    e.sizes = reinterpret_cast<unsigned long long *>(d_sizes);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = pk_launch_planes(plan, e, 0, nframes, stream)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(e, nframes, stream)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, e, 1, nframes, stream)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *d_workspace, size_t workspace_bytes,
                       void *hip_stream)
{
    PkArgs e;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, d_workspace, workspace_bytes, &e);
    if (st != CSIC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    uint32_t gmax = 0;
    for (int p = 0; p < 3; ++p) gmax = e.groups[p] > gmax ? e.groups[p] : gmax;
    if ((st = pk_launch(k_unpack_sums, e, dim3((gmax + PK_T - 1) / PK_T, 3, (unsigned)nframes), stream)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(e, nframes, stream)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, e, 2, nframes, stream)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
