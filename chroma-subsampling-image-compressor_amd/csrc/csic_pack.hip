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
// Every global access goes through the accessors of csic_pack_common.h, which the CSIC_DEBUG build checks against frame_bytes,
// bound_bytes and the workspace's entries.  CSIC_TUNE_NONTEMPORAL selects the accesses of the PLANAR_BITS frames; the block size is fixed.
// csic_pack_common.h holds what csic_rice.hip does as well -- the group load, the store of a block's sections, the nibble and anchor reads,
// the repacking and store of a decoded group, and the launch side's filler, refusals and per-width launches; this unit holds their
// non-template bodies (pk_fill_args, pk_check_buffers, pack_scan_launch with k_pack_scan, pk_kernel_name).
#include <cstdio>

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
    pk_store_sections<Q>(e, cb, plane, G, g0, s_w, s_a);
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
    return min(pk_nibble(e, cb, plane, g), (uint32_t)e.q[plane]);
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
    uint32_t c = pk_anchor<Q>(e, cb, plane, g);
    // 32 steps of the prefix, the payload dwords loaded as they are used up: 32 w bits = exactly w loads
    const uint32_t n = e.n[plane], wmask = (1u << w) - 1u;
    int64_t at = e.payload_offset + 4 * ((int64_t)*pk_ws(e, blockIdx.z, e.block0[plane] + blockIdx.x) + before);
    uint64_t acc = 0;
    uint32_t have = 0;
    PkGroupOut<Q> out;
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
        if (j > 0) c = (c + rice_unfold(uu, MASK)) & MASK;
        out.put(j, 32u * g + (uint32_t)j < n ? c : 0u);                     // slots behind the last sample: zero bits
    }
    out.template store<NT>(e, pk_bits_frame(e), plane, g);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int pk_fill_args(const csic_plan *pl, const PackGeometry &G, const int64_t (&nibbles_offset)[3], const int64_t (&anchors_offset)[3],
                 int64_t payload_offset, int64_t bound_bytes, const char *entry, PkArgs *e)
{
    *e = PkArgs{};
    if ((int64_t)pl->g.W * pl->g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for %s", entry);
    e->frame_bytes = G.bits.frame_bytes;
    e->bound_bytes = bound_bytes;
    e->payload_offset = payload_offset;
    for (int p = 0; p < 3; ++p) {
        e->off[p] = G.src_offset[p];
        e->bytes[p] = G.src_bytes[p];
        e->n[p] = (uint32_t)G.n[p];
        e->groups[p] = (uint32_t)G.layout.groups[p];
        e->q[p] = G.q[p];
        e->woff[p] = (uint32_t)nibbles_offset[p];
        e->aoff[p] = (uint32_t)anchors_offset[p];
        e->adw[p] = (uint32_t)((G.layout.groups[p] * G.q[p] + 31) / 32);
        e->block0[p] = (uint32_t)G.block0[p];
    }
    e->nblocks = (uint32_t)G.nblocks;
    return CSIC_OK;
}

static int fill_pk_args(const csic_plan *pl, PkArgs *e)
{
    PackGeometry G;
    const int st = pack_geometry(&pl->p, &G);
    if (st != CSIC_OK) return st;
    return pk_fill_args(pl, G, G.layout.widths_offset, G.layout.anchors_offset, G.layout.payload_offset, G.layout.bound_bytes, "csic_pack_device", e);
}

static const auto pack_widths = [](auto q, auto nt) { return k_pack_widths<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto pack_emit = [](auto q, auto nt) { return k_pack_emit<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto unpack_emit = [](auto q, auto nt) { return k_unpack_emit<CSIC_CONST(q), CSIC_CONST(nt)>; };

int pack_scan_launch(PkArgs &e, int nframes, hipStream_t stream) { return launch(k_pack_scan, dim3((unsigned)nframes, 1, 1), dim3(PK_T, 1, 1), stream, e); }

int pk_check_buffers(const csic_plan *plan, const void *d_bits, const void *d_coded, int32_t nframes, bool has_ws, const void *d_workspace)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_bits || !d_coded || (has_ws && !d_workspace)) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if (((uintptr_t)d_bits | (uintptr_t)d_coded) & 255u) return set_error(CSIC_EINVAL_SIZE, "PLANAR_BITS and coded frame buffers must be 256-byte aligned");
    if (has_ws && ((uintptr_t)d_workspace & 7u)) return set_error(CSIC_EINVAL_SIZE, "d_workspace must be 8-byte aligned");
    return CSIC_OK;
}

const char *pk_kernel_name(const char *family, const csic_plan *plan)
{
    static thread_local char buf[64];
    if (!plan) return "";
    std::snprintf(buf, sizeof buf, "%s<q%d,%d,%d,%s>", family, plan->p.y_bits, plan->p.cb_bits, plan->p.cr_bits, plan->tune.no_nt ? "cached" : "nt");
    return buf;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_pack_kernel_name(const csic_plan *plan) { return pk_kernel_name("k_pack", plan); }

int csic_pack_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes) { return pk_workspace_bytes(plan, nframes, bytes, fill_pk_args); }

int csic_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace,
                     size_t workspace_bytes, void *hip_stream)
{
    if (plan && !d_sizes) return set_error(CSIC_EINVAL_NULL, "d_sizes is NULL");
    PkArgs e;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, true, d_workspace, workspace_bytes, fill_pk_args, &e);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_sizes & 7u) return set_error(CSIC_EINVAL_SIZE, "d_sizes must be 8-byte aligned");
    e.sizes = reinterpret_cast<unsigned long long *>(d_sizes);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = pk_launch_planes(plan, e, nframes, stream, pack_widths)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(e, nframes, stream)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, e, nframes, stream, pack_emit)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *d_workspace, size_t workspace_bytes,
                       void *hip_stream)
{
    PkArgs e;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, true, d_workspace, workspace_bytes, fill_pk_args, &e);
    if (st != CSIC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    uint32_t gmax = 0;
    for (int p = 0; p < 3; ++p) gmax = e.groups[p] > gmax ? e.groups[p] : gmax;
    if ((st = launch(k_unpack_sums, dim3((gmax + PK_T - 1) / PK_T, 3, (unsigned)nframes), dim3(PK_T, 1, 1), stream, e)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(e, nframes, stream)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, e, nframes, stream, unpack_emit)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
