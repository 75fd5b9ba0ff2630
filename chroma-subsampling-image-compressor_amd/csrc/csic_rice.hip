// csic_rice.hip -- the device codec of the Rice coding (csic_rice_pack_device, csic_rice_unpack_device): CSIC_FMT_PLANAR_BITS frames to
// coded frames and back, lossless.  The format is stated in include/csic.h; csic_rice_host.cpp is the host codec and owns the geometry.
//
// Mapping, as csic_pack.hip (whose argument, accessors, block scan and group load this unit shares through csic_pack_common.h): one lane
// per GROUP of 32 samples, Q a template parameter, 256-thread blocks of 256 consecutive groups of one plane -- a block of the kernels is
// a block of the format, it owns one chunk of the payload and one directory entry; planes of different widths go out as separate
// launches.
//   pack    k_rice_modes<Q, NT>   a lane loads its group, folds the residuals, prices k = 0 .. Q and keeps the cheapest.  The block
//                                 stores its 256 nibbles and anchors whole (as k_pack_widths) and its chunk's dwords -> workspace.
//           k_pack_scan           the group coding's scan: chunk offsets in place, d_sizes[frame] from the total.
//           k_rice_emit<Q, NT>    recomputes u and the mode, a block scan of the (R bits, U bits) pairs gives each lane its two bit
//                                 offsets; the chunk is assembled in LDS: a lane packs its bits in registers and stores the dwords it
//                                 owns alone plainly; only the first dword of a run and its unfinished last one, which neighbours share,
//                                 are ORed atomically into the cleared buffer.  The block stores the chunk as consecutive dwords,
//                                 thread 0 the directory entry, the frame's last block dir[NB] as well.
//   unpack  k_rice_unpack<Q, NT>  ONE pass, no workspace: a block reads dir[b], dir[b + 1], copies its chunk to LDS, scans the lanes'
//                                 (R bits, unary group) pairs, counts the terminators of U per dword and scans those; a lane finds the
//                                 dword that holds terminator 31 z by bisection, the bit inside it by a select, then reads 31 slots.
// The bit reads of unpack are csic_rice_decode.h's, which the host codec and tests/cpp/rice_fuzz.cpp run on the host.  Nothing is
// validated on the device; instead every extent is clamped: a nibble takes part as min(m, Q) (15: zero mode), dir[b] and dir[b + 1] to
// the frame's (bound_bytes - payload_offset) / 4 dwords and the chunk to the 248 Q + 1 dwords of the LDS buffer, the R / U split to the
// chunk, every bit read to the chunk (a unary run ends with it), u to Q bits.  CSIC_TUNE_NONTEMPORAL selects the accesses of the
// PLANAR_BITS frames; the block size is fixed.
#include <cstdio>
#include <cstring>

#include "csic_pack_common.h"
#include "csic_rice_decode.h"

namespace csic {

static_assert(PK_T == RICE_BLOCK, "a block of the kernels is a block of the format");

struct RcArgs {
    PkArgs pk;                     // woff: the modes sections; payload_offset, bound_bytes: the Rice coding's
    uint32_t dir_off;              // byte offset of the directory
    uint32_t max_dwords;           // (bound_bytes - payload_offset) / 4: no payload dword of a frame lies behind
};

template <int Q> struct RcCap { static constexpr uint32_t DW = 248u * Q + 1u; };     // dwords of the longest chunk

// The mode of a group with folded residuals u (w = the significant bits of their OR): 15, or the cheapest k = 0 .. Q, the smallest on
// a tie.  rbits / ubits: what the group adds to R and U.
template <int Q>
__device__ __forceinline__ uint32_t rc_mode(const uint32_t (&u)[32], uint32_t w, uint32_t &rbits, uint32_t &ubits)
{
    rbits = ubits = 0;
    if (w == 0) return 15u;
    uint32_t best = Q, cost = 31u * Q;
#pragma unroll
    for (int k = Q - 1; k >= 0; --k) {
        uint32_t s = 31u;
#pragma unroll
        for (int j = 1; j < 32; ++j) s += u[j] >> k;
        if (31u * (uint32_t)k + s <= cost) { cost = 31u * (uint32_t)k + s; best = (uint32_t)k; ubits = s; }
    }
    rbits = 31u * best;
    return best;
}

// a lane's run of bits inside the chunk that the block assembles in LDS
template <int Q> struct RcWriter {
    uint32_t *s;
    uint32_t wi, fill;
    uint64_t acc;
    bool first;
    __device__ __forceinline__ RcWriter(uint32_t *chunk, uint32_t bit) : s(chunk), wi(bit >> 5), fill(bit & 31u), acc(0), first(true) {}
    __device__ __forceinline__ void flush()            // a finished dword: the run's first is shared with the lane before
    {
        CSIC_CHECK(wi < RcCap<Q>::DW);
        if (first) atomicOr(&s[wi], (uint32_t)acc); else s[wi] = (uint32_t)acc;
        first = false;
        ++wi;
        acc >>= 32;
        fill -= 32u;
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t n)     // n <= 8 bits
    {
        acc |= (uint64_t)v << fill;
        fill += n;
        if (fill >= 32u) flush();
    }
    __device__ __forceinline__ void unary(uint32_t zeros)           // zeros < 256
    {
        fill += zeros;
        while (fill >= 32u) flush();
        put(1u, 1u);
    }
    __device__ __forceinline__ void finish()           // the unfinished last dword is shared with the lane behind
    {
        if (fill > 0 && (uint32_t)acc != 0) {
            CSIC_CHECK(wi < RcCap<Q>::DW);
            atomicOr(&s[wi], (uint32_t)acc);
        }
    }
};

// ------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_rice_modes(RcArgs a)
{
    __shared__ uint32_t s_m[PK_T], s_a[PK_T], s_tot[PK_WAVES];
    const PkArgs &e = a.pk;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x;
    if (g0 >= G) return;                                                    // block-uniform, before any barrier
    const gpdst_t cb = pk_coded_frame(e);
    uint32_t m = 0, anchor = 0, rbits = 0, ubits = 0;
    if (g0 + t < G) {
        uint32_t u[32];
        const uint32_t w = pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g0 + t, u, anchor);
        m = rc_mode<Q>(u, w, rbits, ubits);
    }
    s_m[t] = m;                                                             // groups behind the plane's last: 0, the sections' padding
    s_a[t] = anchor;
    uint32_t total;
    (void)pk_block_scan((rbits << 16) | ubits, s_tot, total);               // (each sum <= 256 * 248 < 2^16; the barriers publish s_m, s_a)
    if (t == 0) *pk_ws(e, blockIdx.z, e.block0[plane] + blockIdx.x) = ((total >> 16) + 31u) / 32u + ((total & 0xFFFFu) + 31u) / 32u;
    if (t < 32u) {
        // wave 0: dword t of the block's nibbles = groups g0 + 8 t .. + 7
        if (g0 + 8u * t < G) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v |= s_m[8u * t + (uint32_t)k] << (4 * k);
            pk_coded_st4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(g0 / 8u + t), v);
        }
    } else if (t >= 64u && t < 64u + 8u * Q) {
        // wave 1: dword i of the block's anchors = bits [32 i, 32 i + 32) of 256 codes at Q bits
        const uint32_t i0 = t - 64u, dw = blockIdx.x * (8u * Q) + i0;
        if (dw < e.adw[plane]) {
            uint32_t v = 0;
            for (uint32_t i = 32u * i0 / Q; i * Q < 32u * i0 + 32u; ++i) {  // (i < 256: the block's string is 256 Q bits)
                const int sh = (int)(i * Q) - (int)(32u * i0);
                v |= sh >= 0 ? s_a[i] << sh : s_a[i] >> -sh;
            }
            pk_coded_st4(e, cb, (int64_t)e.aoff[plane] + 4 * (int64_t)dw, v);
        }
    }
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_rice_emit(RcArgs a)
{
    __shared__ uint32_t s_chunk[RcCap<Q>::DW], s_tot[PK_WAVES];
    const PkArgs &e = a.pk;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x;
    if (g0 >= G) return;
    uint32_t u[32], m = 15u, anchor = 0, rbits = 0, ubits = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = 0;
    if (g0 + t < G) {
        const uint32_t w = pk_fold_group<Q, NT>(e, pk_bits_frame(e), plane, g0 + t, u, anchor);
        m = rc_mode<Q>(u, w, rbits, ubits);
    }
    uint32_t total;
    const uint32_t before = pk_block_scan((rbits << 16) | ubits, s_tot, total);
    const uint32_t rdw = ((total >> 16) + 31u) / 32u, ndw = rdw + ((total & 0xFFFFu) + 31u) / 32u;      // <= 248 Q + 1
    CSIC_CHECK(ndw <= RcCap<Q>::DW);
    for (uint32_t i = t; i < ndw; i += PK_T) s_chunk[i] = 0;
    __syncthreads();
    if (m != 15u) {
        const uint32_t kmask = (1u << m) - 1u;
        if (m > 0) {
            RcWriter<Q> R(s_chunk, before >> 16);
#pragma unroll
            for (int j = 1; j < 32; ++j) R.put(u[j] & kmask, m);
            R.finish();
        }
        if (m < (uint32_t)Q) {
            RcWriter<Q> U(s_chunk, 32u * rdw + (before & 0xFFFFu));
#pragma unroll
            for (int j = 1; j < 32; ++j) U.unary(u[j] >> m);
            U.finish();
        }
    }
    __syncthreads();
    const gpdst_t cb = pk_coded_frame(e);
    const uint32_t blk = e.block0[plane] + blockIdx.x, base = *pk_ws(e, blockIdx.z, blk);
    for (uint32_t i = t; i < ndw; i += PK_T) pk_coded_st4(e, cb, e.payload_offset + 4 * ((int64_t)base + i), s_chunk[i]);
    if (t == 0) {
        pk_coded_st4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)blk, base);
        if (blk + 1u == e.nblocks) pk_coded_st4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)e.nblocks, base + ndw);
    }
}

// ------------------------------------------------------------------------------------------------
// unpack
// ------------------------------------------------------------------------------------------------
template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_rice_unpack(RcArgs a)
{
    constexpr uint32_t MASK = (1u << Q) - 1u, CAP = RcCap<Q>::DW, WPT = (CAP + PK_T - 1) / PK_T;       // U dwords per thread
    __shared__ uint32_t s_chunk[CAP], s_cum[CAP], s_tot[PK_WAVES];
    const PkArgs &e = a.pk;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t;
    if (g0 >= G) return;
    const gpdst_t cb = pk_coded_frame(e);
    const uint32_t blk = e.block0[plane] + blockIdx.x;
    // the mode as the device takes it: 15 is zero mode, anything else k = min(m, Q)
    uint32_t m = 15u;
    if (g < G) m = (pk_coded_ld4(e, cb, (int64_t)e.woff[plane] + 4 * (int64_t)(g >> 3)) >> (4u * (g & 7u))) & 15u;
    const bool zero = m == 15u;
    const uint32_t k = min(m, (uint32_t)Q);
    const bool unary = !zero && k < (uint32_t)Q;
    // the chunk, clamped to the frame and to the buffer, into LDS
    const uint32_t d0 = min(pk_coded_ld4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)blk), a.max_dwords);
    const uint32_t d1 = min(max(pk_coded_ld4(e, cb, (int64_t)a.dir_off + 4 * (int64_t)blk + 4), d0), a.max_dwords);
    const uint32_t nw = min(d1 - d0, CAP);
    for (uint32_t i = t; i < nw; i += PK_T) s_chunk[i] = pk_coded_ld4(e, cb, e.payload_offset + 4 * ((int64_t)d0 + i));
    uint32_t total;
    const uint32_t before = pk_block_scan(zero ? 0u : ((31u * k) << 16) | (unary ? 1u : 0u), s_tot, total);   // (its barriers publish s_chunk)
    const uint32_t rdw = min(((total >> 16) + 31u) / 32u, nw), uw = nw - rdw;
    // terminators per dword of U, and their running count
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t i = 0; i < WPT; ++i) {
        const uint32_t idx = t * WPT + i;
        if (idx < uw) cnt += (uint32_t)__builtin_popcount(s_chunk[rdw + idx]);
    }
    uint32_t ptotal;
    uint32_t run = pk_block_scan(cnt, s_tot, ptotal);
#pragma unroll
    for (uint32_t i = 0; i < WPT; ++i) {
        const uint32_t idx = t * WPT + i;
        if (idx < uw) {
            run += (uint32_t)__builtin_popcount(s_chunk[rdw + idx]);
            s_cum[idx] = run;
        }
    }
    __syncthreads();
    if (g >= G) return;
    // the anchor: Q bits at [g Q, g Q + Q) of the anchors section (g Q < 2^29)
    const uint32_t abit = g * Q, as = abit & 31u;
    const int64_t aat = (int64_t)e.aoff[plane] + 4 * (int64_t)(abit >> 5);
    uint32_t c = pk_coded_ld4(e, cb, aat) >> as;
    if (as + Q > 32u) c |= pk_coded_ld4(e, cb, aat + 4) << (32u - as);     // (a straddling code has both dwords inside the section)
    c &= MASK;
    // where the group's bits start: R by the scan, U behind terminator 31 z
    uint32_t rbit = before >> 16, ubit = 32u * rdw;
    if (unary) ubit += rice_after_terminator(s_chunk + rdw, s_cum, uw, 31u * (before & 0xFFFFu));
    const uint32_t n = e.n[plane], uend = 32u * nw;
    uint32_t d[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) d[i] = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j > 0 && !zero) c = (c + rice_unfold(rice_next_u(s_chunk, nw, &rbit, &ubit, uend, k, (uint32_t)Q), MASK)) & MASK;
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
            for (int kk = 0; kk < 4; ++kk)
                if (base + 4 * i + kk < end) pk_bits_st1(e, fb, base + 4 * i + kk, (d[i] >> (8 * kk)) & 0xFFu);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using RcFn = void (*)(RcArgs);

static int fill_rc_args(const csic_plan *pl, RcArgs *a)
{
    std::memset(a, 0, sizeof *a);
    RiceGeometry G;
    const int st = rice_geometry(&pl->p, &G);
    if (st != CSIC_OK) return st;
    if ((int64_t)pl->g.W * pl->g.H >= ((int64_t)1 << 31)) return set_error(CSIC_EINVAL_SIZE, "frame too large for csic_rice_pack_device");
    PkArgs &e = a->pk;
    e.frame_bytes = G.pk.bits.frame_bytes;
    e.bound_bytes = G.layout.bound_bytes;
    e.payload_offset = G.layout.payload_offset;
    for (int p = 0; p < 3; ++p) {
        e.off[p] = G.pk.src_offset[p];
        e.bytes[p] = G.pk.src_bytes[p];
        e.n[p] = (uint32_t)G.pk.n[p];
        e.groups[p] = (uint32_t)G.layout.groups[p];
        e.q[p] = G.pk.q[p];
        e.woff[p] = (uint32_t)G.layout.modes_offset[p];
        e.aoff[p] = (uint32_t)G.layout.anchors_offset[p];
        e.adw[p] = (uint32_t)((G.layout.groups[p] * G.pk.q[p] + 31) / 32);
        e.block0[p] = (uint32_t)G.block0[p];
    }
    e.nblocks = (uint32_t)G.nblocks;
    a->dir_off = (uint32_t)G.layout.directory_offset;
    a->max_dwords = (uint32_t)((G.layout.bound_bytes - G.layout.payload_offset) / 4);
    return CSIC_OK;
}

static RcFn rc_kernel(int which, int q, bool nt)       // 0 = k_rice_modes, 1 = k_rice_emit, 2 = k_rice_unpack
{
    return with_const<true, false>(nt, [&](auto n) -> RcFn {
        constexpr bool NT = CSIC_CONST(n);
        return with_const<1, 2, 3, 4, 5, 6, 7, 8>(q, [&](auto qq) -> RcFn {
            constexpr int Q = CSIC_CONST(qq);
            return which == 0 ? k_rice_modes<Q, NT> : which == 1 ? k_rice_emit<Q, NT> : k_rice_unpack<Q, NT>;
        });
    });
}

// one launch per run of planes of equal width
static int rc_launch_planes(const csic_plan *plan, RcArgs &a, int which, int nframes, hipStream_t stream)
{
    const PkArgs &e = a.pk;
    for (int p0 = 0; p0 < 3;) {
        int p1 = p0 + 1;
        while (p1 < 3 && e.q[p1] == e.q[p0]) ++p1;
        uint32_t gmax = 0;
        for (int p = p0; p < p1; ++p) gmax = e.groups[p] > gmax ? e.groups[p] : gmax;
        if (gmax > 0) {
            a.pk.plane0 = p0;
            const RcFn fn = rc_kernel(which, e.q[p0], !plan->tune.no_nt);
            void *params[1] = {&a};
            HIP_TRY(hipLaunchKernel(reinterpret_cast<const void *>(fn), dim3((gmax + PK_T - 1) / PK_T, (unsigned)(p1 - p0), (unsigned)nframes),
                                    dim3(PK_T, 1, 1), params, 0, stream));
        }
        p0 = p1;
    }
    return CSIC_OK;
}

// everything both directions refuse, before any device is touched
static int rc_prepare(const csic_plan *plan, const void *d_bits, const void *d_coded, int32_t nframes, RcArgs *a)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_bits || !d_coded) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    if (((uintptr_t)d_bits | (uintptr_t)d_coded) & 255u) return set_error(CSIC_EINVAL_SIZE, "PLANAR_BITS and coded frame buffers must be 256-byte aligned");
    const int st = fill_rc_args(plan, a);
    if (st != CSIC_OK) return st;
    a->pk.bits = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_bits));
    a->pk.coded = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_coded));
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_rice_kernel_name(const csic_plan *plan)
{
    static thread_local char buf[64];
    if (!plan) return "";
    std::snprintf(buf, sizeof buf, "k_rice<q%d,%d,%d,%s>", plan->p.y_bits, plan->p.cb_bits, plan->p.cr_bits, plan->tune.no_nt ? "cached" : "nt");
    return buf;
}

int csic_rice_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes)
{
    if (!plan || !bytes) return set_error(CSIC_EINVAL_NULL, "plan or bytes is NULL");
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be 1..65535. Got %d", nframes);
    RcArgs a;
    const int st = fill_rc_args(plan, &a);
    if (st != CSIC_OK) return st;
    *bytes = ((size_t)nframes * a.pk.nblocks * sizeof(uint32_t) + 7) / 8 * 8;
    clear_error();
    return CSIC_OK;
}

int csic_rice_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace,
                          size_t workspace_bytes, void *hip_stream)
{
    if (plan && !d_sizes) return set_error(CSIC_EINVAL_NULL, "d_sizes is NULL");
    if (plan && !d_workspace) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    RcArgs a;
    int st = rc_prepare(plan, d_bits, d_coded, nframes, &a);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_workspace & 7u) return set_error(CSIC_EINVAL_SIZE, "d_workspace must be 8-byte aligned");
    const size_t need = ((size_t)nframes * a.pk.nblocks * sizeof(uint32_t) + 7) / 8 * 8;
    if (workspace_bytes < need) return set_error(CSIC_EINVAL_SIZE, "workspace of %zu bytes, %d frames need %zu", workspace_bytes, nframes, need);
    if ((uintptr_t)d_sizes & 7u) return set_error(CSIC_EINVAL_SIZE, "d_sizes must be 8-byte aligned");
    a.pk.ws = static_cast<uint32_t *>(d_workspace);
    a.pk.sizes = reinterpret_cast<unsigned long long *>(d_sizes);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = rc_launch_planes(plan, a, 0, nframes, stream)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(a.pk, nframes, stream)) != CSIC_OK) return st;
    if ((st = rc_launch_planes(plan, a, 1, nframes, stream)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_rice_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *hip_stream)
{
    RcArgs a;
    int st = rc_prepare(plan, d_bits, d_coded, nframes, &a);
    if (st != CSIC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = rc_launch_planes(plan, a, 2, nframes, stream)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
