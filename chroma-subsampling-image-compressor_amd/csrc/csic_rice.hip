// csic_rice.hip -- the device codec of the Rice coding (csic_rice_pack_device, csic_rice_unpack_device): CSIC_FMT_PLANAR_BITS frames to
// coded frames and back, lossless.  The format is stated in include/csic.h; csic_rice_host.cpp is the host codec and owns the geometry.
//
// Mapping, as csic_pack.hip: one lane per GROUP of 32 samples, Q a template parameter, 256-thread blocks of 256 consecutive groups of one
// plane -- a block of the kernels is a block of the format, it owns one chunk of the payload and one directory entry; planes of different
// widths go out as separate launches.  What the two units have in common is csic_pack_common.h's: the argument, the accessors, the block
// scan, the group load, the store of a block's nibble and anchors sections, the nibble and anchor reads, the repacking and store of a
// decoded group, and on the launch side the argument's filler, the refusals, the workspace size and the per-width launches.  This unit
// adds the modes, the chunks and the directory.
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

#include "csic_pack_common.h"

namespace csic {

struct RcArgs : PkArgs {           // woff: the modes sections; payload_offset, bound_bytes: the Rice coding's
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
    const PkArgs &e = a;
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
    pk_store_sections<Q>(e, cb, plane, G, g0, s_m, s_a);
}

template <int Q, bool NT>
__global__ void __launch_bounds__(PK_T) k_rice_emit(RcArgs a)
{
    __shared__ uint32_t s_chunk[RcCap<Q>::DW], s_tot[PK_WAVES];
    const PkArgs &e = a;
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
    const PkArgs &e = a;
    const int plane = e.plane0 + (int)blockIdx.y;
    const uint32_t G = e.groups[plane], g0 = blockIdx.x * PK_T, t = threadIdx.x, g = g0 + t;
    if (g0 >= G) return;
    const gpdst_t cb = pk_coded_frame(e);
    const uint32_t blk = e.block0[plane] + blockIdx.x;
    // the mode as the device takes it: 15 is zero mode, anything else k = min(m, Q)
    const uint32_t m = g < G ? pk_nibble(e, cb, plane, g) : 15u;
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
    uint32_t c = pk_anchor<Q>(e, cb, plane, g);
    // where the group's bits start: R by the scan, U behind terminator 31 z
    uint32_t rbit = before >> 16, ubit = 32u * rdw;
    if (unary) ubit += rice_after_terminator(s_chunk + rdw, s_cum, uw, 31u * (before & 0xFFFFu));
    const uint32_t n = e.n[plane], uend = 32u * nw;
    PkGroupOut<Q> out;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j > 0 && !zero) c = (c + rice_unfold(rice_next_u(s_chunk, nw, &rbit, &ubit, uend, k, (uint32_t)Q), MASK)) & MASK;
        out.put(j, 32u * g + (uint32_t)j < n ? c : 0u);                     // slots behind the last sample: zero bits
    }
    out.template store<NT>(e, pk_bits_frame(e), plane, g);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int fill_rc_args(const csic_plan *pl, RcArgs *a)
{
    RiceGeometry G;
    int st = rice_geometry(&pl->p, &G);
    if (st != CSIC_OK) return st;
    const csic_rice_layout &L = G.layout;
    st = pk_fill_args(pl, G.pk, L.modes_offset, L.anchors_offset, L.payload_offset, L.bound_bytes, "csic_rice_pack_device", a);
    a->dir_off = (uint32_t)L.directory_offset;
    a->max_dwords = (uint32_t)((L.bound_bytes - L.payload_offset) / 4);
    return st;
}

static const auto rice_modes = [](auto q, auto nt) { return k_rice_modes<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto rice_emit = [](auto q, auto nt) { return k_rice_emit<CSIC_CONST(q), CSIC_CONST(nt)>; };
static const auto rice_unpack = [](auto q, auto nt) { return k_rice_unpack<CSIC_CONST(q), CSIC_CONST(nt)>; };

} // namespace csic

using namespace csic;

extern "C" {

const char *csic_rice_kernel_name(const csic_plan *plan) { return pk_kernel_name("k_rice", plan); }

int csic_rice_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes) { return pk_workspace_bytes(plan, nframes, bytes, fill_rc_args); }

int csic_rice_pack_device(csic_plan *plan, const void *d_bits, int32_t nframes, void *d_coded, uint64_t *d_sizes, void *d_workspace,
                          size_t workspace_bytes, void *hip_stream)
{
    if (plan && !d_sizes) return set_error(CSIC_EINVAL_NULL, "d_sizes is NULL");
    RcArgs a;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, true, d_workspace, workspace_bytes, fill_rc_args, &a);
    if (st != CSIC_OK) return st;
    if ((uintptr_t)d_sizes & 7u) return set_error(CSIC_EINVAL_SIZE, "d_sizes must be 8-byte aligned");
    a.sizes = reinterpret_cast<unsigned long long *>(d_sizes);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = pk_launch_planes(plan, a, nframes, stream, rice_modes)) != CSIC_OK) return st;
    if ((st = pack_scan_launch(a, nframes, stream)) != CSIC_OK) return st;
    if ((st = pk_launch_planes(plan, a, nframes, stream, rice_emit)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_rice_unpack_device(csic_plan *plan, const void *d_coded, int32_t nframes, void *d_bits, void *hip_stream)
{
    RcArgs a;
    int st = pk_prepare(plan, d_bits, d_coded, nframes, false, nullptr, 0, fill_rc_args, &a);
    if (st != CSIC_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    CSIC_DEVICE_SCOPE(plan->device);
    if ((st = pk_launch_planes(plan, a, nframes, stream, rice_unpack)) != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
