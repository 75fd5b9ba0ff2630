// csic_planar_bits.hip -- out_format = CSIC_FMT_PLANAR_BITS: the planar frame of csic_planar.hip with every sample stored at its
// quantised bit width (LSB-first bit planes; layout and definition in include/csic.h, csic_planar_bits_layout), and
// csic_reconstruct_bits_device, its inverse.  A 6/5/5 frame of 4:2:0 at factor 1 is 1.06 bytes per pixel instead of PLANAR's 1.5.
//
// Kernels (wave64; HBM-bound byte work, no LDS arrays, no MFMA):
//   k_pbits_f1<ROUND, NT>       HOLD_DECIMATE, factor 1, module_width % 128 == 0.  k_planar_flat MODE 2's streaming: one-wave blocks,
//                      K = 4 groups of 4 consecutive pixels per lane spaced by the block size, one 16-byte load per group.  Each lane
//                      turns its group into a chunk of 4 codes per plane (ns = 4 >> log2 hold_h codes for Cb / Cr), and the G lanes
//                      that hold 32 consecutive SAMPLES of a plane (G = 8 for Y, 8 << log2 hold_h for chroma) assemble the plane's q
//                      output dwords: logical lane D of the group collects, with ds_bpermute, the chunks that overlap bits
//                      [32 D, 32 D + 32) and stores that dword (lanes D >= q store nothing).  q is a wave-uniform run-time value.
//   k_pbits_strided<ROUND, NT>  HOLD_DECIMATE, chroma before spatial with a factor >= 2, module_width % 128 == 0.  k_planar_strided's
//                      mapping (4 positions per lane spaced by the block size, rows r % f != 0 never read) and its quad byte transpose,
//                      after which a lane holds 4 consecutive positions and the same assembly runs over the lanes of one round.
//   k_pbits_gen<ROUND, AVG>     anything: one lane per group of 8 samples of the Y plane, or of both chroma planes, each sample by its
//                      definition (the input pixel of its stream position; AVG: the box / pool averages of avg_pixel_generic); the
//                      lane writes the q bytes of its group.  CSIC_TUNE_VARIANT 9 forces it.
//   k_rbits<FMT, FAST, NT>      bits -> packed ARGB / YCbCr, k_recon's replay rule; K = 4 groups of 4 positions per lane, per group the
//                      two dwords that hold its codes in each plane, one 16-byte store.  FAST needs module_width % 4 == 0.  The body
//                      is k_recon's -- recon_body of csic_plane_read.h -- over BitPlanes, the bit planes' source.
// Every output byte is written by exactly one lane (no read-modify-write, no atomics); the fast kernels store dwords only (their
// planes are whole dwords: n and every chroma row are multiples of 32 samples).  Every global access goes through the accessors of
// csic_kernel_ops.h, which the CSIC_DEBUG build range-checks: the input against the extent of KArgs, the bit planes against the
// frame's frame_bytes (bst1 / bst4 name that limit), k_rbits' output stores against the frame's n pixels.  Which forward kernel a
// call takes, its name, threads and blocks are plan_planar_bits of csic_select.cpp (host only).
#include <cstdio>
#include <cstring>

#include "csic_kernel_ops.h"
#include "csic_plane_read.h"

namespace csic {

// the second kernel argument of the kernels below
struct BExtra {
    uint8_t *bits;              // bit-packed frame buffers, frame_bytes apart
    uint32_t *packed;           // reconstruct: destination (n pixels per frame, back to back)
    int64_t off[3];             // plane offsets: Y, Cb, Cr
    int64_t nbytes[3];          // bytes each plane's samples occupy (B(s, q))
    int64_t frame_bytes, n, ns; // frame buffer size; positions; chroma samples
    int32_t q[3];               // bits per sample: y_bits, cb_bits, cr_bits
    int32_t Wm, Wc, lhe, lve, hold_v, replay_last;
    uint32_t mWm, kWm;          // exact j / Wm (magic_div)
    int32_t T;                  // threads per block
    int64_t ngy, ngc;           // general kernel: groups of 8 samples of Y / of the chroma planes
};

// the bit-packed frame's accessors: byte offsets into the frame_bytes of the frame
template <bool NT> __device__ __forceinline__ void bst1(const BExtra &e, gbyte_t fb, int64_t off, uint32_t v) { by_st1<NT>(e.frame_bytes, fb, off, v); }
template <bool NT> __device__ __forceinline__ void bst4(const BExtra &e, gbyte_t fb, int64_t off, uint32_t v) { by_st4<NT>(e.frame_bytes, fb, off, v); }
__device__ __forceinline__ gbyte_t bits_frame(const BExtra &e) { return frame_at_z(e.bits, e.frame_bytes); }

// ------------------------------------------------------------------------------------------------
// fast forward, HOLD_DECIMATE: chunks and their assembly into output dwords
// ------------------------------------------------------------------------------------------------
// codes of byte values: 4 (b0..b3), 2 (b0, b2) or 1 (b0) of them, LSB first, q bits each
__device__ __forceinline__ uint32_t chunk_of(uint32_t b4, uint32_t q, int lhe)
{
    const uint32_t s = 8u - q;
    const uint32_t c0 = (b4 & 0xFFu) >> s, c2 = ((b4 >> 16) & 0xFFu) >> s;
    if (lhe == 2) return c0;
    if (lhe == 1) return c0 | (c2 << q);
    const uint32_t c1 = ((b4 >> 8) & 0xFFu) >> s, c3 = (b4 >> 24) >> s;
    return c0 | (c1 << q) | (c2 << (2u * q)) | (c3 << (3u * q));
}

// One plane's view of a lane: the G lanes of a packing group hold 32 consecutive samples, chunk of w = ns * q bits each; the lane of
// logical index D in its group produces output dword D (D < q), from chunks first .. first + cnt - 1 of the group.  cnt depends on
// w and G only: the loop below is wave-uniform, so every lane takes part in every ds_bpermute.
struct Asm {
    uint32_t D, lane_g0, lstep, first, w, G;
    int cnt;
};
__device__ __forceinline__ Asm make_asm(uint32_t u, uint32_t G, uint32_t w, uint32_t lane0, uint32_t lstep)
{
    Asm m;
    m.D = u & (G - 1u);
    m.lane_g0 = lane0 + lstep * (u - m.D);          // physical lane (within the wave) of the group's logical lane 0
    m.lstep = lstep;
    m.first = (32u * m.D) / w;
    m.w = w;
    m.G = G;
    m.cnt = (int)min(G, 31u / w + 2u);
    return m;
}
__device__ __forceinline__ uint32_t assemble(const Asm &m, uint32_t chunk)
{
    uint32_t out = 0;
    for (int t = 0; t < m.cnt; ++t) {
        const uint32_t src = m.first + (uint32_t)t;
        const uint32_t v = (uint32_t)__shfl((int)chunk, (int)(m.lane_g0 + m.lstep * min(src, m.G - 1u)), 64);
        const int s = (int)(src * m.w) - (int)(32u * m.D);     // bit offset of chunk src relative to the dword; > -32 by choice of first
        const uint32_t c = s >= 0 ? (s < 32 ? v << s : 0u) : v >> (-s);
        out |= src < m.G ? c : 0u;
    }
    return out;
}

struct PlaneAsm {
    Asm a[3];                   // Y, Cb, Cr
};
__device__ __forceinline__ PlaneAsm make_plane_asm(const BExtra &e, uint32_t u, uint32_t lane0, uint32_t lstep)
{
    PlaneAsm p;
    const uint32_t ns = 4u >> e.lhe, Gc = 8u << e.lhe;
    p.a[0] = make_asm(u, 8u, 4u * (uint32_t)e.q[0], lane0, lstep);
    p.a[1] = make_asm(u, Gc, ns * (uint32_t)e.q[1], lane0, lstep);
    p.a[2] = make_asm(u, Gc, ns * (uint32_t)e.q[2], lane0, lstep);
    return p;
}

// one group of 4 consecutive positions j0 .. j0 + 3 (one chroma row; y4 / cb4 / cr4: their unquantised values, byte i = position
// j0 + i): assemble and store.  live: the group lies in the stream (a whole packing group is live or dead together).
template <bool NT>
__device__ __forceinline__ void pbits_emit(const BExtra &e, const PlaneAsm &pa, gbyte_t fb, uint32_t j0, bool live,
                                           uint32_t y4, uint32_t cb4, uint32_t cr4)
{
    const uint32_t qy = (uint32_t)e.q[0], qb = (uint32_t)e.q[1], qr = (uint32_t)e.q[2];
    const uint32_t dy = assemble(pa.a[0], chunk_of(y4, qy, 0));
    const uint32_t db = assemble(pa.a[1], chunk_of(cb4, qb, e.lhe));
    const uint32_t dr = assemble(pa.a[2], chunk_of(cr4, qr, e.lhe));
    if (!live) return;
    // Y: the group's first position is j0 - 4 D (a multiple of 32): its q dwords start at byte (first / 32) * 4 q
    if (pa.a[0].D < qy) bst4<NT>(e, fb, e.off[0] + (int64_t)((j0 - 4u * pa.a[0].D) >> 5) * (4 * qy) + 4 * pa.a[0].D, dy);
    const uint32_t r = (uint32_t)(((uint64_t)j0 * e.mWm) >> e.kWm), c0 = j0 - r * (uint32_t)e.Wm;
    if ((r & ((1u << e.lve) - 1u)) != 0) return;                         // a row without sample points
    const int64_t k0 = (int64_t)(r >> e.lve) * e.Wc + (c0 >> e.lhe);    // this lane's first sample
    const int64_t kg = (k0 - (int64_t)(pa.a[1].D * (4u >> e.lhe))) >> 5;     // its packing group (32 samples)
    if (pa.a[1].D < qb) bst4<NT>(e, fb, e.off[1] + kg * (4 * qb) + 4 * pa.a[1].D, db);
    if (pa.a[2].D < qr) bst4<NT>(e, fb, e.off[2] + kg * (4 * qr) + 4 * pa.a[2].D, dr);
}

template <int ROUND, bool NT, bool CHECK>
__device__ __forceinline__ void pbits_f1_body(const KArgs &a, const BExtra &e, gin_t in, gbyte_t fb, const PlaneAsm &pa, uint32_t g0,
                                              uint32_t T, uint32_t ngroups)
{
    u32x4 v[PBITS_K];
#pragma unroll
    for (int k = 0; k < PBITS_K; ++k) {
        const uint32_t g = g0 + (uint32_t)k * T;
        const uint32_t gc = CHECK ? min(g, ngroups - 1u) : g;            // clamp: every lane stays in the exchange
        v[k] = in4<NT>(a, in, stream_in_off(a, 4u * gc));
    }
#pragma unroll
    for (int k = 0; k < PBITS_K; ++k) {
        const uint32_t g = g0 + (uint32_t)k * T;
        const uint32_t px[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        uint32_t y4 = 0, cb4 = 0, cr4 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t cb, cr;
            fwd_c<ROUND>(px[i], cb, cr);
            y4 |= fwd_y(px[i]) << (8 * i);
            cb4 |= cb << (8 * i);
            cr4 |= cr << (8 * i);
        }
        pbits_emit<NT>(e, pa, fb, 4u * g, !CHECK || g < ngroups, y4, cb4, cr4);
    }
    if (!CHECK) keep_tail_apart();
}

template <int ROUND, bool NT>
__global__ void __launch_bounds__(256) k_pbits_f1(KArgs a, BExtra e)
{
    pin_args(a);
    const uint32_t T = (uint32_t)e.T;
    const uint32_t ngroups = (uint32_t)(e.n >> 2);
    const uint32_t b0 = blockIdx.x * (T * PBITS_K);
    const gin_t in = frame_in(a);
    const gbyte_t fb = bits_frame(e);
    // a wave's lanes hold 64 consecutive groups (256 positions, 256-aligned) in every round
    const PlaneAsm pa = make_plane_asm(e, threadIdx.x & 63u, 0u, 1u);
    if (b0 + T * PBITS_K <= ngroups) pbits_f1_body<ROUND, NT, false>(a, e, in, fb, pa, b0 + threadIdx.x, T, ngroups);
    else                             pbits_f1_body<ROUND, NT, true>(a, e, in, fb, pa, b0 + threadIdx.x, T, ngroups);
}

// quad transpose of bytes (csic_planar.hip: k_planar_strided): lane q of a quad collects byte q of its four lanes
__device__ __forceinline__ uint32_t pbits_quad_transpose(uint32_t w, uint32_t sel_lo, uint32_t sel_hi)
{
    const uint32_t a0 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0x00 /* quad_perm:[0,0,0,0] */, 0xF, 0xF, false);
    const uint32_t a1 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0x55 /* quad_perm:[1,1,1,1] */, 0xF, 0xF, false);
    const uint32_t a2 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0xAA /* quad_perm:[2,2,2,2] */, 0xF, 0xF, false);
    const uint32_t a3 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0xFF /* quad_perm:[3,3,3,3] */, 0xF, 0xF, false);
    return __builtin_amdgcn_perm(a1, a0, sel_lo) | __builtin_amdgcn_perm(a3, a2, sel_hi);
}

template <int ROUND, bool NT, bool CHECK>
__device__ __forceinline__ void pbits_strided_body(const KArgs &a, const BExtra &e, gin_t in, gbyte_t fb, const PlaneAsm &pa,
                                                   uint32_t b0, uint32_t T)
{
    const uint32_t n = (uint32_t)e.n;
    const uint32_t tid = threadIdx.x, q = tid & 3u;
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t j = b0 + (uint32_t)k * T + tid;
        px[k] = in1<NT>(a, in, stream_in_off(a, CHECK ? min(j, n - 1u) : j));
    }
    uint32_t wy = 0, wb = 0, wr = 0;                                      // byte k = position b0 + k * T + tid
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t cb, cr;
        fwd_c<ROUND>(px[k], cb, cr);
        wy |= fwd_y(px[k]) << (8 * k);
        wb |= cb << (8 * k);
        wr |= cr << (8 * k);
    }
    const uint32_t sel_lo = 0x0c0c0000u | q | ((4u + q) << 8), sel_hi = 0x00000c0cu | (q << 16) | ((4u + q) << 24);
    const uint32_t y4 = pbits_quad_transpose(wy, sel_lo, sel_hi);
    const uint32_t cb4 = pbits_quad_transpose(wb, sel_lo, sel_hi);
    const uint32_t cr4 = pbits_quad_transpose(wr, sel_lo, sel_hi);
    // this lane now holds positions j0 .. j0 + 3, the group its quad loaded in round q; lanes q, q + 4, ... of a wave hold the
    // wave's 16 consecutive groups of that round
    const uint32_t j0 = b0 + q * T + (tid & ~3u);
    pbits_emit<NT>(e, pa, fb, j0, !CHECK || j0 < n, y4, cb4, cr4);
    if (!CHECK) keep_tail_apart();
}

template <int ROUND, bool NT>
__global__ void __launch_bounds__(256) k_pbits_strided(KArgs a, BExtra e)
{
    pin_args(a);
    const uint32_t T = (uint32_t)e.T;                 // a multiple of 64
    const uint32_t b0 = blockIdx.x * (T * 4u);
    const gin_t in = frame_in(a);
    const gbyte_t fb = bits_frame(e);
    const PlaneAsm pa = make_plane_asm(e, (threadIdx.x & 63u) >> 2, threadIdx.x & 3u, 4u);
    if ((uint64_t)b0 + (uint64_t)T * 4u <= (uint64_t)e.n) pbits_strided_body<ROUND, NT, false>(a, e, in, fb, pa, b0, T);
    else                                                   pbits_strided_body<ROUND, NT, true>(a, e, in, fb, pa, b0, T);
}

// ------------------------------------------------------------------------------------------------
// general forward: one lane per group of 8 samples, every sample by its definition
// ------------------------------------------------------------------------------------------------
// AVG: the quantised f x f average of Y at output (ro, co) -- avg_pixel_generic's Y half
template <int ROUND>
__device__ __forceinline__ uint32_t avg_y_generic(const KArgs &a, gin_t in, int ro, int co)
{
    const int f = a.f;
    uint32_t sy = 0;
    for (int i = 0; i < f; ++i)
        for (int j = 0; j < f; ++j) {
            const int r = min(ro * f + i, a.H - 1), c = min(co * f + j, a.W - 1);
            sy += fwd_y(in1<false>(a, in, (int64_t)r * a.ip + c));
        }
    return ((sy + ((f * f) >> 1)) >> (2 * a.sc_shift)) & a.my;
}

// the q bytes of one group of 8 codes (fewer at the plane's tail: the plane ends at byte nbytes)
__device__ __forceinline__ void store_group(const BExtra &e, gbyte_t fb, int64_t off, int64_t g, uint32_t q, int64_t nbytes, uint64_t acc)
{
    const int64_t b0 = g * q;
    const int nb = (int)min((int64_t)q, nbytes - b0);
    for (int b = 0; b < nb; ++b) bst1<false>(e, fb, off + b0 + b, (uint32_t)(acc >> (8 * b)) & 0xFFu);
}

template <int ROUND, bool AVG>
__global__ void __launch_bounds__(256) k_pbits_gen(KArgs a, BExtra e)
{
    pin_args(a);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= e.ngy + e.ngc) return;
    const gin_t in = frame_in(a);
    const gbyte_t fb = bits_frame(e);
    if (t < e.ngy) {                                                      // Y: positions 8 t .. 8 t + 7
        const uint32_t q = (uint32_t)e.q[0];
        uint64_t acc = 0;
        for (int i = 0; i < 8; ++i) {
            const int64_t j = 8 * t + i;
            if (j >= e.n) break;
            uint32_t y;
            if (AVG) y = avg_y_generic<ROUND>(a, in, (int)(j / a.Wo), (int)(j % a.Wo));
            else     y = fwd_y(in1<false>(a, in, stream_in_off(a, (uint32_t)j)));
            acc |= (uint64_t)(y >> (8 - q)) << (i * q);
        }
        store_group(e, fb, e.off[0], t, q, e.nbytes[0], acc);
        return;
    }
    const int64_t g = t - e.ngy;                                          // Cb and Cr: samples 8 g .. 8 g + 7
    const uint32_t qb = (uint32_t)e.q[1], qr = (uint32_t)e.q[2];
    uint64_t ab = 0, ar = 0;
    for (int i = 0; i < 8; ++i) {
        const int64_t k = 8 * g + i;
        if (k >= e.ns) break;
        // the sample point of index k: chroma row k / Wc, column k % Wc -> stream row * hold_v, column * hold_h
        const int64_t crow = k / e.Wc, ccol = k - crow * e.Wc;
        const int64_t r = crow * e.hold_v, c = ccol << e.lhe;
        uint32_t cb, cr;
        if (AVG) {                                                        // module_width == Wo under AVG
            const uint32_t ycc = avg_pixel_generic<ROUND, F_YCC, F_ARGB>(a, in, (int)r, (int)c);
            cb = (ycc >> 8) & 0xFFu; cr = (ycc >> 16) & 0xFFu;
        } else {
            fwd_c<ROUND>(in1<false>(a, in, stream_in_off(a, (uint32_t)(r * e.Wm + c))), cb, cr);
        }
        ab |= (uint64_t)(cb >> (8 - qb)) << (i * qb);
        ar |= (uint64_t)(cr >> (8 - qr)) << (i * qr);
    }
    store_group(e, fb, e.off[1], g, qb, e.nbytes[1], ab);
    store_group(e, fb, e.off[2], g, qr, e.nbytes[2], ar);
}

// ------------------------------------------------------------------------------------------------
// reconstruct: bits -> packed
// ------------------------------------------------------------------------------------------------
using RbitsPlanes = BitPlanes<BExtra, &BExtra::frame_bytes>;

template <int FMT, bool FAST, bool NT>
__global__ void __launch_bounds__(256) k_rbits(KArgs a, BExtra e)
{
    pin_args(a);
    (void)a;
    const uint32_t T = (uint32_t)e.T;
    const uint32_t ngroups = (uint32_t)((e.n + 3) >> 2);
    const uint32_t b0 = blockIdx.x * (T * RBITS_K);
    const gcbyte_t fb = (gcbyte_t)bits_frame(e);
    const gout_t out = (gout_t)(uintptr_t)e.packed + (int64_t)blockIdx.z * e.n;
    if (b0 + T * RBITS_K <= ngroups && (uint64_t)4 * (b0 + T * RBITS_K) <= (uint64_t)e.n)
        recon_body<FMT, FAST, NT, false, RBITS_K, RbitsPlanes>(e, fb, out, b0 + threadIdx.x, T, ngroups);
    else
        recon_body<FMT, FAST, NT, true, RBITS_K, RbitsPlanes>(e, fb, out, b0 + threadIdx.x, T, ngroups);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using BitsFn = void (*)(KArgs, BExtra);

static void fill_bits_extra(const csic_planar_bits_layout &L, BExtra *e)
{
    std::memset(e, 0, sizeof *e);
    const csic_planar_layout &G = L.geometry;
    e->off[0] = L.y_offset; e->off[1] = L.cb_offset; e->off[2] = L.cr_offset;
    e->nbytes[0] = L.y_bytes; e->nbytes[1] = L.cb_bytes; e->nbytes[2] = L.cr_bytes;
    e->frame_bytes = L.frame_bytes;
    e->n = (int64_t)G.y_width * G.y_height;
    e->ns = G.chroma_samples;
    e->q[0] = L.y_bits; e->q[1] = L.cb_bits; e->q[2] = L.cr_bits;
    e->Wm = G.module_width; e->Wc = G.chroma_width; e->lhe = ilog2(G.hold_h); e->lve = ilog2(G.hold_v); e->hold_v = G.hold_v;
    e->replay_last = G.replay_last;
    magic_div((uint32_t)G.module_width, &e->mWm, &e->kWm);
    e->ngy = (e->n + 7) / 8;
    e->ngc = (e->ns + 7) / 8;
}

int planar_bits_forward(const csic_plan *pl, const void *d_in, void *d_bits, int nframes, hipStream_t stream)
{
    if (!d_in || !d_bits) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    const csic_params &p = pl->p;
    const Geometry &g = pl->g;
    csic_planar_bits_layout L;
    planar_bits_layout(g, &p, &L);
    if ((uintptr_t)d_bits & 255u) return set_error(CSIC_EINVAL_SIZE, "a bit-packed planar frame buffer must be 256-byte aligned");
    if ((uintptr_t)d_in & 3u) return set_error(CSIC_EINVAL_SIZE, "the input must be 4-byte aligned");
    BitsPlan bp;                                                        // kind, threads and blocks: csic_select.cpp
    const int st = plan_planar_bits(p, g, pl->tune, (uintptr_t)d_in, nframes, &bp);
    if (st != CSIC_OK) return st;
    const bool nt = !pl->tune.no_nt;
    const bool avg = p.sampling == CSIC_SAMPLING_AVG;
    const BitsFn fn = with_const<R_FLOOR, R_TRUNC>(p.rounding, [&](auto round) {
        return with_const<true, false>(bp.kind == PBITS_GEN ? avg : nt, [&](auto b) -> BitsFn {      // b: k_pbits_gen's AVG, the others' NT
            if (bp.kind == PBITS_F1) return k_pbits_f1<CSIC_CONST(round), CSIC_CONST(b)>;
            if (bp.kind == PBITS_STRIDED) return k_pbits_strided<CSIC_CONST(round), CSIC_CONST(b)>;
            return k_pbits_gen<CSIC_CONST(round), CSIC_CONST(b)>;
        });
    });
    return for_frame_batches(nframes, [&](int f0, int nz) {
        KArgs a;
        fill_base_args(g, g.W, g.Wo, &a);
        BExtra e;
        fill_bits_extra(L, &e);
        a.in = static_cast<const uint32_t *>(d_in) + (int64_t)f0 * a.in_frame_px;
        e.bits = static_cast<uint8_t *>(d_bits) + (int64_t)f0 * L.frame_bytes;
        e.T = bp.T;
        a.bdx = bp.bdx; a.bdy = bp.bdy; a.row_step = bp.row_step;
        return launch(fn, dim3(bp.grid.x, 1, (unsigned)nz), dim3(bp.block.x, 1, 1), stream, a, e);
    });
}

} // namespace csic

using namespace csic;

extern "C" int csic_reconstruct_bits_device(csic_plan *plan, const void *d_bits, void *d_out, int32_t nframes, int32_t out_format,
                                            void *hip_stream)
{
    return reconstruct_device(plan, d_bits, &BExtra::bits, d_out, nframes, out_format, hip_stream, "csic_reconstruct_bits_device",
                              "a bit-packed planar frame buffer must be 256-byte aligned and the packed output 16-byte aligned", RBITS_K,
                              [](const csic_plan *pl, BExtra *e) { csic_planar_bits_layout L; planar_bits_layout(pl->g, &pl->p, &L); fill_bits_extra(L, e); },
                              [](auto fmt, auto fast, auto nt) -> BitsFn { return k_rbits<CSIC_CONST(fmt), CSIC_CONST(fast), CSIC_CONST(nt)>; });
}
