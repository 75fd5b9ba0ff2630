// csic_planar.hip -- out_format = CSIC_FMT_PLANAR: the same pixel pipeline with a genuinely subsampled result (one Y byte
// per output pixel, one Cb and one Cr byte per chroma SAMPLE POINT), and csic_reconstruct_device, its inverse.  The layout
// and the reconstruct rule are defined in include/csic.h (csic_planar_layout); SURVEY.md 8 f3, VERDICT r03 item 4.
//
// Why it is reference-derivable although the reference never builds the format (ChromaSubsampler.scala:57-65 re-emits the held
// chroma with every pixel; README.md:35-46 only describes the subsampled wire format): the packed YCbCr stream the reference
// does produce is, by App. A.3, a pure function of Y at every position and Cb / Cr at the sample points -- the planar frame
// stores exactly those, and reconstruct replays the hold (the in-row hold and the 4:x:0 "odd rows replay the last sample of
// the row above" quirk), so  reconstruct(planar(x)) == packed(x)  bit for bit (tests/test_gpu_planar.py, against the oracle).
//
// Kernels (wave64; HBM-bound byte work, no LDS, no MFMA):
//   k_planar_flat<ROUND, MODE, NT>  HOLD_DECIMATE.  Lanes over groups of 4 consecutive positions of the OUTPUT stream, K = 4
//                      groups per lane spaced by the block size: 4 Y bytes leave as one 4-byte store.
//                        MODE 2  factor 1, W % 4 == 0 (the stream IS the image): one 16-byte load per group; Cb / Cr of a group
//                                leave as one 4-, 2- or 1-byte store (h = 1, 2, 4); rows without sample points (4:x:0 odd rows)
//                                compute Y only.  One-wave blocks: a wave's four loads cover 4 KiB of consecutive pixels.
//                        MODE 0  anything whose groups may straddle chroma rows (module_width % 4 != 0: spatial before chroma
//                                with ragged widths): 4-byte loads, per-position chroma byte stores.
//                        MODE 1  (CSIC_TUNE_VARIANT 10 only) the first form of k_planar_strided's job, kept for A/B.
//   k_planar_strided<ROUND, NT>  HOLD_DECIMATE with a factor >= 2 (module_width % 4 == 0): k_decflat's mapping -- 4 positions per
//                      lane spaced by the block size, loads at stride f (rows r % f != 0 are never read) -- and a 4 x 4 byte
//                      transpose inside each quad of lanes (DPP + v_perm), after which a lane owns 4 consecutive positions and
//                      stores Y, Cb, Cr as dwords.
//   k_planar_avg_f1<ROUND, HE, VE, NT>  AVG extension, factor 1, whole 4 x VE tiles: a lane owns a 4-pixel x VE-row tile
//                      (VE 16-byte loads), so every h x v chroma block lies in its registers: true 4:2:2 / 4:2:0 / 4:1:1
//                      box-filtered chroma -- what the north star's prose describes -- at 1.5-3 bytes per pixel out.
//   k_planar_avg_gen<ROUND>  AVG, anything else: one output position per lane by the definition (avg_pixel_generic).
//   k_recon<FMT, FAST, NT>  planar -> packed: K = 4 groups of 4 positions per lane; per group one 4-byte Y load and the aligned
//                      dword that holds the group's chroma samples (branch-free: shifted into place), one 16-byte store;
//                      FAST needs module_width % 4 == 0, otherwise position by position.  The body is recon_body of
//                      csic_plane_read.h (shared with k_rbits) over BytePlanes, this format's plane source.
// Measured on 8192x8192 (profiles/r04_bench_all_configs.jsonl, r04_planar_bt.log): 4:2:0 at factor 1 -- 5.5 algorithmic bytes per pixel
// instead of 8 -- k_planar_flat 77 % of the 8 TB/s roofline (59.8 us per frame against 87.3 us for the packed k_f1x4),
// k_planar_avg_f1 77 %; factor 2 (3 bytes per output pixel) k_planar_strided 72-74 % (the 4-consecutive form: 45 %);
// k_recon 67-72 %.
// Algorithmic bytes: input as for the packed path (4 * W * ceil(H / f), AVG: 4 * W * H) + csic_planar_layout.payload_bytes;
// reconstruct: payload_bytes + 4 * n.
// Every global access goes through the accessors of csic_kernel_ops.h, which the CSIC_DEBUG build range-checks: the input against
// the extent of KArgs, the planes against the frame's frame_bytes (pst1 / pst2 / pst4 name that limit), k_recon's output stores
// -- the 16-byte ones of both paths and the tail's single pixels -- against the frame's n pixels.  Which kernel a plan takes, its
// name, grid and block are plan_planar / plan_reconstruct of csic_select.cpp (host only); batches of 65535 frames, the launch and
// csic_reconstruct_device's body are the shell of csic_hip_common.h.
#include <cstdio>
#include <cstring>

#include "csic_kernel_ops.h"
#include "csic_plane_read.h"
#include "csic_avg_tile.h"

namespace csic {

// the planar frame's accessors: byte offsets into the frame_bytes of the frame
template <bool NT> __device__ __forceinline__ void pst1(const PExtra &e, gbyte_t fb, int64_t off, uint32_t v) { by_st1<NT>(e.frame_bytes, fb, off, v); }
template <bool NT> __device__ __forceinline__ void pst2(const PExtra &e, gbyte_t fb, int64_t off, uint32_t v) { by_st2<NT>(e.frame_bytes, fb, off, v); }
template <bool NT> __device__ __forceinline__ void pst4(const PExtra &e, gbyte_t fb, int64_t off, uint32_t v) { by_st4<NT>(e.frame_bytes, fb, off, v); }

// base of the planar frame this block works on (grid z = frame): consecutive buffers, or -- frame-table mode -- whatever the
// device-resident table names (read through the constant address space: one wave-uniform s_load, as frame_in / frame_out)
__device__ __forceinline__ gbyte_t planar_frame(const PExtra &e)
{
    if (e.planar_tab) return (gbyte_t)((const uint64_t CSIC_CONSTANT *)(uintptr_t)e.planar_tab)[blockIdx.z];
    return (gbyte_t)(uintptr_t)e.planar + (int64_t)blockIdx.z * e.frame_bytes;
}

// ------------------------------------------------------------------------------------------------
// forward, HOLD_DECIMATE
// ------------------------------------------------------------------------------------------------
// one position on its own (the stream's ragged tail, and every position of MODE 0)
template <int ROUND, bool NT>
__device__ __forceinline__ void planar_one(const KArgs &a, const PExtra &e, gin_t in, gbyte_t fb, uint32_t j, uint32_t px, bool store_y)
{
    if (store_y) pst1<NT>(e, fb, (int64_t)j, fwd_y(px) & a.my);
    const uint32_t r = (uint32_t)(((uint64_t)j * e.mWm) >> e.kWm), c = j - r * (uint32_t)e.Wm;
    if ((c & ((1u << e.lhe) - 1u)) == 0 && (r & ((1u << e.lve) - 1u)) == 0) {          // a sample point emits its OWN chroma
        uint32_t cb, cr;
        fwd_c<ROUND>(px, cb, cr);
        const int64_t k = (int64_t)(r >> e.lve) * e.Wc + (c >> e.lhe);
        pst1<NT>(e, fb, e.cb_off + k, cb & a.mcb);
        pst1<NT>(e, fb, e.cr_off + k, cr & a.mcr);
    }
    (void)in;
}

template <int ROUND, int MODE, int K, bool NT, bool CHECK>
__device__ __forceinline__ void planar_flat_body(const KArgs &a, const PExtra &e, gin_t in, gbyte_t fb, uint32_t g0, uint32_t T, uint32_t ngroups)
{
    const uint32_t n = (uint32_t)e.n;
    uint32_t px[K][4];
    bool live[K], full[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t g = g0 + (uint32_t)k * T;
        live[k] = !CHECK || g < ngroups;
        const uint32_t gc = CHECK ? min(g, ngroups - 1) : g;                 // clamp instead of branching: the loads still issue back to back
        const uint32_t j0 = 4u * gc;
        full[k] = !CHECK || j0 + 3u < n;
        if (MODE == 2) {
            // factor 1, W % 4 == 0: the group is 4 consecutive pixels of one row (the stream IS the image)
            const u32x4 v = in4<NT>(a, in, stream_in_off(a, j0));
            px[k][0] = v.x; px[k][1] = v.y; px[k][2] = v.z; px[k][3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) px[k][q] = in1<NT>(a, in, stream_in_off(a, min(j0 + (uint32_t)q, n - 1u)));
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!live[k]) continue;
        const uint32_t j0 = 4u * (g0 + (uint32_t)k * T);
        if (CHECK && !full[k]) {                                             // the stream's ragged tail: position by position
            for (uint32_t q = 0; q < 4u && j0 + q < n; ++q) planar_one<ROUND, NT>(a, e, in, fb, j0 + q, px[k][q], true);
            continue;
        }
        const uint32_t y4 = (fwd_y(px[k][0]) & a.my) | ((fwd_y(px[k][1]) & a.my) << 8) | ((fwd_y(px[k][2]) & a.my) << 16) |
                            ((fwd_y(px[k][3]) & a.my) << 24);
        pst4<NT>(e, fb, (int64_t)j0, y4);
        if (MODE == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) planar_one<ROUND, NT>(a, e, in, fb, j0 + (uint32_t)q, px[k][q], false);
        } else {
            // module_width % 4 == 0: the group sits in ONE chroma row at a column that is a multiple of 4
            const uint32_t r = (uint32_t)(((uint64_t)j0 * e.mWm) >> e.kWm), c0 = j0 - r * (uint32_t)e.Wm;
            if ((r & ((1u << e.lve) - 1u)) != 0) continue;                   // no sample point in this row (wave-uniform almost everywhere)
            const int64_t k0 = (int64_t)(r >> e.lve) * e.Wc + (c0 >> e.lhe);
            uint32_t cb[4], cr[4];
            if (e.lhe == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { fwd_c<ROUND>(px[k][q], cb[q], cr[q]); cb[q] &= a.mcb; cr[q] &= a.mcr; }
                pst4<NT>(e, fb, e.cb_off + k0, cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24));
                pst4<NT>(e, fb, e.cr_off + k0, cr[0] | (cr[1] << 8) | (cr[2] << 16) | (cr[3] << 24));
            } else if (e.lhe == 1) {
                fwd_c<ROUND>(px[k][0], cb[0], cr[0]);
                fwd_c<ROUND>(px[k][2], cb[2], cr[2]);
                pst2<NT>(e, fb, e.cb_off + k0, (cb[0] & a.mcb) | ((cb[2] & a.mcb) << 8));
                pst2<NT>(e, fb, e.cr_off + k0, (cr[0] & a.mcr) | ((cr[2] & a.mcr) << 8));
            } else {
                fwd_c<ROUND>(px[k][0], cb[0], cr[0]);
                pst1<NT>(e, fb, e.cb_off + k0, cb[0] & a.mcb);
                pst1<NT>(e, fb, e.cr_off + k0, cr[0] & a.mcr);
            }
        }
    }
    if (!CHECK) keep_tail_apart();
}

template <int ROUND, int MODE, bool NT>
__global__ void __launch_bounds__(256) k_planar_flat(KArgs a, PExtra e)
{
    pin_args(a);
    const uint32_t T = (uint32_t)e.T;
    const uint32_t ngroups = (uint32_t)((e.n + 3) >> 2);
    const uint32_t b0 = blockIdx.x * (T * PLANAR_K);
    const gin_t in = frame_in(a);
    const gbyte_t fb = planar_frame(e);
    // whole block inside the stream AND no ragged tail in it: the straight-line path
    if (b0 + T * PLANAR_K <= ngroups && (uint64_t)4 * (b0 + T * PLANAR_K) <= (uint64_t)e.n)
        planar_flat_body<ROUND, MODE, PLANAR_K, NT, false>(a, e, in, fb, b0 + threadIdx.x, T, ngroups);
    else
        planar_flat_body<ROUND, MODE, PLANAR_K, NT, true>(a, e, in, fb, b0 + threadIdx.x, T, ngroups);
}

// ------------------------------------------------------------------------------------------------
// k_planar_strided: factor f >= 2 (or any plan with module_width % 4 == 0 that is not the factor-1 image): k_decflat's mapping
// -- lane = 4 positions of the output stream spaced by the block size, so that every load instruction of a wave reads
// consecutive OUTPUT positions (input stride f * 4 bytes across lanes, the best the decimator allows) -- and then a 4 x 4
// transpose inside every quad of lanes, so that each lane ends up with 4 CONSECUTIVE positions and can store its Y (and Cb, Cr)
// bytes as one dword.  Loading 4 consecutive positions per lane instead (the first version of MODE 1) spread every load
// instruction over 4 x as many sectors at f = 2: 45 % of the roofline on 8192x8192 against 79 % for the packed k_decflat.
// The transpose is 4 DPP quad broadcasts + 2 v_perm + 1 v_lshl_or per plane: lane q of a quad collects byte q of its four lanes.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t quad_transpose_bytes(uint32_t w, uint32_t sel_lo, uint32_t sel_hi)
{
    const uint32_t a0 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0x00 /* quad_perm:[0,0,0,0] */, 0xF, 0xF, false);
    const uint32_t a1 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0x55 /* quad_perm:[1,1,1,1] */, 0xF, 0xF, false);
    const uint32_t a2 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0xAA /* quad_perm:[2,2,2,2] */, 0xF, 0xF, false);
    const uint32_t a3 = (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0xFF /* quad_perm:[3,3,3,3] */, 0xF, 0xF, false);
    // v_perm_b32(s0, s1, sel): selector bytes 0..3 pick from s1, 4..7 from s0
    const uint32_t lo = __builtin_amdgcn_perm(a1, a0, sel_lo);          // { a0.byte[q], a1.byte[q], 0, 0 }
    const uint32_t hi = __builtin_amdgcn_perm(a3, a2, sel_hi);          // { 0, 0, a2.byte[q], a3.byte[q] }
    return lo | hi;
}

template <int ROUND, bool NT, bool CHECK>
__device__ __forceinline__ void planar_strided_body(const KArgs &a, const PExtra &e, gin_t in, gbyte_t fb, uint32_t b0, uint32_t T)
{
    const uint32_t n = (uint32_t)e.n;
    const uint32_t tid = threadIdx.x, q = tid & 3u;
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t j = b0 + (uint32_t)k * T + tid;
        px[k] = in1<NT>(a, in, stream_in_off(a, CHECK ? min(j, n - 1u) : j));
    }
    uint32_t wy = 0, wb = 0, wr = 0;                                       // this lane's 4 positions, byte k = position b0 + k * T + tid
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t cb, cr;
        fwd_c<ROUND>(px[k], cb, cr);
        wy |= (fwd_y(px[k]) & a.my) << (8 * k);
        wb |= (cb & a.mcb) << (8 * k);
        wr |= (cr & a.mcr) << (8 * k);
    }
    // 0x0c = constant zero byte in v_perm_b32's selector
    const uint32_t sel_lo = 0x0c0c0000u | q | ((4u + q) << 8), sel_hi = 0x00000c0cu | (q << 16) | ((4u + q) << 24);
    const uint32_t y4 = quad_transpose_bytes(wy, sel_lo, sel_hi);
    const uint32_t cb4 = quad_transpose_bytes(wb, sel_lo, sel_hi);
    const uint32_t cr4 = quad_transpose_bytes(wr, sel_lo, sel_hi);
    // this lane now holds the group of 4 consecutive positions j0 .. j0 + 3 that its quad loaded in round k = q
    const uint32_t j0 = b0 + q * T + (tid & ~3u);
    if (CHECK && j0 >= n) return;
    if (CHECK && j0 + 3u >= n) {                                            // the stream's ragged tail: byte by byte
        for (uint32_t i = 0; j0 + i < n; ++i) {
            const uint32_t j = j0 + i;
            pst1<NT>(e, fb, (int64_t)j, (y4 >> (8 * i)) & 0xFFu);
            const uint32_t r = (uint32_t)(((uint64_t)j * e.mWm) >> e.kWm), c = j - r * (uint32_t)e.Wm;
            if ((c & ((1u << e.lhe) - 1u)) == 0 && (r & ((1u << e.lve) - 1u)) == 0) {
                const int64_t kk = (int64_t)(r >> e.lve) * e.Wc + (c >> e.lhe);
                pst1<NT>(e, fb, e.cb_off + kk, (cb4 >> (8 * i)) & 0xFFu);
                pst1<NT>(e, fb, e.cr_off + kk, (cr4 >> (8 * i)) & 0xFFu);
            }
        }
        return;
    }
    pst4<NT>(e, fb, (int64_t)j0, y4);
    // module_width % 4 == 0: the group sits in ONE chroma row at a column that is a multiple of 4
    const uint32_t r = (uint32_t)(((uint64_t)j0 * e.mWm) >> e.kWm), c0 = j0 - r * (uint32_t)e.Wm;
    if ((r & ((1u << e.lve) - 1u)) != 0) return;                            // a row without sample points
    const int64_t k0 = (int64_t)(r >> e.lve) * e.Wc + (c0 >> e.lhe);
    if (e.lhe == 0) {
        pst4<NT>(e, fb, e.cb_off + k0, cb4);
        pst4<NT>(e, fb, e.cr_off + k0, cr4);
    } else if (e.lhe == 1) {                                                // samples at positions 0 and 2 of the group
        pst2<NT>(e, fb, e.cb_off + k0, (cb4 & 0xFFu) | ((cb4 >> 8) & 0xFF00u));
        pst2<NT>(e, fb, e.cr_off + k0, (cr4 & 0xFFu) | ((cr4 >> 8) & 0xFF00u));
    } else {
        pst1<NT>(e, fb, e.cb_off + k0, cb4 & 0xFFu);
        pst1<NT>(e, fb, e.cr_off + k0, cr4 & 0xFFu);
    }
    if (!CHECK) keep_tail_apart();
}

template <int ROUND, bool NT>
__global__ void __launch_bounds__(256) k_planar_strided(KArgs a, PExtra e)
{
    pin_args(a);
    const uint32_t T = (uint32_t)e.T;                   // a multiple of 4: quads of lanes are quads of positions
    const uint32_t b0 = blockIdx.x * (T * 4u);
    const gin_t in = frame_in(a);
    const gbyte_t fb = planar_frame(e);
    // (every lane takes part in the quad exchange: no early exit before it)
    if ((uint64_t)b0 + (uint64_t)T * 4u <= (uint64_t)e.n) planar_strided_body<ROUND, NT, false>(a, e, in, fb, b0, T);
    else                                                   planar_strided_body<ROUND, NT, true>(a, e, in, fb, b0, T);
}

// ------------------------------------------------------------------------------------------------
// forward, AVG extension
// ------------------------------------------------------------------------------------------------
// factor 1, W % 4 == 0, H % VE == 0: a lane owns a 4-pixel x VE-row tile; K tiles per lane spaced by the block width
template <int ROUND, int HE, int VE, bool NT>
__global__ void __launch_bounds__(256) k_planar_avg_f1(KArgs a, PExtra e)
{
    constexpr int K = 2;
    constexpr int NLOG = (HE == 4 ? 2 : HE == 2 ? 1 : 0) + (VE == 2 ? 1 : 0);
    pin_args(a);
    const int W4 = a.W >> 2;
    const int x0 = blockIdx.x * (a.bdx * K) + threadIdx.x;
    if (x0 >= W4) return;
    const gin_t in = frame_in(a);
    const gbyte_t fb = planar_frame(e);
    const int ntr = a.H / VE;
    const u16x2 qmask = {(unsigned short)a.mcb, (unsigned short)a.mcr};
    for (int tr = blockIdx.y * a.bdy + threadIdx.y; tr < ntr; tr += a.row_step) {
        u32x4 p[K][VE];
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int x4 = min(x0 + t * a.bdx, W4 - 1);
#pragma unroll
            for (int i = 0; i < VE; ++i) p[t][i] = in4<NT>(a, in, (int64_t)(tr * VE + i) * a.ip + 4 * x4);
        }
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int x4 = x0 + t * a.bdx;
            if (x4 >= W4) continue;
            u16x2 C[VE][4];
#pragma unroll
            for (int i = 0; i < VE; ++i) {
                const uint32_t px[4] = {p[t][i].x, p[t][i].y, p[t][i].z, p[t][i].w};
                uint32_t y4 = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { y4 |= (fwd_y(px[j]) & a.my) << (8 * j); C[i][j] = fwd_c_pk<ROUND>(px[j]); }
                pst4<NT>(e, fb, (int64_t)(tr * VE + i) * a.W + 4 * x4, y4);
            }
            // HE x VE box averages: 4 / HE samples per tile
            uint32_t cb = 0, cr = 0;
            const u16x2 half = {(HE * VE) >> 1, (HE * VE) >> 1};
#pragma unroll
            for (int bj = 0; bj < 4; bj += HE) {
                u16x2 s = {0, 0};
#pragma unroll
                for (int i = 0; i < VE; ++i)
#pragma unroll
                    for (int j = 0; j < HE; ++j) s += C[i][bj + j];
                s = ((s + half) >> (unsigned short)NLOG) & qmask;
                cb |= (uint32_t)s.x << (8 * (bj / HE));
                cr |= (uint32_t)s.y << (8 * (bj / HE));
            }
            const int64_t k0 = (int64_t)tr * e.Wc + x4 * (4 / HE);
            if (HE == 1) { pst4<NT>(e, fb, e.cb_off + k0, cb); pst4<NT>(e, fb, e.cr_off + k0, cr); }
            else if (HE == 2) { pst2<NT>(e, fb, e.cb_off + k0, cb); pst2<NT>(e, fb, e.cr_off + k0, cr); }
            else { pst1<NT>(e, fb, e.cb_off + k0, cb); pst1<NT>(e, fb, e.cr_off + k0, cr); }
        }
    }
}

// any factor, any shape with a whole tile: k_avg's body (csic_avg_tile.h: 4 x max(f, v) tiles in registers, edge blocks for the
// cut tiles) computing packed YCbCr -- under AVG every pixel carries its chroma block's average -- with a sink that scatters the
// bytes into the planes instead of packing pixels: the Y byte of every position, Cb / Cr at the sample points, which the AVG
// layout puts at every (max(1, h / f))-th column of every (max(1, v / f))-th row of the output (csic.h).  A tile yields 4 / f
// consecutive positions of max(f, v) / f rows (one position per lane pair at f = 8).  Stores are as wide as the run is long where
// the plane's rows keep them aligned (wave-uniform), single bytes otherwise.
template <int LHE, int LVE>
struct PlanarSink {
    const PExtra &e;
    gbyte_t fb;
    int Wo;
    // n bytes (n = 1, 2, 4; v holds them little-endian) at byte offset off of the planar frame
    template <int NB> __device__ __forceinline__ void run(int64_t off, uint32_t v, bool aligned) const
    {
        if (NB == 1) pst1<true>(e, fb, off, v & 0xFFu);
        else if (aligned) { if (NB == 2) pst2<true>(e, fb, off, v); else pst4<true>(e, fb, off, v); }
        else {
#pragma unroll
            for (int i = 0; i < NB; ++i) pst1<true>(e, fb, off + i, (v >> (8 * i)) & 0xFFu);
        }
    }
    template <int N> __device__ __forceinline__ void put(int row, int col, const uint32_t (&o)[N]) const
    {
        static_assert(N == 1 || N == 2 || N == 4, "a tile yields 1, 2 or 4 positions per row");
        constexpr int NS = (N >> LHE) > 0 ? (N >> LHE) : 1;             // chroma samples among the N positions (N < hold_h: one or none)
        uint32_t y = 0, cb = 0, cr = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) y |= (o[i] & 0xFFu) << (8 * i);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            cb |= ((o[i << LHE] >> 8) & 0xFFu) << (8 * i);
            cr |= ((o[i << LHE] >> 16) & 0xFFu) << (8 * i);
        }
        // col is a multiple of N: a run is aligned iff its plane's rows are a multiple of its length apart
        run<N>((int64_t)row * Wo + col, y, (Wo & (N - 1)) == 0);
        if ((row & ((1 << LVE) - 1)) == 0 && (N >= (1 << LHE) || (col & ((1 << LHE) - 1)) == 0)) {
            const int64_t k = (int64_t)(row >> LVE) * e.Wc + (col >> LHE);
            const bool al = (e.Wc & (NS - 1)) == 0;
            run<NS>(e.cb_off + k, cb, al);
            run<NS>(e.cr_off + k, cr, al);
        }
    }
    __device__ __forceinline__ void put_edge(int row, int col, uint32_t v) const
    {
        pst1<false>(e, fb, (int64_t)row * Wo + col, v & 0xFFu);
        if ((col & ((1 << LHE) - 1)) == 0 && (row & ((1 << LVE) - 1)) == 0) {
            const int64_t k = (int64_t)(row >> LVE) * e.Wc + (col >> LHE);
            pst1<false>(e, fb, e.cb_off + k, (v >> 8) & 0xFFu);
            pst1<false>(e, fb, e.cr_off + k, (v >> 16) & 0xFFu);
        }
    }
};

template <int ROUND, int F, int HH, int VV>
__global__ void __launch_bounds__(256) k_planar_avg_tile(KArgs a, PExtra e)
{
    constexpr int HOLD_H = HH > F ? HH / F : 1, HOLD_V = VV > F ? VV / F : 1;        // csic_planar_layout under AVG
    constexpr int LHE = HOLD_H == 4 ? 2 : HOLD_H == 2 ? 1 : 0, LVE = HOLD_V == 2 ? 1 : 0;
    pin_args(a);
    const PlanarSink<LHE, LVE> sink{e, planar_frame(e), a.Wo};
    avg_kernel_body<ROUND, F_YCC, F, HH, VV, true, (F <= 2 ? 2 : 1)>(a, frame_in(a), sink);
}

// any factor, any shape: one output position per lane by the definition
template <int ROUND>
__global__ void __launch_bounds__(256) k_planar_avg_gen(KArgs a, PExtra e)
{
    pin_args(a);
    const int co = blockIdx.x * a.bdx + threadIdx.x;
    if (co >= a.Wo) return;
    const gin_t in = frame_in(a);
    const gbyte_t fb = planar_frame(e);
    for (int ro = blockIdx.y * a.bdy + threadIdx.y; ro < a.Ho; ro += a.row_step) {
        const uint32_t ycc = avg_pixel_generic<ROUND, F_YCC, F_ARGB>(a, in, ro, co);    // Y | Cb << 8 | Cr << 16, quantised
        pst1<false>(e, fb, (int64_t)ro * a.Wo + co, ycc & 0xFFu);
        if ((co & ((1 << e.lhe) - 1)) == 0 && (ro & ((1 << e.lve) - 1)) == 0) {           // module_width == Wo under AVG
            const int64_t k = (int64_t)(ro >> e.lve) * e.Wc + (co >> e.lhe);
            pst1<false>(e, fb, e.cb_off + k, (ycc >> 8) & 0xFFu);
            pst1<false>(e, fb, e.cr_off + k, (ycc >> 16) & 0xFFu);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// reconstruct: planar -> packed
// ------------------------------------------------------------------------------------------------
// PLANAR as a plane source of csic_plane_read.h: a sample is a byte, a word the aligned dword that holds the first sample, shifted
// into place (planes are padded to 256 bytes)
struct BytePlanes {
    typedef int64_t idx;
    const PExtra &e;
    gcbyte_t fb;
    __device__ __forceinline__ int64_t plane(int p) const { return p == 1 ? e.cb_off : e.cr_off; }
    template <bool NT> __device__ __forceinline__ uint32_t y_word(uint32_t j0) const { return by_ld4<NT>(e.frame_bytes, fb, (int64_t)j0); }
    __device__ __forceinline__ uint32_t c_word(int p, idx k0) const
    { return by_ld4<false>(e.frame_bytes, fb, (plane(p) + k0) & ~(int64_t)3) >> (8u * (uint32_t)(k0 & 3)); }
    __device__ __forceinline__ uint32_t y_at(uint32_t w, uint32_t i) const { return (w >> (8u * i)) & 0xFFu; }
    __device__ __forceinline__ uint32_t c_at(int, uint32_t w, uint32_t i) const { return (w >> (8u * i)) & 0xFFu; }
    __device__ __forceinline__ uint32_t y_one(uint32_t j) const { return by_ld1(e.frame_bytes, fb, (int64_t)j); }
    __device__ __forceinline__ uint32_t c_one(int p, idx k) const { return by_ld1(e.frame_bytes, fb, plane(p) + k); }
};

template <int FMT, bool FAST, bool NT>
__global__ void __launch_bounds__(256) k_recon(KArgs a, PExtra e)
{
    pin_args(a);
    (void)a;
    const uint32_t T = (uint32_t)e.T;
    const uint32_t ngroups = (uint32_t)((e.n + 3) >> 2);
    const uint32_t b0 = blockIdx.x * (T * RECON_K);
    const gcbyte_t fb = (gcbyte_t)planar_frame(e);
    const gout_t out = (gout_t)(uintptr_t)e.packed + (int64_t)blockIdx.z * e.n;
    if (b0 + T * RECON_K <= ngroups && (uint64_t)4 * (b0 + T * RECON_K) <= (uint64_t)e.n)
        recon_body<FMT, FAST, NT, false, RECON_K, BytePlanes>(e, fb, out, b0 + threadIdx.x, T, ngroups);
    else
        recon_body<FMT, FAST, NT, true, RECON_K, BytePlanes>(e, fb, out, b0 + threadIdx.x, T, ngroups);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using PlanarFn = void (*)(KArgs, PExtra);

static void fill_extra(const csic_planar_layout &L, PExtra *e)
{
    std::memset(e, 0, sizeof *e);
    e->cb_off = L.cb_offset; e->cr_off = L.cr_offset; e->frame_bytes = L.frame_bytes;
    e->n = (int64_t)L.y_width * L.y_height;
    e->Wm = L.module_width; e->Wc = L.chroma_width; e->lhe = ilog2(L.hold_h); e->lve = ilog2(L.hold_v); e->replay_last = L.replay_last;
    magic_div((uint32_t)L.module_width, &e->mWm, &e->kWm);
}

// the kernel of a forward kind (he, ve: the layout's holds; g: the plan's geometry, for the tile kernel)
static PlanarFn forward_kernel(PlanarKind kind, int rounding, bool nontemporal, int he, int ve, const Geometry &g)
{
    return with_const<R_FLOOR, R_TRUNC>(rounding, [&](auto round) {
    return with_const<true, false>(nontemporal, [&](auto nt) -> PlanarFn {
        constexpr int ROUND = CSIC_CONST(round);
        constexpr bool NT = CSIC_CONST(nt);
        const auto hv = [](int h, int v, auto pick) {
            return with_const<1, 2, 4>(h, [&](auto hc) { return with_const<1, 2>(v, [&](auto vc) { return pick(hc, vc); }); });
        };
        switch (kind) {
        case PLANAR_FLAT_GEN: return k_planar_flat<ROUND, 0, NT>;
        case PLANAR_STRIDED: return k_planar_strided<ROUND, NT>;
        case PLANAR_FLAT_4PL: return k_planar_flat<ROUND, 1, NT>;
        case PLANAR_FLAT_F1X4: return k_planar_flat<ROUND, 2, NT>;
        case PLANAR_AVG_F1: return hv(he, ve, [](auto h, auto v) -> PlanarFn { return k_planar_avg_f1<ROUND, CSIC_CONST(h), CSIC_CONST(v), NT>; });
        case PLANAR_AVG_TILE:
            return with_const<1, 2, 4, 8>(g.f, [&](auto f) {
                return hv(g.h, g.v, [](auto h, auto v) -> PlanarFn { return k_planar_avg_tile<ROUND, CSIC_CONST(f), CSIC_CONST(h), CSIC_CONST(v)>; });
            });
        case PLANAR_AVG_GEN: break;
        }
        return k_planar_avg_gen<ROUND>;
    }); });
}

// kernel, grid, block and both argument blocks of one forward launch over nz <= 65535 frames whose pointers OR to align_bits: what
// plan_planar decides (csic_select.cpp), the kernel of that kind and PExtra from the layout; the frame pointers stay unset
static int planar_resolve(const csic_plan *pl, uintptr_t align_bits, int nz, PlanarLaunchDesc *d)
{
    PlanarPlan pp;
    const int st = plan_planar(pl->p, pl->g, pl->tune, align_bits, nz, &pp);
    if (st != CSIC_OK) return st;
    csic_planar_layout L;
    planar_layout(pl->g, &pl->p, &L);
    fill_extra(L, &d->extra);
    d->extra.T = pp.T;
    d->args = pp.args;
    d->fn = forward_kernel(pp.kind, pl->p.rounding, !pl->tune.no_nt, L.hold_h, L.hold_v, pl->g);
    d->grid = dim3(pp.grid.x, pp.grid.y, pp.grid.z);
    d->block = dim3(pp.block.x, pp.block.y, pp.block.z);
    return CSIC_OK;
}

int planar_enqueue(const PlanarLaunchDesc &d, hipStream_t stream) { return launch(d.fn, d.grid, d.block, stream, d.args, d.extra); }

int planar_forward(const csic_plan *pl, const void *d_in, void *d_planar, int nframes, hipStream_t stream)
{
    if (!d_in || !d_planar) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    if (((uintptr_t)d_planar & 255u) || ((uintptr_t)d_in & 3u))
        return set_error(CSIC_EINVAL_SIZE, "a planar frame buffer must be 256-byte aligned (and the input 4-byte aligned)");
    return for_frame_batches(nframes, [&](int f0, int nz) {
        PlanarLaunchDesc d;
        const int st = planar_resolve(pl, (uintptr_t)d_in | (uintptr_t)d_planar, nz, &d);
        if (st != CSIC_OK) return st;
        d.args.in = static_cast<const uint32_t *>(d_in) + (int64_t)f0 * d.args.in_frame_px;
        d.extra.planar = static_cast<uint8_t *>(d_planar) + (int64_t)f0 * d.extra.frame_bytes;
        return planar_enqueue(d, stream);
    });
}

int planar_prepare_table(const csic_plan *pl, const void *const *d_in_tab, void *const *d_planar_tab, uintptr_t align_bits, int nframes,
                         PlanarLaunchDesc *d)
{
    if (!pl) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_in_tab || !d_planar_tab) return set_error(CSIC_EINVAL_NULL, "frame table is NULL");
    if (nframes <= 0 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes per launch must be in 1..65535. Got %d", nframes);
    if (align_bits & 3u) return set_error(CSIC_EINVAL_SIZE, "frame buffers must be 4-byte aligned");
    const int st = planar_resolve(pl, align_bits, nframes, d);
    if (st != CSIC_OK) return st;
    d->args.in_tab = reinterpret_cast<const uint32_t *const *>(d_in_tab);
    d->extra.planar_tab = reinterpret_cast<const uint64_t *>(d_planar_tab);
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" int csic_reconstruct_device(csic_plan *plan, const void *d_planar, void *d_out, int32_t nframes, int32_t out_format,
                                       void *hip_stream)
{
    return reconstruct_device(plan, d_planar, &PExtra::planar, d_out, nframes, out_format, hip_stream, "csic_reconstruct_device",
                              "a planar frame buffer must be 256-byte aligned and the packed output 16-byte aligned", RECON_K,
                              [](const csic_plan *pl, PExtra *e) { csic_planar_layout L; planar_layout(pl->g, &pl->p, &L); fill_extra(L, e); },
                              [](auto fmt, auto fast, auto nt) -> PlanarFn { return k_recon<CSIC_CONST(fmt), CSIC_CONST(fast), CSIC_CONST(nt)>; });
}
