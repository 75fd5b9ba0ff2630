// csic_ssim.hip -- csic_ssim_device: the per-channel sums of the 8 x 8 block SSIM (16.16 fixed point, integer throughout) between
// input frames and the output their plan's parameters produce.  Channels and pairing are csic_distortion_*'s (R, G, B against the
// packed ARGB output, Y, Cb, Cr against the packed YCbCr output; input pixel (r, c) against output pixel (r / f, c / f)); the
// definition -- windows, the five sums, N, D and the quotient q -- is in include/csic.h.  Fused like csic_distortion.hip: every
// input byte is read once and the output is never written -- only a 48-byte partial per block and, on request, the map of q.
//
// Kernels (wave64, 256-thread blocks = 32 windows; a window belongs to 8 adjacent lanes of one wave):
//   k_ssim_fast<ROUND, F, HH, VV, VEC, NT>  the class of k_dist_fast (HOLD_DECIMATE, ARGB input, factor F in {1, 2}, chroma before
//                      spatial at F = 2) on frames of whole windows (width % 8 == 0 and height % 8 == 0).  Lane l of a window takes
//                      its rows 2 (l / 2), 2 (l / 2) + 1 and its columns 4 (l % 2) .. + 3: one 16-byte load per row (VEC; four 4-byte
//                      loads for a d_in that is only 4-byte aligned), both issued before any arithmetic.  The lane then holds every
//                      pixel its outputs take Y and held chroma from (HH divides 4; at F = 2 the output row's source is the even row),
//                      so the hold is a byte select; only the 4:x:0 odd row at F = 1 needs one more pixel, the last chroma sample of
//                      the row above -- one load whose address is uniform over the lanes of a row pair.  The four pixels of a row are
//                      transposed into one dword per channel (v_perm_b32) for the reference and for the output, and the sums are
//                      v_dot4_u32_u8: sum x = dot4(x, 0x01010101), sum x^2 = dot4(x, x), sum xy = dot4(x, y) -- five per channel per
//                      four pixels.  The quantiser is one AND on the transposed dword.
//   k_ssim_gen<ROUND, AVG, INFMT>   anything csic_validate accepts: lane l of a window takes its row l.  The output pixel of each
//                      f-wide run of the row is hold_pixel_generic's (both order classes, 4:x:0 replay row included; written out
//                      in the kernel, see there) or avg_pixel_generic's for AVG, the sums are scalar multiply-adds.  The lanes of a
//                      window that share an output row each compute it: f-fold redundant arithmetic on cached loads, the price of a
//                      kernel without a second mapping.
//   k_sum_partials     (csic_measure.h) one block per frame: the frame's partials, summed in a fixed order, -> d_ssim[frame * 6 + channel].
// Which of the two a plan takes is measure_kind (csic_select.cpp); what this unit shares with csic_distortion.hip is csic_measure.h.
// Both pixel kernels end in ssim_finish: the 8 lanes' sums are added with three DPP steps (quad_perm xor 1, xor 2, row_half_mirror),
// lane l < 6 of the window then takes channel l, so that N, D and the 64-bit quotient are evaluated once per wave for all 8 windows
// x 6 channels instead of six times with an eighth of the lanes live.
// Widths: a lane sums at most 8 pixels of 8 bits -- sum x <= 2040, sum x^2 + sum y^2 <= 1 040 400, sum xy <= 520 200; a window
// sum x <= 16 320 (sum x and sum y share a dword through the reduction), sum x^2 + sum y^2 <= 8 323 200, sum xy <= 4 161 600, and
// 64 times either of the last two is below 2^30.  N and D are 64-bit products of two 32-bit factors.  q fits 18 bits, a wave's sum of
// 8 of them 21; the block sum, the partials and the per-frame sums are int64.  No atomics: each block writes its own partial.
#include <cstdio>

#include "csic_measure.h"

namespace csic {

constexpr int SSIM_T = MEAS_T;
constexpr int SSIM_CH = MEAS_CH;
constexpr int SSIM_WPB = SSIM_T / 8;            // windows per block
constexpr uint32_t SSIM_C1 = 416u, SSIM_C2 = 235963u;
static_assert(CSIC_SSIM_WINDOW == 8 && CSIC_SSIM_ONE == 65536, "the kernels are written for 8 x 8 windows and 16.16 quotients");

struct SExtra {
    int64_t *part;                   // workspace: nblk partials of SSIM_CH int64 per frame, frames back to back
    int32_t *map;                    // [frame][channel][H / 8][W / 8], or NULL
    uint32_t nblk;                   // blocks (= partials) per frame
    uint32_t nwin, nwx;              // windows per frame and per window row
    uint32_t mNwx, kNwx;             // exact n / nwx (magic_div)
};

typedef int64_t CSIC_GLOBAL *gspart_t;
typedef int32_t CSIC_GLOBAL *gsmap_t;

// what a lane knows of its window: sum x | sum y << 16, sum x^2 + sum y^2, sum xy, per channel
struct WSums { uint32_t s12[SSIM_CH], ss[SSIM_CH], sxy[SSIM_CH]; };

__device__ __forceinline__ uint32_t group8_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm:[2,3,0,1] */, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141 /* row_half_mirror: lane i <- lane 7 - i */, 0xF, 0xF, false);
    return v;
}

// floor(a / b) for a < 2^63, 0 < b < 2^47 and a quotient of at most 17 bits: the double quotient is within 2^-35 of the real one,
// so its integer part is off by at most one either way, and one remainder test settles it.
__device__ __forceinline__ uint32_t div_exact(uint64_t a, uint64_t b)
{
    uint32_t q = (uint32_t)((double)a / (double)b);
    const int64_t r = (int64_t)(a - (uint64_t)q * b);
    if (r < 0) --q;
    else if ((uint64_t)r >= b) ++q;
    return q;
}

// q of one window and channel from its four sums (include/csic.h)
__device__ __forceinline__ int32_t ssim_q(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12)
{
    const uint32_t p = s1 * s2, sq = s1 * s1 + s2 * s2;                      // <= 16320^2, <= 2 * 16320^2
    const int32_t covar = (int32_t)(64u * s12) - (int32_t)p;
    const uint32_t vars = 64u * ss - sq;
    const int64_t n = (int64_t)(2u * p + SSIM_C1) * (int64_t)(2 * covar + (int32_t)SSIM_C2);
    const uint64_t d = (uint64_t)(sq + SSIM_C1) * (uint64_t)(vars + SSIM_C2);
    const uint32_t q = div_exact(64ull * (uint64_t)(n < 0 ? -n : n), d >> 10);
    return n < 0 ? -(int32_t)q : (int32_t)q;
}

// lane sums -> window sums -> q of channel (lane % 8) in the lanes with lane % 8 < 6 -> the map, and this block's 64-bit partial
__device__ __forceinline__ void ssim_finish(const SExtra &e, WSums &w, uint32_t wi, bool valid)
{
    __shared__ int32_t red[SSIM_T / 64][SSIM_CH];
#pragma unroll
    for (int ch = 0; ch < SSIM_CH; ++ch) { w.s12[ch] = group8_sum(w.s12[ch]); w.ss[ch] = group8_sum(w.ss[ch]); w.sxy[ch] = group8_sum(w.sxy[ch]); }
    const uint32_t gl = threadIdx.x & 7u;
    uint32_t s12 = w.s12[0], ss = w.ss[0], sxy = w.sxy[0];
#pragma unroll
    for (int ch = 1; ch < SSIM_CH; ++ch)
        if (gl == (uint32_t)ch) { s12 = w.s12[ch]; ss = w.ss[ch]; sxy = w.sxy[ch]; }
    int32_t q = ssim_q(s12 & 0xFFFFu, s12 >> 16, ss, sxy);
    const bool mine = valid && gl < (uint32_t)SSIM_CH;
    if (!mine) q = 0;
    if (e.map && mine) {
        const uint64_t at = ((uint64_t)blockIdx.z * SSIM_CH + gl) * e.nwin + wi;
        CSIC_CHECK(wi < e.nwin);
        ((gsmap_t)(uintptr_t)e.map)[at] = q;
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) q += __shfl_xor(q, off, 64);
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    if (lane < SSIM_CH) red[wave][lane] = q;
    __syncthreads();
    if (threadIdx.x < (unsigned)SSIM_CH) {
        int64_t t = 0;
#pragma unroll
        for (int k = 0; k < SSIM_T / 64; ++k) t += red[k][threadIdx.x];
        CSIC_CHECK(blockIdx.x < e.nblk);
        ((gspart_t)(uintptr_t)e.part)[((uint64_t)blockIdx.z * e.nblk + blockIdx.x) * SSIM_CH + threadIdx.x] = t;
    }
}

// The window of this lane's group.  The groups past the frame's last window in its last block take that window again, so that
// they run the same loads and cross-lane steps, and ssim_finish drops what they compute.
__device__ __forceinline__ uint32_t window_of_lane(const SExtra &e, bool &valid, uint32_t &wy, uint32_t &wx)
{
    const uint32_t wi0 = blockIdx.x * (uint32_t)SSIM_WPB + (threadIdx.x >> 3);
    valid = wi0 < e.nwin;
    const uint32_t wi = valid ? wi0 : e.nwin - 1u;
    wy = (uint32_t)(((uint64_t)wi * e.mNwx) >> e.kNwx);
    wx = wi - wy * e.nwx;
    return wi;
}

// ------------------------------------------------------------------------------------------------
// k_ssim_fast
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) { return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24); }
// byte 1 of four clamped 16-bit values -> one dword
__device__ __forceinline__ uint32_t pack4_b1(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3)
{
    const uint32_t lo = __builtin_amdgcn_perm(v1, v0, 0x0c0c0501u), hi = __builtin_amdgcn_perm(v3, v2, 0x0c0c0501u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
// bytes { 0, 0, 2, 2 } (H == 2) or { 0, 0, 0, 0 } (H == 4) of a transposed dword: a horizontal hold inside four pixels
template <int H>
__device__ __forceinline__ uint32_t hold4(uint32_t v)
{
    if (H == 1) return v;
    return __builtin_amdgcn_perm(v, v, H == 2 ? 0x02020000u : 0x00000000u);
}

// four pixels of one row, one dword per channel: reference (x) and output (y) -> the lane's sums
__device__ __forceinline__ void acc4(uint32_t (&s1)[SSIM_CH], uint32_t (&s2)[SSIM_CH], WSums &w, const uint32_t (&x)[SSIM_CH], const uint32_t (&y)[SSIM_CH])
{
#pragma unroll
    for (int ch = 0; ch < SSIM_CH; ++ch) {
        s1[ch] = __builtin_amdgcn_udot4(x[ch], 0x01010101u, s1[ch], false);
        s2[ch] = __builtin_amdgcn_udot4(y[ch], 0x01010101u, s2[ch], false);
        w.ss[ch] = __builtin_amdgcn_udot4(x[ch], x[ch], w.ss[ch], false);
        w.ss[ch] = __builtin_amdgcn_udot4(y[ch], y[ch], w.ss[ch], false);
        w.sxy[ch] = __builtin_amdgcn_udot4(x[ch], y[ch], w.sxy[ch], false);
    }
}

// The reference of four ARGB pixels: R, G, B transposed out of the pixels (7 v_perm_b32), Y, Cb, Cr through the forward transform
// (scalar values in ry / rcb / rcr as well: the output's inverse transform wants them one by one).
template <int ROUND>
__device__ __forceinline__ void ref4(const u32x4 &p, uint32_t (&x)[SSIM_CH], uint32_t (&ry)[4], uint32_t (&rcb)[4], uint32_t (&rcr)[4])
{
    const uint32_t bg01 = __builtin_amdgcn_perm(p.y, p.x, 0x05010400u), ra01 = __builtin_amdgcn_perm(p.y, p.x, 0x07030602u);
    const uint32_t bg23 = __builtin_amdgcn_perm(p.w, p.z, 0x05010400u), ra23 = __builtin_amdgcn_perm(p.w, p.z, 0x07030602u);
    x[0] = __builtin_amdgcn_perm(ra23, ra01, 0x05040100u);
    x[1] = __builtin_amdgcn_perm(bg23, bg01, 0x07060302u);
    x[2] = __builtin_amdgcn_perm(bg23, bg01, 0x05040100u);
    const uint32_t q[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { ry[i] = fwd_y(q[i]); fwd_c<ROUND>(q[i], rcb[i], rcr[i]); }
    x[3] = pack4(ry[0], ry[1], ry[2], ry[3]);
    x[4] = pack4(rcb[0], rcb[1], rcb[2], rcb[3]);
    x[5] = pack4(rcr[0], rcr[1], rcr[2], rcr[3]);
}

template <int ROUND, int F, int HH, int VV, bool VEC, bool NT>
__global__ void __launch_bounds__(SSIM_T) k_ssim_fast(KArgs a, SExtra e)
{
    pin_args(a);
    const gin_t in = frame_in(a);
    bool valid;
    uint32_t wy, wx;
    const uint32_t wi = window_of_lane(e, valid, wy, wx);
    const uint32_t gl = threadIdx.x & 7u, W = (uint32_t)a.W;
    const uint32_t r0 = 8u * wy + 2u * (gl >> 1);                               // even; < 2^24 (measure_kind)
    const uint32_t off = __umul24(r0, W) + 8u * wx + 4u * (gl & 1u);            // < 2^30
    uint32_t cpx = 0;
    // 4:x:0 at F = 1: the odd row holds the chroma latched at the last sample of the row above (ChromaSubsampler.scala:52-65)
    if (F == 1 && VV == 2) cpx = in1n<false>(a, in, __umul24(r0, W) + (uint32_t)a.last_sample_col);
    const u32x4 p0 = in4n_or_1n<VEC, NT>(a, in, off), p1 = in4n_or_1n<VEC, NT>(a, in, off + W);

    const uint32_t my4 = (a.my & 0xFFu) * 0x01010101u, mcb4 = (a.mcb & 0xFFu) * 0x01010101u, mcr4 = (a.mcr & 0xFFu) * 0x01010101u;
    uint32_t s1[SSIM_CH] = {0, 0, 0, 0, 0, 0}, s2[SSIM_CH] = {0, 0, 0, 0, 0, 0};
    WSums w;
#pragma unroll
    for (int ch = 0; ch < SSIM_CH; ++ch) w.ss[ch] = w.sxy[ch] = 0;
    uint32_t x[SSIM_CH], y[SSIM_CH], ry[4], rcb[4], rcr[4];
    ref4<ROUND>(p0, x, ry, rcb, rcr);
    if constexpr (F == 1) {
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            if (row == 1) ref4<ROUND>(p1, x, ry, rcb, rcr);
            const bool held_row = VV == 2 && row == 1;
            uint32_t ocb = 0, ocr = 0;
            if (held_row) fwd_c<ROUND>(cpx, ocb, ocr);
            Rgb16 o[4];
#pragma unroll
            for (int g = 0; g < 4; g += HH) {
                const ChromaTerm t = chroma_term_q<F_ARGB>((held_row ? ocb : rcb[g]) & a.mcb, (held_row ? ocr : rcr[g]) & a.mcr);
#pragma unroll
                for (int i = g; i < g + HH; ++i) o[i] = rgb16_of(ry[i] & a.my, t);
            }
            y[0] = pack4_b1(o[0].r, o[1].r, o[2].r, o[3].r);
            y[1] = pack4_b1(o[0].g, o[1].g, o[2].g, o[3].g);
            y[2] = pack4_b1(o[0].b, o[1].b, o[2].b, o[3].b);
            y[3] = x[3] & my4;
            y[4] = (held_row ? ocb * 0x01010101u : hold4<HH>(x[4])) & mcb4;
            y[5] = (held_row ? ocr * 0x01010101u : hold4<HH>(x[5])) & mcr4;
            acc4(s1, s2, w, x, y);
        }
    } else {
        // outputs (r0 / 2, 4 wx + 2 (gl & 1) + o), o = 0, 1: Y of this lane's column 2 o of the even row, chroma held from column
        // 2 o & ~(h - 1) of it; both rows of the lane are measured against them
        Rgb16 o[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int src = HH == 4 ? 0 : 2 * k;
            o[k] = rgb16_of(ry[2 * k] & a.my, chroma_term_q<F_ARGB>(rcb[src] & a.mcb, rcr[src] & a.mcr));
        }
        y[0] = __builtin_amdgcn_perm(o[1].r, o[0].r, 0x05050101u);
        y[1] = __builtin_amdgcn_perm(o[1].g, o[0].g, 0x05050101u);
        y[2] = __builtin_amdgcn_perm(o[1].b, o[0].b, 0x05050101u);
        y[3] = hold4<2>(x[3]) & my4;
        y[4] = hold4<HH == 4 ? 4 : 2>(x[4]) & mcb4;
        y[5] = hold4<HH == 4 ? 4 : 2>(x[5]) & mcr4;
        acc4(s1, s2, w, x, y);
        ref4<ROUND>(p1, x, ry, rcb, rcr);
        acc4(s1, s2, w, x, y);
    }
#pragma unroll
    for (int ch = 0; ch < SSIM_CH; ++ch) w.s12[ch] = s1[ch] | (s2[ch] << 16);
    ssim_finish(e, w, wi, valid);
}

// ------------------------------------------------------------------------------------------------
// k_ssim_gen
// ------------------------------------------------------------------------------------------------
template <int ROUND, bool AVG, int INFMT>
__global__ void __launch_bounds__(SSIM_T) k_ssim_gen(KArgs a, SExtra e)
{
    pin_args(a);
    const gin_t in = frame_in(a);
    bool valid;
    uint32_t wy, wx;
    const uint32_t wi = window_of_lane(e, valid, wy, wx);
    const int r = (int)(8u * wy + (threadIdx.x & 7u)), c0 = (int)(8u * wx);
    const int ro = r >> a.sc_shift;
    WSums w;
#pragma unroll
    for (int ch = 0; ch < SSIM_CH; ++ch) w.s12[ch] = w.ss[ch] = w.sxy[ch] = 0;
    uint32_t out[SSIM_CH] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        if ((j & (a.f - 1)) == 0) {
            // a new output pixel (ro, co): f divides 8 and c0 is a multiple of 8
            const int co = c >> a.sc_shift;
            uint32_t y, cb, cr;
            if (AVG) {
                const uint32_t o = avg_pixel_generic<ROUND, F_YCC, INFMT>(a, in, ro, co);
                y = o & 0xFFu; cb = (o >> 8) & 0xFFu; cr = (o >> 16) & 0xFFu;
            } else {
                // hold_pixel_generic (csic_kernel_ops.h) written out: inside this 8-fold unrolled loop the call compiles to a
                // longer schedule (12 instructions more, 0.5-0.7 % slower on 8192 x 8192: profiles/r10_measure_refactor.md).
                // The rule is stated THERE; change it there first and keep this copy equal to it.
                const int64_t y_idx = (int64_t)(ro * a.f) * a.ip + co * a.f;
                int64_t c_idx;
                if (!a.s_first) {
                    const int rs = ro * a.f, cs = co * a.f;
                    c_idx = ((rs & a.vmask) == 0) ? (int64_t)rs * a.ip + (cs & ~a.hmask) : (int64_t)(rs - 1) * a.ip + a.last_sample_col;
                } else {
                    const int jj = ro * a.Wo + co;
                    const int rs = (int)(((uint64_t)(uint32_t)jj * a.mW) >> a.kW), cs = jj - rs * a.W;
                    const int src = ((rs & a.vmask) == 0) ? (jj - (cs & a.hmask)) : ((rs - 1) * a.W + a.last_sample_col);
                    const int sro = (int)(((uint64_t)(uint32_t)src * a.mWo) >> a.kWo), sco = src - sro * a.Wo;
                    c_idx = (int64_t)(sro * a.f) * a.ip + sco * a.f;
                }
                in_c<ROUND, INFMT>(in1<false>(a, in, c_idx), cb, cr);
                cb &= a.mcb; cr &= a.mcr;
                y = in_y<ROUND, INFMT>(in1<false>(a, in, y_idx)) & a.my;
            }
            const Rgb16 o = rgb16_of(y, chroma_term_q<F_ARGB>(cb, cr));
            out[0] = o.r >> 8; out[1] = o.g >> 8; out[2] = o.b >> 8; out[3] = y; out[4] = cb; out[5] = cr;
        }
        uint32_t ref[SSIM_CH];
        ref_channels<ROUND, INFMT, true>(in1<false>(a, in, (int64_t)r * a.ip + c), ref);
#pragma unroll
        for (int ch = 0; ch < SSIM_CH; ++ch) {
            w.s12[ch] += ref[ch] | (out[ch] << 16);
            w.ss[ch] += __umul24(ref[ch], ref[ch]) + __umul24(out[ch], out[ch]);
            w.sxy[ch] += __umul24(ref[ch], out[ch]);
        }
    }
    ssim_finish(e, w, wi, valid);
}

// ------------------------------------------------------------------------------------------------
// host side: what csic_measure.h asks of a unit
// ------------------------------------------------------------------------------------------------
struct SsimUnit {
    typedef SExtra Extra;
    static constexpr MeasureFamily family = MEASURE_SSIM;
    static constexpr const char *result_name = "d_ssim", *workspace_fn = "csic_ssim_workspace_bytes";
    static int check_plan(const csic_plan *pl)
    {
        if (pl->g.W < CSIC_SSIM_WINDOW || pl->g.H < CSIC_SSIM_WINDOW)
            return set_error(CSIC_EINVAL_DIMS, "a %dx%d frame has no %dx%d window", pl->g.W, pl->g.H, CSIC_SSIM_WINDOW, CSIC_SSIM_WINDOW);
        return CSIC_OK;
    }
    static int check_extra(const SExtra &e)
    {
        if ((uintptr_t)e.map & 3u) return set_error(CSIC_EINVAL_SIZE, "d_map must be 4-byte aligned");
        return CSIC_OK;
    }
    static uint32_t windows(const csic_plan *pl) { return (uint32_t)(pl->g.W / CSIC_SSIM_WINDOW) * (uint32_t)(pl->g.H / CSIC_SSIM_WINDOW); }
    static uint32_t blocks(const csic_plan *pl, int) { return (windows(pl) + SSIM_WPB - 1) / SSIM_WPB; }
    static void fill_extra(const csic_plan *pl, int, SExtra *e)
    {
        e->nwin = windows(pl);
        e->nwx = (uint32_t)(pl->g.W / CSIC_SSIM_WINDOW);
        magic_div(e->nwx, &e->mNwx, &e->kNwx);
    }
    static MeasureFn<SExtra> kernel(const csic_plan *pl, int kind, bool vec)
    {
        return measure_kernel<MeasureFn<SExtra>>(
            pl, kind, vec,
            [](auto round, auto avg, auto in) { return k_ssim_gen<CSIC_CONST(round), CSIC_CONST(avg), CSIC_CONST(in)>; },
            [](auto round, auto f, auto h, auto v, auto v16, auto nt) {
                return k_ssim_fast<CSIC_CONST(round), CSIC_CONST(f), CSIC_CONST(h), CSIC_CONST(v), CSIC_CONST(v16), CSIC_CONST(nt)>;
            });
    }
};

} // namespace csic

using namespace csic;

extern "C" {

int csic_ssim_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes)
{
    return measure_workspace_bytes<SsimUnit>(plan, nframes, bytes);
}

const char *csic_ssim_kernel_name(const csic_plan *plan)
{
    return plan ? measure_kernel_name(MEASURE_SSIM, measure_kind_of<SsimUnit>(plan), plan->p) : "";
}

int csic_ssim_device(csic_plan *plan, const void *d_in, int32_t nframes, int64_t *d_ssim, int32_t *d_map, void *d_workspace,
                     size_t workspace_bytes, void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    SExtra e{};
    e.map = d_map;
    return measure_device<SsimUnit>(plan, d_in, nframes, d_ssim, d_workspace, workspace_bytes, e, hip_stream);
}

int csic_ssim_host(csic_plan *plan, const uint32_t *in, size_t in_px, int32_t nframes, int64_t *ssim, int32_t *map)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!in || !ssim) return set_error(CSIC_EINVAL_NULL, "host buffer is NULL");
    size_t ws = 0;
    int st = measure_workspace<SsimUnit>(plan, nframes, &ws);
    if (st != CSIC_OK) return st;
    const Geometry &g = plan->g;
    const size_t need = (size_t)nframes * (size_t)g.W * (size_t)g.H;
    if (in_px != need) return set_error(CSIC_EINVAL_SIZE, "expected %zu input pixels (%d frames), got %zu", need, nframes, in_px);
    CSIC_DEVICE_SCOPE(plan->device);
    const size_t ssim_bytes = (size_t)nframes * SSIM_CH * sizeof(int64_t);
    const size_t map_bytes = (size_t)nframes * SSIM_CH * SsimUnit::windows(plan) * sizeof(int32_t);
    DeviceStaging dev;
    void *d_in = dev.alloc(need * 4), *d_ws = dev.alloc(ws), *d_ssim = dev.alloc(ssim_bytes), *d_map = map ? dev.alloc(map_bytes) : nullptr;
    dev.to_device(d_in, in, need * 4);
    if (dev.ok()) {
        st = csic_ssim_device(plan, d_in, nframes, static_cast<int64_t *>(d_ssim), static_cast<int32_t *>(d_map), d_ws, ws, nullptr);
        if (st == CSIC_OK) {
            dev.to_host(ssim, d_ssim, ssim_bytes);
            if (map) dev.to_host(map, d_map, map_bytes);
            dev.sync();
        }
    }
    if (st != CSIC_OK) return st;
    if (!dev.ok()) return set_error(CSIC_EHIP, "csic_ssim_host: %s", hipGetErrorString(dev.error()));
    clear_error();
    return CSIC_OK;
}

} // extern "C"
