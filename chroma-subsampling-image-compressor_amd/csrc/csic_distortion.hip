// csic_distortion.hip -- csic_distortion_device: the per-channel sums of squared errors between input frames and the output their
// plan's parameters produce (R, G, B against the packed ARGB output, Y, Cb, Cr against the packed YCbCr output; input pixel (r, c)
// is paired with output pixel (r / f, c / f); definition in include/csic.h).  Fused: every input byte is read once and the output
// is never written -- only a 48-byte partial per block.
//
// Kernels (wave64, 256-thread blocks; integer byte work, no MFMA, LDS only for the block sum):
//   k_dist_fast<ROUND, F, HH, VV, VEC, NT>  HOLD_DECIMATE, ARGB input, factor F in {1, 2} (chroma before spatial at F = 2; at F = 1
//                      the order classes coincide), width % 4 == 0, height % F == 0.  A "unit" is F input rows x 4 columns: one
//                      16-byte load per row (VEC; four 4-byte loads when d_in is only 4-byte aligned, the packed path's rule), so a
//                      lane holds every input pixel of its unit AND the pixel(s) its output takes Y and held chroma from: the
//                      in-unit chroma hold is a register select (HH in {1, 2, 4} divides 4; at F = 2 the held column 2co & ~(h-1)
//                      is inside the unit too), and only a 4:x:0 odd row at F = 1 needs one more pixel -- the last sample of the row
//                      above, one row-uniform load issued only by waves that sit on such a row (as k_f1flat).  K = 4 / F units per
//                      lane spaced by the block: 16 input pixels per lane, 4096 per block, all loads issued before any arithmetic.
//   k_dist_gen<ROUND, AVG, INFMT>   anything csic_validate accepts: one output pixel per lane (measure_out_pixel: hold_pixel_generic
//                      for HOLD, avg_pixel_generic for AVG), then its f x f input block, clamped at the frame edge.
//   k_sum_partials     (csic_measure.h) one block per frame: the frame's partials, summed in a fixed order, -> d_sse[frame * 6 + channel].
// Which of the two a plan takes is measure_kind (csic_select.cpp); what this unit shares with csic_ssim.hip is csic_measure.h.
// Accumulation widths: a lane sums squared 8-bit errors in 32 bits (it sees at most 64 input pixels -- 16 in k_dist_fast, f * f <= 64
// in k_dist_gen), and so does the wave reduction (at most 64 * 64 = 4096 pixels; 2^32 / 255^2 = 66 051).  The block sum, the partials
// and the per-frame sums are 64-bit.  No atomics: each block writes its own partial with plain vector stores.
#include <cstdio>

#include "csic_measure.h"

namespace csic {

constexpr int DIST_T = MEAS_T;
constexpr int DIST_CH = MEAS_CH;

struct DExtra {
    uint64_t *part;                  // workspace: nblk partials of DIST_CH uint64 per frame, frames back to back
    uint32_t nblk;                   // blocks (= partials) per frame
    uint32_t nunits;                 // k_dist_fast: units per frame; k_dist_gen: output pixels per frame
};

typedef uint64_t CSIC_GLOBAL *gpart_t;

// (R, G, B) of (Y, Cb, Cr) through YCbCrUtils.ycbcr2rgb, as finish_y computes it for the packed ARGB output
struct DRgb { int r, g, b; };
__device__ __forceinline__ DRgb rgb_of(uint32_t y, const ChromaTerm &t)
{
    const Rgb16 o = rgb16_of<8>(y, t);
    return DRgb{(int)o.r, (int)o.g, (int)o.b};
}

__device__ __forceinline__ void sq_add(uint32_t &s, int e) { s += (uint32_t)__mul24(e, e); }

// one input pixel against its output pixel: reference RGB (rr, rg, rb) and YCbCr (ry, rcb, rcr) vs output RGB o and YCbCr (y, cb, cr)
__device__ __forceinline__ void acc_px(uint32_t (&s)[DIST_CH], int rr, int rg, int rb, uint32_t ry, uint32_t rcb, uint32_t rcr,
                                       const DRgb &o, uint32_t y, uint32_t cb, uint32_t cr)
{
    sq_add(s[0], rr - o.r);
    sq_add(s[1], rg - o.g);
    sq_add(s[2], rb - o.b);
    sq_add(s[3], (int)ry - (int)y);
    sq_add(s[4], (int)rcb - (int)cb);
    sq_add(s[5], (int)rcr - (int)cr);
}
__device__ __forceinline__ void acc_argb(uint32_t (&s)[DIST_CH], uint32_t px, uint32_t ry, uint32_t rcb, uint32_t rcr,
                                         const DRgb &o, uint32_t y, uint32_t cb, uint32_t cr)
{
    acc_px(s, (int)((px >> 16) & 0xFFu), (int)((px >> 8) & 0xFFu), (int)(px & 0xFFu), ry, rcb, rcr, o, y, cb, cr);
}

// lane sums -> wave sums (32-bit, see the header) -> this block's 64-bit partial
__device__ __forceinline__ void block_partial(const DExtra &e, uint32_t (&s)[DIST_CH])
{
    __shared__ uint64_t red[DIST_T / 64][DIST_CH];
#pragma unroll
    for (int ch = 0; ch < DIST_CH; ++ch)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[ch] += (uint32_t)__shfl_xor((int)s[ch], off, 64);
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    if (lane == 0)
#pragma unroll
        for (int ch = 0; ch < DIST_CH; ++ch) red[wave][ch] = s[ch];
    __syncthreads();
    if (threadIdx.x < (unsigned)DIST_CH) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < DIST_T / 64; ++w) t += red[w][threadIdx.x];
        CSIC_CHECK(blockIdx.x < e.nblk);
        ((gpart_t)(uintptr_t)e.part)[((uint64_t)blockIdx.z * e.nblk + blockIdx.x) * DIST_CH + threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// k_dist_fast
// ------------------------------------------------------------------------------------------------
template <int ROUND, int F, int HH, int VV, bool VEC, bool NT, bool CHECK>
__device__ __forceinline__ void dist_fast_body(const KArgs &a, gin_t in, uint32_t u0, uint32_t nunits, uint32_t (&s)[DIST_CH])
{
    constexpr int K = 4 / F;
    const uint32_t W = (uint32_t)a.W;
    uint32_t off[K], cpx[K];
    bool odd[K];
    u32x4 p[K][F];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        // the frame's last block: clamp instead of branching, so that every load still issues ahead of the arithmetic
        const uint32_t u = CHECK ? min(u0 + (uint32_t)(k * DIST_T), nunits - 1u) : u0 + (uint32_t)(k * DIST_T);
        const uint32_t j0 = 4u * u;                                         // < 2^30 (measure_kind)
        const uint32_t ur = (uint32_t)(((uint64_t)j0 * a.mW) >> a.kW);      // unit row = j0 / W, exact
        off[k] = F == 1 ? j0 : j0 + __umul24(ur, W);                        // rows F * ur .. : (F * ur) * W + (j0 - ur * W)
        odd[k] = F == 1 && VV == 2 && (ur & 1u);
        cpx[k] = 0;
        if constexpr (F == 1 && VV == 2) {
            // 4:x:0 odd row: every pixel holds the chroma latched at the last sample of the row above (ChromaSubsampler.scala:52-65)
            if (__builtin_amdgcn_ballot_w64(odd[k]) != 0)
                cpx[k] = in1n<false>(a, in, odd[k] ? __umul24(ur - 1u, W) + (uint32_t)a.last_sample_col : off[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < F; ++i) p[k][i] = in4n_or_1n<VEC, NT>(a, in, off[k] + (uint32_t)i * W);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (CHECK && u0 + (uint32_t)(k * DIST_T) >= nunits) continue;
        const uint32_t q0[4] = {p[k][0].x, p[k][0].y, p[k][0].z, p[k][0].w};
        uint32_t ry[4], rcb[4], rcr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { ry[i] = fwd_y(q0[i]); fwd_c<ROUND>(q0[i], rcb[i], rcr[i]); }
        if constexpr (F == 1) {
            uint32_t ocb = 0, ocr = 0;
            if (VV == 2) fwd_c<ROUND>(cpx[k], ocb, ocr);
#pragma unroll
            for (int g = 0; g < 4; g += HH) {
                const uint32_t cb = ((VV == 2 && odd[k]) ? ocb : rcb[g]) & a.mcb;     // held chroma, quantised
                const uint32_t cr = ((VV == 2 && odd[k]) ? ocr : rcr[g]) & a.mcr;
                const ChromaTerm t = chroma_term_q<F_ARGB>(cb, cr);
#pragma unroll
                for (int i = g; i < g + HH; ++i) {
                    const uint32_t y = ry[i] & a.my;
                    acc_argb(s, q0[i], ry[i], rcb[i], rcr[i], rgb_of(y, t), y, cb, cr);
                }
            }
        } else {
            const uint32_t q1[4] = {p[k][1].x, p[k][1].y, p[k][1].z, p[k][1].w};
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                // output (ro, co) = (ur, 2 ug + o): Y of input column 2 co = unit column 2 o; chroma held from column 2 co & ~(h - 1)
                const int src = HH == 4 ? 0 : 2 * o;
                const uint32_t y = ry[2 * o] & a.my, cb = rcb[src] & a.mcb, cr = rcr[src] & a.mcr;
                const DRgb rgb = rgb_of(y, chroma_term_q<F_ARGB>(cb, cr));
#pragma unroll
                for (int i = 2 * o; i < 2 * o + 2; ++i) {
                    acc_argb(s, q0[i], ry[i], rcb[i], rcr[i], rgb, y, cb, cr);
                    uint32_t b1, c1;
                    fwd_c<ROUND>(q1[i], b1, c1);
                    acc_argb(s, q1[i], fwd_y(q1[i]), b1, c1, rgb, y, cb, cr);
                }
            }
        }
    }
}

template <int ROUND, int F, int HH, int VV, bool VEC, bool NT>
__global__ void __launch_bounds__(DIST_T) k_dist_fast(KArgs a, DExtra e)
{
    pin_args(a);
    const gin_t in = frame_in(a);
    constexpr uint32_t per_block = DIST_T * (4 / F);
    const uint32_t b0 = blockIdx.x * per_block;
    uint32_t s[DIST_CH] = {0, 0, 0, 0, 0, 0};
    if (b0 + per_block <= e.nunits) dist_fast_body<ROUND, F, HH, VV, VEC, NT, false>(a, in, b0 + threadIdx.x, e.nunits, s);
    else                            dist_fast_body<ROUND, F, HH, VV, VEC, NT, true>(a, in, b0 + threadIdx.x, e.nunits, s);
    block_partial(e, s);
}

// ------------------------------------------------------------------------------------------------
// k_dist_gen
// ------------------------------------------------------------------------------------------------
template <int ROUND, bool AVG, int INFMT>
__global__ void __launch_bounds__(DIST_T) k_dist_gen(KArgs a, DExtra e)
{
    pin_args(a);
    const gin_t in = frame_in(a);
    const uint32_t j = blockIdx.x * (uint32_t)DIST_T + threadIdx.x;
    uint32_t s[DIST_CH] = {0, 0, 0, 0, 0, 0};
    if (j < e.nunits) {
        const int ro = (int)(((uint64_t)j * a.mWo) >> a.kWo), co = (int)j - ro * a.Wo;      // j / Wo, exact for j < 2^31
        const Ycc o = measure_out_pixel<ROUND, AVG, INFMT>(a, in, ro, co);                  // the output pixel, packed-YCbCr values
        const uint32_t y = o.y, cb = o.cb, cr = o.cr;
        const DRgb rgb = rgb_of(y, chroma_term_q<F_ARGB>(cb, cr));
        const int r0 = ro * a.f, c0 = co * a.f, r1 = min(r0 + a.f, a.H), c1 = min(c0 + a.f, a.W);
        for (int r = r0; r < r1; ++r) {
            for (int c = c0; c < c1; ++c) {
                uint32_t ref[DIST_CH];
                ref_channels<ROUND, INFMT>(in1<false>(a, in, (int64_t)r * a.ip + c), ref);
                acc_px(s, (int)ref[0], (int)ref[1], (int)ref[2], ref[3], ref[4], ref[5], rgb, y, cb, cr);
            }
        }
    }
    block_partial(e, s);
}

// ------------------------------------------------------------------------------------------------
// host side: what csic_measure.h asks of a unit
// ------------------------------------------------------------------------------------------------
struct DistUnit {
    typedef DExtra Extra;
    static constexpr MeasureFamily family = MEASURE_DIST;
    static constexpr const char *result_name = "d_sse", *workspace_fn = "csic_distortion_workspace_bytes";
    static int check_plan(const csic_plan *) { return CSIC_OK; }
    static int check_extra(const DExtra &) { return CSIC_OK; }
    // k_dist_fast: units per frame; k_dist_gen: output pixels per frame
    static uint32_t units(const csic_plan *pl, int kind)
    {
        const Geometry &g = pl->g;
        if (kind == 0) return (uint32_t)((int64_t)g.Wo * g.Ho);
        return (uint32_t)((int64_t)(g.W / 4) * (g.H / kind));
    }
    static uint32_t blocks(const csic_plan *pl, int kind)
    {
        const int64_t per_block = kind == 0 ? DIST_T : (int64_t)DIST_T * (4 / kind);
        return (uint32_t)((units(pl, kind) + per_block - 1) / per_block);
    }
    static void fill_extra(const csic_plan *pl, int kind, DExtra *e) { e->nunits = units(pl, kind); }
    static MeasureFn<DExtra> kernel(const csic_plan *pl, int kind, bool vec)
    {
        return measure_kernel<MeasureFn<DExtra>>(
            pl, kind, vec,
            [](auto round, auto avg, auto in) { return k_dist_gen<CSIC_CONST(round), CSIC_CONST(avg), CSIC_CONST(in)>; },
            [](auto round, auto f, auto h, auto v, auto v16, auto nt) {
                return k_dist_fast<CSIC_CONST(round), CSIC_CONST(f), CSIC_CONST(h), CSIC_CONST(v), CSIC_CONST(v16), CSIC_CONST(nt)>;
            });
    }
};

} // namespace csic

using namespace csic;

extern "C" {

int csic_distortion_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes)
{
    return measure_workspace_bytes<DistUnit>(plan, nframes, bytes);
}

const char *csic_distortion_kernel_name(const csic_plan *plan)
{
    return plan ? measure_kernel_name(MEASURE_DIST, measure_kind_of<DistUnit>(plan), plan->p) : "";
}

int csic_distortion_device(csic_plan *plan, const void *d_in, int32_t nframes, uint64_t *d_sse, void *d_workspace,
                           size_t workspace_bytes, void *hip_stream)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    return measure_device<DistUnit>(plan, d_in, nframes, d_sse, d_workspace, workspace_bytes, DExtra{}, hip_stream);
}

int csic_distortion_host(csic_plan *plan, const uint32_t *in, size_t in_px, int32_t nframes, uint64_t *sse)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!in || !sse) return set_error(CSIC_EINVAL_NULL, "host buffer is NULL");
    size_t ws = 0;
    int st = measure_workspace<DistUnit>(plan, nframes, &ws);
    if (st != CSIC_OK) return st;
    const Geometry &g = plan->g;
    const size_t need = (size_t)nframes * (size_t)g.W * (size_t)g.H;
    if (in_px != need) return set_error(CSIC_EINVAL_SIZE, "expected %zu input pixels (%d frames), got %zu", need, nframes, in_px);
    CSIC_DEVICE_SCOPE(plan->device);
    const size_t sse_bytes = (size_t)nframes * DIST_CH * sizeof(uint64_t);
    DeviceStaging dev;
    void *d_in = dev.alloc(need * 4), *d_ws = dev.alloc(ws), *d_sse = dev.alloc(sse_bytes);
    dev.to_device(d_in, in, need * 4);
    if (dev.ok()) {
        st = csic_distortion_device(plan, d_in, nframes, static_cast<uint64_t *>(d_sse), d_ws, ws, nullptr);
        if (st == CSIC_OK) { dev.to_host(sse, d_sse, sse_bytes); dev.sync(); }
    }
    if (st != CSIC_OK) return st;
    if (!dev.ok()) return set_error(CSIC_EHIP, "csic_distortion_host: %s", hipGetErrorString(dev.error()));
    clear_error();
    return CSIC_OK;
}

} // extern "C"
