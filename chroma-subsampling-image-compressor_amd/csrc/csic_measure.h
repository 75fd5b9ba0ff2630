// csic_measure.h -- what the measurement units (csic_distortion.hip, csic_ssim.hip) share.  Both measure the six channels R, G, B
// (against the packed ARGB output) and Y, Cb, Cr (against the packed YCbCr output) of input pixel (r, c) against output pixel
// (r / f, c / f) without writing the output, both have a fast kernel for the class measure_kind (csic_select.cpp) names and a
// general one-output-pixel-at-a-time kernel for everything else, and both leave one 48-byte partial per block that a second
// launch sums.  Device side: the output pixel and the reference channels of the general kernels, the fast kernels' load, the
// clamped inverse transform, the sum of the partials.  Host side: kernel pick, workspace size, the checked two-launch sequence.
// What differs stays in the units: DExtra / SExtra, block_partial / ssim_finish, the four pixel kernels, the SSIM window arithmetic.
#pragma once
#include <cstring>

#include "csic_kernel_ops.h"

namespace csic {

constexpr int MEAS_T = 256;                      // threads per block, every measurement kernel
constexpr int MEAS_CH = CSIC_DIST_CHANNELS;      // R, G, B, Y, Cb, Cr

// ------------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------------
// output pixel (ro, co) of any plan csic_validate accepts, as the packed YCbCr output holds it (k_dist_gen)
template <int ROUND, bool AVG, int INFMT>
__device__ __forceinline__ Ycc measure_out_pixel(const KArgs &a, gin_t in, int ro, int co)
{
    if (AVG) {
        const uint32_t o = avg_pixel_generic<ROUND, F_YCC, INFMT>(a, in, ro, co);
        return Ycc{o & 0xFFu, (o >> 8) & 0xFFu, (o >> 16) & 0xFFu};
    }
    return hold_pixel_generic<ROUND, INFMT>(a, in, ro, co);
}

// the clamped 16-bit (R, G, B) << 8 of (Y, chroma): byte 1 of each is the packed ARGB output's channel (finish_y).  SHIFT = 8
// gives the channels themselves (the shift sits here, next to its clamp, so that csic_distortion.hip compiles to what it was)
struct Rgb16 { uint32_t r, g, b; };
template <int SHIFT = 0>
__device__ __forceinline__ Rgb16 rgb16_of(uint32_t y, const ChromaTerm &t)
{
    const int yy = __mul24((int)y, 298);
    return Rgb16{(uint32_t)(min(max(yy + t.kr, 0), 65535) >> SHIFT), (uint32_t)(min(max(yy + t.kg, 0), 65535) >> SHIFT),
                 (uint32_t)(min(max(yy + t.kb, 0), 65535) >> SHIFT)};
}

// the reference of one input pixel in the six channels: an ARGB pixel's own R, G, B and its forward transform; a YCbCr pixel's
// own Y, Cb, Cr and their inverse transform.  Y_FIRST only orders the two halves of the forward transform: each unit keeps the
// order its general kernel had, and with it that kernel's instruction schedule
template <int ROUND, int INFMT, bool Y_FIRST = false>
__device__ __forceinline__ void ref_channels(uint32_t px, uint32_t (&ref)[MEAS_CH])
{
    if (INFMT == F_YCC) {
        ref[3] = px & 0xFFu; ref[4] = (px >> 8) & 0xFFu; ref[5] = (px >> 16) & 0xFFu;
        const Rgb16 o = rgb16_of(ref[3], chroma_term_q<F_ARGB>(ref[4], ref[5]));
        ref[0] = o.r >> 8; ref[1] = o.g >> 8; ref[2] = o.b >> 8;
    } else {
        ref[0] = (px >> 16) & 0xFFu; ref[1] = (px >> 8) & 0xFFu; ref[2] = px & 0xFFu;
        if (Y_FIRST) ref[3] = fwd_y(px);
        fwd_c<ROUND>(px, ref[4], ref[5]);
        if (!Y_FIRST) ref[3] = fwd_y(px);
    }
}

// four consecutive input pixels: one 16-byte load, or four 4-byte loads for a d_in that is only 4-byte aligned
template <bool VEC, bool NT>
__device__ __forceinline__ u32x4 in4n_or_1n(const KArgs &a, gin_t in, uint32_t off)
{
    if (VEC) return in4n<NT>(a, in, off);
    const u32x4 v = {in1n<NT>(a, in, off), in1n<NT>(a, in, off + 1u), in1n<NT>(a, in, off + 2u), in1n<NT>(a, in, off + 3u)};
    return v;
}

// One block per frame: frame blockIdx.x's nblk partials of MEAS_CH 64-bit words, summed in a fixed order (so that a result does
// not depend on how the blocks were scheduled), -> sums[frame * MEAS_CH + channel].  The words are SSE partials (uint64_t) or
// SSIM partials (int64_t, possibly negative): two's-complement addition is the same instruction for both, so one element type
// serves.  CH words per partial, and frame z's sums at sums[z * STRIDE]: the two measurement units have CH = STRIDE = MEAS_CH, the
// quantiser sweep (csic_qsweep.hip) 24 words into a larger per-frame result.
template <int CH, int STRIDE>
__device__ __forceinline__ void sum_partials(const uint64_t *part, uint32_t nblk, uint64_t *sums)
{
    typedef const uint64_t CSIC_GLOBAL *gcpart_t;
    typedef uint64_t CSIC_GLOBAL *gsum_t;
    const gcpart_t p = (gcpart_t)(uintptr_t)part + (uint64_t)blockIdx.x * nblk * CH;
    uint64_t t[CH] = {};
    for (uint32_t b = threadIdx.x; b < nblk; b += MEAS_T)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) t[ch] += p[(uint64_t)b * CH + ch];
    __shared__ uint64_t red[MEAS_T][CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) red[threadIdx.x][ch] = t[ch];
    __syncthreads();
    for (int w = MEAS_T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) red[threadIdx.x][ch] += red[threadIdx.x + w][ch];
        __syncthreads();
    }
    if (threadIdx.x < (unsigned)CH) ((gsum_t)(uintptr_t)sums)[(uint64_t)blockIdx.x * STRIDE + threadIdx.x] = red[0][threadIdx.x];
}

// `static`: each unit compiles its own copy into its own code object (csic_qsweep.hip, which has its own width, none).
__attribute__((unused)) static __global__ void __launch_bounds__(MEAS_T) k_sum_partials(const uint64_t *part, uint32_t nblk, uint64_t *sums)
{
    sum_partials<MEAS_CH, MEAS_CH>(part, nblk, sums);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// A unit describes itself by a struct U with
//   typedef ... Extra;                               the second kernel argument; measure_device sets its members `part` (the
//                                                    workspace, 8-byte words) and `nblk` (uint32_t)
//   static constexpr MeasureFamily family;           for measure_kind / measure_kernel_name
//   static const char *result_name, *workspace_fn;   as the error texts name the result pointer and the size function
//   static int check_plan(const csic_plan *);        what the unit asks of a plan beyond csic_validate
//   static uint32_t blocks(const csic_plan *, int kind);     blocks (= partials) per frame
//   static MeasureFn<Extra> kernel(const csic_plan *, int kind, bool vec);
//   static int check_extra(const Extra &);           the unit's own pointers, which the entry point has put into its Extra
//   static void fill_extra(const csic_plan *, int kind, Extra *);    the unit's geometry members
template <class Extra> using MeasureFn = void (*)(KArgs, Extra);

template <class U> int measure_kind_of(const csic_plan *pl) { return measure_kind(pl->p, pl->g, pl->tune, U::family); }

// The kernel of a plan: `kind` from measure_kind, `vec` = 16-byte loads.  gen(round, avg, in) and fast(round, f, h, v, v16, nt)
// return the unit's instantiation for those constants.
template <class Fn, class Gen, class Fast>
Fn measure_kernel(const csic_plan *pl, int kind, bool vec, Gen gen, Fast fast)
{
    const csic_params &p = pl->p;
    const Geometry &g = pl->g;
    return with_const<R_FLOOR, R_TRUNC>(p.rounding, [&](auto round) -> Fn {
        if (kind == 0)
            return with_const<true, false>(p.sampling == CSIC_SAMPLING_AVG, [&](auto avg) {
                return with_const<F_YCC, F_ARGB>(p.in_format, [&](auto in) -> Fn { return gen(round, avg, in); });
            });
        return with_const<true, false>(vec, [&](auto v16) {
        return with_const<true, false>(!pl->tune.no_nt, [&](auto nt) {
        return with_const<1, 2>(kind, [&](auto f) {
        return with_const<1, 2, 4>(g.h, [&](auto h) -> Fn {
            // at F = 2 the output rows are sample rows: v does not matter, and only V = 1 exists
            if constexpr (CSIC_CONST(f) == 2) return fast(round, f, h, std::integral_constant<int, 1>{}, v16, nt);
            else return with_const<2, 1>(g.v, [&](auto v) -> Fn { return fast(round, f, h, v, v16, nt); });
        }); }); }); });
    });
}

template <class U> int measure_workspace(const csic_plan *pl, int32_t nframes, size_t *bytes)
{
    if (nframes <= 0 || nframes > 65535)
        return set_error(CSIC_EINVAL_SIZE, "nframes must be in 1..65535. Got %d", nframes);
    const int st = U::check_plan(pl);
    if (st != CSIC_OK) return st;
    *bytes = (size_t)nframes * U::blocks(pl, measure_kind_of<U>(pl)) * MEAS_CH * sizeof(uint64_t);
    return CSIC_OK;
}

// csic_*_workspace_bytes
template <class U> int measure_workspace_bytes(const csic_plan *plan, int32_t nframes, size_t *bytes)
{
    if (!plan || !bytes) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    const int st = measure_workspace<U>(plan, nframes, bytes);
    if (st == CSIC_OK) clear_error();
    return st;
}

// csic_*_device: the checks, the pixel kernel over (blocks, 1, nframes), then k_sum_partials over the frames.  `e` arrives zeroed
// but for the unit's own pointers.
template <class U>
int measure_device(csic_plan *plan, const void *d_in, int32_t nframes, void *d_result, void *d_workspace, size_t workspace_bytes,
                   typename U::Extra e, void *hip_stream)
{
    if (!d_in || !d_result || !d_workspace) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    size_t need = 0;
    const int st = measure_workspace<U>(plan, nframes, &need);
    if (st != CSIC_OK) return st;
    if (workspace_bytes < need)
        return set_error(CSIC_EINVAL_SIZE, "workspace of %zu bytes is smaller than the %zu bytes %s asks for", workspace_bytes, need,
                         U::workspace_fn);
    if ((uintptr_t)d_result & 7u) return set_error(CSIC_EINVAL_SIZE, "%s must be 8-byte aligned", U::result_name);
    if ((uintptr_t)d_workspace & 7u) return set_error(CSIC_EINVAL_SIZE, "the workspace must be 8-byte aligned");
    const int est = U::check_extra(e);
    if (est != CSIC_OK) return est;
    if ((uintptr_t)d_in & 3u) return set_error(CSIC_EINVAL_SIZE, "the input must be 4-byte aligned");
    const Geometry &g = plan->g;
    const int kind = measure_kind_of<U>(plan);
    // 16-byte loads only for a 16-byte aligned d_in (the frame stride W * H * 4 is a multiple of 16 whenever width % 4 == 0)
    const bool vec = ((uintptr_t)d_in & 15u) == 0 && !plan->tune.no_vec;
    const MeasureFn<typename U::Extra> fn = U::kernel(plan, kind, vec);
    CSIC_DEVICE_SCOPE(plan->device);
    KArgs a;
    fill_base_args(g, g.W, g.Wo, &a);
    a.in = static_cast<const uint32_t *>(d_in);
    a.bdx = MEAS_T; a.bdy = 1; a.row_step = 1;
    e.part = static_cast<decltype(e.part)>(d_workspace);
    e.nblk = U::blocks(plan, kind);
    U::fill_extra(plan, kind, &e);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    int lst = launch(fn, dim3(e.nblk, 1, (unsigned)nframes), dim3(MEAS_T, 1, 1), stream, a, e);
    if (lst == CSIC_OK)
        lst = launch(k_sum_partials, dim3((unsigned)nframes, 1, 1), dim3(MEAS_T, 1, 1), stream, static_cast<const uint64_t *>(d_workspace), e.nblk,
                     static_cast<uint64_t *>(d_result));
    if (lst != CSIC_OK) return lst;
    clear_error();
    return CSIC_OK;
}

} // namespace csic
